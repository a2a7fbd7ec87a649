"""Golden vectors for EmergencyResponseEnv, produced by running the reference's own emergency_response_env/emergency_env.py (unmodified,
imported from the reference checkout under the stub gymnasium / pygame).  Run it in a process of its own.

Seeding protocol: the env draws from the global `random` only (`random`, `uniform`, `randint`) and never seeds it (`super().reset(seed=)`
seeds the unused np_random), so env i is `random.seed(seed0 + i)`, `EmergencyResponseEnv()` and then `env.reset(seed=seed0 + i)`.
Unlike the airline env the constructor does NOT call reset().  It draws, in order, 900 `randint` for `population_density` (rows 0-9 and
21-29 `randint(100, 300)`, rows 10-15 `randint(50, 500)`, rows 16-20 `randint(20, 100)`), 20 `randint(5, 25)` for the stations of units
30-39 and 32 `randint` for the eight hospitals (`(50, 150)`, `(10, 30)`, `(80, 200)`, `(15, 40)` each).  `randint` goes through
`_randbelow_with_getrandbits`, so the number of generator words consumed varies with the rejections.  On `terminated` the terminal
observation is recorded and `env.reset()` continues the same stream and keeps the network (auto-reset) — and `_prev_resolved`,
`_prev_lives_saved`, `_prev_casualties`, which reset() does not touch; `emergency_overrun` never resets and steps the reference on
past `terminated`.  `emergency_timeout` sets `env.max_timesteps = 90` after construction: a random policy never survives 1,440 steps.

The hospital distance sums are Python's sum() of floats, which Python 3.12 and later compensate: the fixtures are those of a plain
left-to-right sum, so this script refuses to run there.

Policies: "hash" = the counter hash over 0..49; "dispatch" = hashed over 0..19 three steps out of four, otherwise over 20..49;
"idle" = action 49 only.
The event counters are taken by watching the env from outside: its methods are wrapped per instance, its code is not touched.
`obs_xor` is the per-step observation as uint32 bit patterns [env, element, step], each step XORed with the step before it;
emergency_model.fixture_obs() undoes it.  `info` holds the six info values, `termination_reason` as a code (0 none, 1 success,
2 casualties, 3 overwhelmed, 4 timeout).
Outputs: tests/golden/emergency_hash.npz, emergency_dispatch.npz, emergency_idle.npz, emergency_timeout.npz, emergency_overrun.npz (RUNS)
and emergency_day.npz (NEW_RUNS; `python gen_emergency.py --new` writes it alone and leaves the others' bytes as they are): like
emergency_overrun it never resets, and it runs on to 22:10 on the env's clock, through every arm of the traffic's hour-of-day chain.
"""
import json
import os
import random
import sys

import numpy as np

import common

assert sys.version_info < (3, 12), "Python 3.12+ sums floats with compensation: the distance sums would not be the recorded left-to-right sums"

common.use_stubs()
common.add_reference_dir("emergency_response_env")
from emergency_env import EmergencyResponseEnv  # noqa: E402  (reference code)

INFO = ("active_emergencies", "total_casualties", "lives_saved", "emergencies_resolved", "avg_response_time", "termination_reason")
REASONS = {None: 0, "success": 1, "casualties": 2, "overwhelmed": 3, "timeout": 4}
EVENTS = ("success", "casualties", "overwhelmed", "timeout", "escalations", "cascades", "mutual_aid", "national_guard", "gridlock", "quick_response",
          "escalated_after_work", "full", "prev_carried", "resolved", "overallocated")
# counted in the runs of NEW_RUNS only (the older files' `events` have the keys above): steps by the hour-of-day arm of :787-792
NEW_EVENTS = ("hour_night_early", "hour_before_rush", "hour_rush_morning", "hour_midday", "hour_rush_evening", "hour_evening", "hour_night_late")
OBS = 276


def action(policy, a_seed, i, t):
    if policy == "dispatch":
        return common.hash_action(a_seed, i, t, 20) if t % 4 != 3 else 20 + common.hash_action(a_seed, i, t, 30)
    if policy == "idle":
        return 49
    return common.hash_action(a_seed, i, t, 50)


def xor_time(obs):
    """float32 [n, T, 276] -> uint32 [n, 276, T], every step XORed with its predecessor (np.bitwise_xor.accumulate along the last axis undoes it)"""
    x = np.ascontiguousarray(obs.transpose(0, 2, 1)).view(np.uint32).copy()
    x[:, :, 1:] ^= x[:, :, :-1].copy()
    return x


def watch(env, ev):
    """count what the fixtures are for, from outside the env"""
    worked = set()
    escalate, cascade, work = env._escalate_emergency, env._trigger_cascade_event, env._work_on_incident
    mutual, guard = env._add_mutual_aid_units, env._add_national_guard_units

    def _escalate(incident):
        ev["escalations"] += 1
        ev["escalated_after_work"] += id(incident) in worked
        return escalate(incident)

    def _cascade(incident):
        before = len(env.active_emergencies)
        cascade(incident)
        ev["cascades"] += len(env.active_emergencies) - before

    def _work(unit, incident):
        before = incident.severity
        work(unit, incident)
        if incident.severity < before:
            worked.add(id(incident))

    def _mutual():
        ev["mutual_aid"] += 1
        return mutual()

    def _guard():
        ev["national_guard"] += 1
        return guard()

    env._escalate_emergency, env._trigger_cascade_event, env._work_on_incident = _escalate, _cascade, _work
    env._add_mutual_aid_units, env._add_national_guard_units = _mutual, _guard
    return worked


def run_env(seed, T, a_seed, i, policy, autoreset, ev, max_timesteps=None):
    random.seed(seed)
    env = EmergencyResponseEnv()
    if max_timesteps is not None:
        env.max_timesteps = max_timesteps
    worked = watch(env, ev)
    obs, info = env.reset(seed=seed)
    assert info == {}
    out = dict(obs0=obs, A=np.zeros(T, np.int8), R=np.zeros(T, np.float64), TM=np.zeros(T, np.uint8), I=np.zeros((T, 6), np.float64),
               O=np.zeros((T, OBS), np.float32), resets=[])
    for t in range(T):
        a = action(policy, a_seed, i, t)
        resolved = env.emergencies_resolved
        if "hour_midday" in ev:
            hour = (env.current_timestep // 60) % 24
            ev["hour_night_early" if hour <= 5 else "hour_before_rush" if hour < 7 else "hour_rush_morning" if hour <= 9 else "hour_midday" if hour < 17
               else "hour_rush_evening" if hour <= 19 else "hour_evening" if hour < 22 else "hour_night_late"] += 1
        obs, rew, term, trunc, info = env.step(a)
        assert not trunc and obs.dtype == np.float32 and rew == int(rew) and list(info) == list(INFO)
        ev["gridlock"] += bool(np.mean(env.traffic_congestion) > 0.8)
        ev["quick_response"] += bool(env.response_times and env.response_times[-1] <= 15)
        ev["full"] += len(env.active_emergencies) == 20
        ev["resolved"] += env.emergencies_resolved - resolved
        ev["overallocated"] += sum(len(inc.active_units) > sum(inc.required_units.values()) * 1.5 for inc in env.active_emergencies.values())
        out["A"][t] = a; out["R"][t] = rew; out["TM"][t] = term; out["O"][t] = obs
        out["I"][t] = [float(info[k]) for k in INFO[:5]] + [REASONS[info["termination_reason"]]]
        if term:
            assert info["termination_reason"] in REASONS
        if term and autoreset:
            ev[info["termination_reason"]] += 1
            ev["prev_carried"] += bool(env._prev_resolved or env._prev_lives_saved or env._prev_casualties)
            worked.clear()
            obs, _ = env.reset()
            out["resets"].append((t, obs))
    return env, out


def make(name, n_envs, T, seed0, a_seed, policy, autoreset=True, max_timesteps=None):
    ev = dict.fromkeys(EVENTS + (NEW_EVENTS if name in NEW_RUNS else ()), 0)
    rows = [run_env(seed0 + i, T, a_seed, i, policy, autoreset, ev, max_timesteps) for i in range(n_envs)]
    env = rows[0][0]
    rows = [r[1] for r in rows]
    ridx = [(i, t) for i, r in enumerate(rows) for t, _ in r["resets"]]
    sp = dict(action=dict(kind=type(env.action_space).__name__, n=int(env.action_space.n)),
              observation=dict(kind=type(env.observation_space).__name__, shape=list(env.observation_space.shape), dtype=str(env.observation_space.dtype),
                               low=float(env.observation_space.low.min()), high=float(env.observation_space.high.max())))
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), autoreset=np.int64(autoreset),
                  max_timesteps=np.int64(env.max_timesteps),
                  actions=np.stack([r["A"] for r in rows]), obs0=np.stack([r["obs0"] for r in rows]), obs_xor=xor_time(np.stack([r["O"] for r in rows])),
                  reward=np.stack([r["R"] for r in rows]), terminated=np.stack([r["TM"] for r in rows]), info=np.stack([r["I"] for r in rows]),
                  info_keys=np.array(json.dumps(INFO)), reset_index=np.array(ridx, np.int32).reshape(-1, 2),
                  reset_obs=np.array([ob for r in rows for _, ob in r["resets"]], np.float32).reshape(-1, OBS),
                  spaces=np.array(json.dumps(sp)), events=np.array(json.dumps(ev)), versions=np.array(json.dumps(common.versions())))
    return arrays, ev


def save(name, arrays):
    out = os.path.join(common.GOLDEN, name + ".npz")
    np.savez_compressed(out, **arrays)
    print(name, "ends", len(arrays["reset_index"]), "sum reward", arrays["reward"].sum(), "events", str(arrays["events"]), os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1 << 20, "a committed file stays under 1 MiB"


# seed0 / a_seed: found by a search on the CPU for runs in which episodes end in "success" (about one per 16 x 150 run otherwise)
RUNS = dict(emergency_hash=dict(n_envs=16, T=150, seed0=2944, a_seed=301, policy="hash"),
            emergency_dispatch=dict(n_envs=16, T=150, seed0=5684, a_seed=302, policy="dispatch"),
            emergency_idle=dict(n_envs=16, T=200, seed0=2232, a_seed=303, policy="idle"),
            emergency_timeout=dict(n_envs=16, T=150, seed0=2636, a_seed=304, policy="dispatch", max_timesteps=90),
            emergency_overrun=dict(n_envs=8, T=300, seed0=2400, a_seed=305, policy="hash", autoreset=False))
# recorded later than RUNS, for the branches of csrc/emergency_env.hpp that those leave unentered (tests/test_lane_env_branch_coverage.py)
NEW_RUNS = dict(emergency_day=dict(n_envs=4, T=1330, seed0=3000, a_seed=306, policy="dispatch", autoreset=False))


def check_new(name, ev):
    if name == "emergency_day":
        return min(ev[k] for k in NEW_EVENTS if k.startswith("hour_")) >= 4 * 10
    return True


def check(evs):
    """the conditions the fixtures are recorded for (tests/test_emergency_cpu.py asserts them again)"""
    auto = [evs[k] for k in ("emergency_hash", "emergency_dispatch", "emergency_idle", "emergency_timeout")]
    tot = {k: sum(e[k] for e in auto) for k in EVENTS}
    every = {k: tot[k] + evs["emergency_overrun"][k] for k in EVENTS}
    assert min(tot[k] for k in ("success", "casualties", "overwhelmed", "timeout")) >= 8, tot
    assert every["escalations"] >= 30 and every["cascades"] >= 20 and every["mutual_aid"] >= 3 and every["national_guard"] >= 3, every
    assert every["gridlock"] >= 20 and every["quick_response"] >= 20 and every["escalated_after_work"] >= 1 and every["full"] >= 1, every
    assert tot["prev_carried"] >= 1, tot


if __name__ == "__main__":
    if "--new" in sys.argv[1:]:
        made = {name: make(name, **kw) for name, kw in NEW_RUNS.items()}
        for name, (_, ev) in made.items():
            assert check_new(name, ev), (name, ev)
        for name, (arrays, _) in made.items():
            save(name, arrays)
        sys.exit(0)
    made = {name: make(name, **kw) for name, kw in RUNS.items()}
    check({name: ev for name, (_, ev) in made.items()})                   # nothing is written unless the runs hold what they are for
    for name, (arrays, _) in made.items():
        save(name, arrays)
