"""Golden vectors for AirlineOperationsEnv, produced by running the reference's own airline_operations_env/airline_env.py (unmodified,
imported from the reference checkout under the stub gymnasium / pygame).  Run it in a process of its own.

Protocol: the env draws from the global `random` only and never seeds it (`super().reset(seed=)` seeds the unused np_random), so env
i is `random.seed(seed0 + i)`, `AirlineOperationsEnv()` — whose constructor draws the network and one reset of its own — and then
`env.reset(seed=seed0 + i)`.  On `terminated` the terminal observation is recorded and `env.reset()` continues the same stream and
keeps the network (auto-reset); `airline_overrun` never resets and steps the reference on past `terminated`.

`fuel_costs` is Python's sum() of floats, which Python 3.12 and later compensate: the fixtures are those of a plain left-to-right sum,
so this script refuses to run there.

Policies: "hash" = the counter hash over 0..44; "dispatch" = hashed over 0..24 three steps out of four, otherwise over 35..44;
"cancel" = hashed over 25..34.
`obs_xor` is the per-step observation as uint32 bit patterns [env, element, step], each step XORed with the step before it (an
element's run over time is mostly constant, so most words are zero and the file stays small); airline_model.fixture_obs() undoes it.
Outputs: tests/golden/airline_hash.npz, airline_dispatch.npz, airline_cancel.npz, airline_overrun.npz.
"""
import json
import os
import random
import sys

import numpy as np

import common

assert sys.version_info < (3, 12), "Python 3.12+ sums floats with compensation: fuel_costs would not be the recorded left-to-right sum"

common.use_stubs()
common.add_reference_dir("airline_operations_env")
from airline_env import AirlineOperationsEnv  # noqa: E402  (reference code)

INFO = ("on_time_performance", "passenger_satisfaction", "daily_revenue", "daily_costs", "current_hour")
EVENTS = ("end_clock", "end_satisfaction", "delayed_on_time", "a41_accepted", "a41_refused", "wraps", "maintenance", "fuel_floor")


def action(policy, a_seed, i, t):
    if policy == "dispatch":
        return common.hash_action(a_seed, i, t, 25) if t % 4 != 3 else 35 + common.hash_action(a_seed, i, t, 10)
    if policy == "cancel":
        return 25 + common.hash_action(a_seed, i, t, 10)
    return common.hash_action(a_seed, i, t, 45)


def xor_time(obs):
    """float32 [n, T, 160] -> uint32 [n, 160, T], every step XORed with its predecessor (np.bitwise_xor.accumulate along the last axis undoes it)"""
    x = np.ascontiguousarray(obs.transpose(0, 2, 1)).view(np.uint32).copy()
    x[:, :, 1:] ^= x[:, :, :-1].copy()
    return x


def run_env(seed, T, a_seed, i, policy, autoreset, ev):
    random.seed(seed)
    env = AirlineOperationsEnv()
    obs, info = env.reset(seed=seed)
    assert list(info) == list(INFO)
    out = dict(obs0=obs, A=np.zeros(T, np.int8), R=np.zeros(T, np.float64), TM=np.zeros(T, np.uint8), I=np.zeros((T, 5), np.float64),
               O=np.zeros((T, 160), np.float32), resets=[], wraps=0, ends=[0, 0])
    for t in range(T):
        a = action(policy, a_seed, i, t)
        costs, hour = env.daily_costs, env.current_hour
        maint = sum(ac.delay_minutes for ac in env.aircraft)
        ground = sum(not ac.in_flight for ac in env.aircraft)
        obs, rew, term, trunc, info = env.step(a)
        assert not trunc and obs.dtype == np.float32 and rew == int(rew) and list(info) == list(INFO)
        if a == 41:
            ev["a41_accepted" if costs < 500000 else "a41_refused"] += 1
        wrapped = env.current_hour < hour
        out["wraps"] += wrapped
        ev["wraps"] += wrapped
        ev["maintenance"] += (sum(ac.delay_minutes for ac in env.aircraft) - maint - (30 * ground if a == 43 else 0)) // 120
        ev["fuel_floor"] += any(ac.fuel_level == 0.1 for ac in env.aircraft)
        out["A"][t] = a; out["R"][t] = rew; out["TM"][t] = term; out["O"][t] = obs
        out["I"][t] = [info[k] for k in INFO]
        if term and autoreset:
            clock = env.current_hour >= 23.75
            ev["end_clock" if clock else "end_satisfaction"] += 1
            out["ends"][0 if clock else 1] += 1
            ev["delayed_on_time"] += sum(f.status == "delayed" and abs(f.actual_time - f.scheduled_time) < 0.25 for f in env.flights)
            obs, _ = env.reset()
            out["resets"].append((t, obs))
    return env, out


def make(name, n_envs, T, seed0, a_seed, policy, autoreset=True):
    ev = dict.fromkeys(EVENTS, 0)
    rows = [run_env(seed0 + i, T, a_seed, i, policy, autoreset, ev) for i in range(n_envs)]
    env = rows[0][0]
    rows = [r[1] for r in rows]
    ridx = [(i, t) for i, r in enumerate(rows) for t, _ in r["resets"]]
    sp = dict(action=dict(kind=type(env.action_space).__name__, n=int(env.action_space.n)),
              observation=dict(kind=type(env.observation_space).__name__, shape=list(env.observation_space.shape), dtype=str(env.observation_space.dtype),
                               low=float(env.observation_space.low.min()), high=float(env.observation_space.high.max())))
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), autoreset=np.int64(autoreset),
                  actions=np.stack([r["A"] for r in rows]), obs0=np.stack([r["obs0"] for r in rows]), obs_xor=xor_time(np.stack([r["O"] for r in rows])),
                  reward=np.stack([r["R"] for r in rows]), terminated=np.stack([r["TM"] for r in rows]), info=np.stack([r["I"] for r in rows]),
                  info_keys=np.array(json.dumps(INFO)), reset_index=np.array(ridx, np.int32).reshape(-1, 2),
                  reset_obs=np.array([ob for r in rows for _, ob in r["resets"]], np.float32).reshape(-1, 160),
                  ends=np.array([r["ends"] for r in rows], np.int32), wraps=np.array([r["wraps"] for r in rows], np.int32),
                  spaces=np.array(json.dumps(sp)), events=np.array(json.dumps(ev)), versions=np.array(json.dumps(common.versions())))
    out = os.path.join(common.GOLDEN, name + ".npz")
    np.savez_compressed(out, **arrays)
    print(name, "ends", len(ridx), "sum reward", arrays["reward"].sum(), "events", ev, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 315465, "larger than the largest restaurant fixture: cut envs"
    return arrays, ev


if __name__ == "__main__":
    h, eh = make("airline_hash", 16, 150, seed0=1500, a_seed=201, policy="hash")
    d, ed = make("airline_dispatch", 16, 150, seed0=1530, a_seed=202, policy="dispatch")
    c, ec = make("airline_cancel", 16, 60, seed0=1560, a_seed=203, policy="cancel")
    o, eo = make("airline_overrun", 8, 420, seed0=1590, a_seed=204, policy="hash", autoreset=False)
    tot = {k: eh[k] + ed[k] + ec[k] for k in EVENTS}
    assert ((h["ends"][:, 0] + d["ends"][:, 0] + c["ends"][:, 0]) >= 2).all(), "fewer than two ends on the clock in some env"
    assert tot["end_satisfaction"] >= 16 and tot["delayed_on_time"] >= 1 and tot["a41_accepted"] >= 1 and tot["a41_refused"] >= 1, tot
    assert c["ends"][:, 0].sum() == 0 and c["ends"][:, 1].sum() == len(c["reset_index"]) >= 16, "a cancel episode ended on the clock"
    assert (o["wraps"] >= 1).all() and eo["maintenance"] >= 100 and eo["fuel_floor"] >= 1, eo
