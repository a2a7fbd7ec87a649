"""Golden vectors for SpaceStationEnv, produced by running the reference's own space_station_env/station_env.py (unmodified, imported
from the reference checkout under the stub gymnasium / pygame).  Run it in a process of its own.

Seeding protocol: the env draws from the process-global NumPy legacy stream only (`np.random.normal / uniform / random / choice`) and
never seeds it (`super().reset(seed=)` seeds the unused np_random), so env i is `np.random.seed(seed0 + i)`, `SpaceStationEnv()` — the
constructor draws nothing — and `env.reset(seed=seed0 + i)`.  On `terminated` the terminal observation is recorded and `env.reset()`
continues the same stream (auto-reset) and keeps what reset() does not touch: `episode_reward`, `last_emergency_time`, every crew
member's `current_module`, `solar_angle`, `radiation_level`, `total_power_consumption`.  `station_overrun` never resets and steps the
reference on past `terminated`.  `station_timeout` sets `env.max_steps = 20` after construction.

The power sum is Python's sum() of floats, which Python 3.12 and later compensate: the fixtures are those of a plain left-to-right
sum, so this script refuses to run there.

Policies: "hash" = the counter hash over 0..39; "keep" = two steps in three a hashed action over 0..11, otherwise action 36 and
12 + a hashed index over 0..11 in turn; "idle" = action 39 only; "evacuate" = action 38 at step 3, otherwise 39.
The event counters are taken by watching the env from outside: its methods are wrapped per instance, its code is not touched.
`obs_xor` is the per-step observation as uint32 bit patterns [env, element, step], each step XORed with the step before it;
space_station_model.fixture_obs() undoes it.  `info` holds the nine info values in the reference's order, `system_failures` as the
length of the list, and as a tenth column the 12-bit mask of the systems named in it.
`station_poked` sets plain state attributes of the env object between steps, where the reference's own arithmetic keeps a state out
of reach of any run a fixture can hold (water and food fall below 20 after some 8,000 steps, the oxygen tanks never rise above their
initial 20, the pressure falls only by a micrometeorite of probability 0.00025 a step, the cascade of failed systems ends an unattended
station long before the air does); the reference's code stays untouched.  Its `pokes` table holds (env, step, index into
`poke_fields`, value): the field, named as csrc/space_station_env.hpp names it, is set to the value before the action of that step.
Outputs: tests/golden/station_hash.npz, station_keep.npz, station_idle.npz, station_evacuate.npz, station_timeout.npz,
station_overrun.npz (RUNS) and station_poked.npz (NEW_RUNS; `python gen_space_station.py --new` writes it alone and leaves the others'
bytes as they are).
"""
import json
import os
import re
import sys

import numpy as np

import common

assert sys.version_info < (3, 12), "Python 3.12+ sums floats with compensation: the power sum would not be the recorded left-to-right sum"

common.use_stubs()
common.add_reference_dir("space_station_env")
from station_env import SpaceStationEnv  # noqa: E402  (reference code)

INFO = ("time_step", "day", "crew_alive", "system_failures", "emergency_count", "mission_success", "episode_reward", "battery_level", "avg_crew_health")
EVENTS = ("crew_dead", "cascade", "uninhabitable", "timeout", "carried_angle", "backup_used", "backup_gone", "no_spares", "thermal_drift",
          "micrometeorite", "system_failure", "medical", "solar_storm", "failure_critical", "failure_noncritical", "choice_rejected",
          "negative_health", "docking_after_reset", "both_flags", "mission_success", "power_failure_steps")
# counted in the runs of NEW_RUNS only (the older files' `events` have the keys above)
NEW_EVENTS = ("water_low", "food_low", "resources_bonus", "module_cold", "module_hot", "fatigued", "suffocated_alive", "air_thin", "air_alert",
              "end_air", "end_pressure", "end_crew", "crew_lost_systems_fine", "oxygen_exactly_19", "water_short", "food_short", "waste_short")
KINDS = ("micrometeorite", "system_failure", "medical", "solar_storm")
OBS = 120


def action(policy, a_seed, i, t):
    if policy == "keep":
        if t % 3 != 2:
            return common.hash_action(a_seed, i, t, 12)
        return 36 if (t // 3) % 2 == 0 else 12 + common.hash_action(a_seed, i, t, 12)
    if policy == "idle":
        return 39
    if policy == "evacuate":
        return 38 if t == 3 else 39
    return common.hash_action(a_seed, i, t, 40)


def set_field(env, name, value):
    """a poke: the header's name of a plain state field -> the reference's attribute"""
    m = re.fullmatch(r"(o2|co2|pres|temp|health|oxy|fatigue|eff)(\d+)", name)
    if m:
        kind, k = m.group(1), int(m.group(2))
        if kind in ("o2", "co2", "pres", "temp"):
            setattr(list(env.modules.values())[k], dict(o2="oxygen_percent", co2="co2_ppm", pres="pressure", temp="temperature")[kind], float(value))
        elif kind == "eff":
            list(env.systems.values())[k].efficiency = float(value)
        else:
            setattr(env.crew[k], dict(health="health", oxy="oxygen_level", fatigue="fatigue")[kind], float(value))
    elif name in ("water", "food", "tanks", "waste"):
        env.resources[dict(water="water", food="food", tanks="oxygen_tanks", waste="waste_capacity")[name]] = float(value)
    else:
        raise KeyError(name)


O2_JUST_ABOVE_19 = 19.0 + 0.01                                            # minus the 0.01 one crew member breathes: 19.0 exactly (asserted)


def plan_poked(i, t):
    """-> the pokes [(field, value)] before step t of env i (every action is 39).  Step 1: the oxygen generator off and module 2 at
    19.01 % oxygen, which one crew member's 0.01 makes 19.0 exactly (neither `< 19` nor `> 19`); env 3 loses crew member 0 there, with
    the systems and the battery fine.  Steps 2 to 5: water at 15, food at 15, the tanks at 25, each alone.  Step 6: module 0 at 12
    degrees, module 1 at 33.  Step 7: a fatigue of 85.  Step 8: crew member 1 at an oxygen level of 1 in a module at 18 %.  Step 9:
    every module at 18.5 % (a mean at or below 19), step 10: at 17 % (the life-support alert).  Step 11: the ends: env 0 every module
    at 14 % oxygen, env 1 every module at 75 kPa, env 2 every crew member at health 0.  Steps 12 to 15 (after the resets of envs 0 to
    2): water at 5, food at 5, the waste capacity at 5, each alone: the terms of the shortage penalty (`< 10`, :702-705) that no
    other run makes true (the tanks and the spare parts fall below 10 in the older files)."""
    all_o2 = lambda v: [(f"o2{m}", v) for m in range(8)]
    if t == 1:
        return [("eff0", 20.0), ("o2" + "2", O2_JUST_ABOVE_19)] + ([("health0", 0.0)] if i == 3 else [])
    if t == 2:
        return [("eff0", 100.0), ("water", 15.0)]
    if t == 3:
        return [("water", 1000.0), ("food", 15.0)]
    if t == 4:
        return [("food", 500.0), ("tanks", 25.0)]
    if t == 5:
        return [("tanks", 20.0)]
    if t == 6:
        return [("temp0", 12.0), ("temp1", 33.0)]
    if t == 7:
        return [("fatigue2", 85.0)]
    if t == 8:
        return [("oxy1", 1.0), ("o2" + "1", 18.0)]
    if t == 9:
        return all_o2(18.5)
    if t == 10:
        return all_o2(17.0)
    if t == 11:
        return [all_o2(14.0), all_o2(21.0) + [(f"pres{m}", 75.0) for m in range(8)], all_o2(21.0) + [(f"health{c}", 0.0) for c in range(6)], all_o2(21.0)][i]
    if t == 12:
        return [("water", 5.0)]
    if t == 13:
        return [("water", 1000.0), ("food", 5.0)]
    if t == 14:
        return [("food", 500.0), ("waste", 5.0)]
    if t == 15:
        return [("waste", 100.0)]
    return []


def xor_time(obs):
    """float32 [n, T, 120] -> uint32 [n, 120, T], every step XORed with its predecessor (np.bitwise_xor.accumulate along the last axis undoes it)"""
    x = np.ascontiguousarray(obs.transpose(0, 2, 1)).view(np.uint32).copy()
    x[:, :, 1:] ^= x[:, :, :-1].copy()
    return x


def watch(env, ev):
    """count what the fixtures are for, from outside the env"""
    check, life, act = env._check_emergencies, env._update_life_support, env._process_action
    names = list(env.systems)

    def _check():
        before, count, failures = np.random.get_state(), env.emergency_count, len(env.system_failures)
        check()
        if env.emergency_count > count:
            rs = np.random.RandomState()
            rs.set_state(before)
            rs.random_sample()
            kind = int(rs.randint(0, 4))                              # what choice() over the four kinds drew
            ev[KINDS[kind]] += 1
            used = (np.random.get_state()[2] - before[2]) % 624
            ev["choice_rejected"] += int(used > (3 if kind == 3 else 4))
            if len(env.system_failures) > failures:
                ev["failure_critical" if env.systems[env.system_failures[-1]].is_critical else "failure_noncritical"] += 1

    def _life():
        ev["thermal_drift"] += int(env.systems["Thermal Control"].efficiency <= 50)
        life()

    def _act(a):
        if a == 37:
            ev["backup_used" if env.backup_power_available else "backup_gone"] += 1
        if 12 <= a < 24:
            ev["no_spares"] += int(not env.resources["spare_parts"] > 0)
        act(a)

    env._check_emergencies, env._update_life_support, env._process_action = _check, _life, _act
    return names


def info_row(env, info, names):
    assert list(info) == list(INFO)
    mask = 0
    for name in info["system_failures"]:
        mask |= 1 << names.index(name)
    row = [float(info[k]) if k != "system_failures" else float(len(info[k])) for k in INFO]
    return row + [float(mask)]


def run_env(seed, T, a_seed, i, policy, autoreset, ev, max_steps=None):
    np.random.seed(seed)
    env = SpaceStationEnv()
    if max_steps is not None:
        env.max_steps = max_steps
    names = watch(env, ev)
    obs, info = env.reset(seed=seed)
    assert obs.shape == (OBS,) and obs.dtype == np.float32
    out = dict(obs0=obs, info0=info_row(env, info, names), A=np.zeros(T, np.int8), R=np.zeros(T, np.float64), TM=np.zeros(T, np.uint8),
               TR=np.zeros(T, np.uint8), I=np.zeros((T, 10), np.float64), O=np.zeros((T, OBS), np.float32), resets=[], pokes=[])
    for t in range(T):
        a = action("idle" if policy == "poked" else policy, a_seed, i, t)
        if policy == "poked":
            for name, value in plan_poked(i, t):
                set_field(env, name, value)
                out["pokes"].append((i, t, name, value))
        obs, rew, term, trunc, info = env.step(a)
        if "water_low" in ev:                                         # what the step saw, read off the state it left
            res, mods, alive = env.resources, list(env.modules.values()), sum(1 for c in env.crew if c.health > 0)
            avg_o2 = np.mean([m.oxygen_percent for m in mods])
            avg_eff = np.mean([s.efficiency for s in env.systems.values()])
            ev["water_low"] += int(not res["water"] > 20)
            ev["food_low"] += int(res["water"] > 20 and not res["food"] > 20)
            ev["water_short"] += int(res["water"] < 10)
            ev["food_short"] += int(res["food"] < 10)
            ev["waste_short"] += int(res["waste_capacity"] < 10)
            ev["resources_bonus"] += int(res["water"] > 20 and res["food"] > 20 and res["oxygen_tanks"] > 20)
            ev["module_cold"] += sum(1 for k in range(6) if mods[k].temperature < 15)
            ev["module_hot"] += sum(1 for k in range(6) if mods[k].temperature > 30)
            ev["fatigued"] += sum(1 for c in env.crew if c.fatigue > 80)
            ev["suffocated_alive"] += sum(1 for c in env.crew if c.health > 0 and c.oxygen_level <= 0)
            ev["air_thin"] += int(not 19 < avg_o2)
            ev["air_alert"] += int(avg_o2 < 18)
            ev["crew_lost_systems_fine"] += int(env.battery_level > 50 and avg_eff > 80 and alive < 6)
            ev["oxygen_exactly_19"] += sum(1 for k in range(6) if mods[k].oxygen_percent == 19.0)
            if term:
                crit = sum(1 for s in env.systems.values() if s.is_critical and s.efficiency < 10)
                dead = all(c.health <= 0 for c in env.crew)
                ev["end_crew"] += int(dead)
                ev["end_air"] += int(not dead and crit < 3 and avg_o2 < 15)
                ev["end_pressure"] += int(not dead and crit < 3 and not avg_o2 < 15 and np.mean([m.pressure for m in mods]) < 80)
        assert obs.dtype == np.float32 and rew == int(rew) and (not trunc or term)
        ev["negative_health"] += int((obs[2:24:4] < 0).any())
        ev["power_failure_steps"] += int(env.emergency_alerts["power_failure"])
        out["A"][t] = a; out["R"][t] = rew; out["TM"][t] = term; out["TR"][t] = trunc; out["O"][t] = obs
        out["I"][t] = info_row(env, info, names)
        if term and autoreset:
            crit = sum(1 for s in env.systems.values() if s.is_critical and s.efficiency < 10)
            kind = ("timeout" if env.time_step >= env.max_steps else "crew_dead" if all(c.health <= 0 for c in env.crew)
                    else "cascade" if crit >= 3 else "uninhabitable")
            ev[kind] += 1
            ev["both_flags"] += int(bool(term and trunc))
            ev["mission_success"] += int(bool(info["mission_success"]))
            obs, _ = env.reset()
            ev["carried_angle"] += int(obs[111] != 1.0)
            ev["docking_after_reset"] += int(all(c.current_module == "Docking" for c in env.crew))
            out["resets"].append((t, obs))
    return env, out


def make(name, n_envs, T, seed0, a_seed, policy, autoreset=True, max_steps=None):
    ev = dict.fromkeys(EVENTS + (NEW_EVENTS if name in NEW_RUNS else ()), 0)
    rows = [run_env(seed0 + i, T, a_seed, i, policy, autoreset, ev, max_steps) for i in range(n_envs)]
    env = rows[0][0]
    rows = [r[1] for r in rows]
    ridx = [(i, t) for i, r in enumerate(rows) for t, _ in r["resets"]]
    sp = dict(action=dict(kind=type(env.action_space).__name__, n=int(env.action_space.n)),
              observation=dict(kind=type(env.observation_space).__name__, shape=list(env.observation_space.shape), dtype=str(env.observation_space.dtype),
                               low=float(env.observation_space.low.min()), high=float(env.observation_space.high.max()), returned=OBS))
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), autoreset=np.int64(autoreset),
                  max_steps=np.int64(env.max_steps),
                  actions=np.stack([r["A"] for r in rows]), obs0=np.stack([r["obs0"] for r in rows]), info0=np.array([r["info0"] for r in rows], np.float64),
                  obs_xor=xor_time(np.stack([r["O"] for r in rows])),
                  reward=np.stack([r["R"] for r in rows]), terminated=np.stack([r["TM"] for r in rows]), truncated=np.stack([r["TR"] for r in rows]),
                  info=np.stack([r["I"] for r in rows]),
                  info_keys=np.array(json.dumps(INFO + ("system_failure_mask",))), reset_index=np.array(ridx, np.int32).reshape(-1, 2),
                  reset_obs=np.array([ob for r in rows for _, ob in r["resets"]], np.float32).reshape(-1, OBS),
                  spaces=np.array(json.dumps(sp)), events=np.array(json.dumps(ev)), versions=np.array(json.dumps(common.versions())))
    if policy == "poked":
        pokes = [p for r in rows for p in r["pokes"]]
        names = sorted({p[2] for p in pokes})
        arrays["poke_fields"] = np.array(json.dumps(names))
        arrays["pokes"] = np.array([(i, t, names.index(name), value) for i, t, name, value in pokes], np.float64).reshape(-1, 4)
    return arrays, ev


def save(name, arrays):
    out = os.path.join(common.GOLDEN, name + ".npz")
    np.savez_compressed(out, **arrays)
    print(name, "ends", len(arrays["reset_index"]), "sum reward", arrays["reward"].sum(), "events", str(arrays["events"]), os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1 << 20, "a committed file stays under 1 MiB"


# seed0: found by a search on the CPU (`--search NAME`) for runs that hold what check() asks of them
RUNS = dict(station_hash=dict(n_envs=8, T=400, seed0=0, a_seed=401, policy="hash"),
            station_keep=dict(n_envs=8, T=600, seed0=264, a_seed=402, policy="keep"),
            station_idle=dict(n_envs=16, T=100, seed0=300, a_seed=403, policy="idle"),
            station_evacuate=dict(n_envs=8, T=80, seed0=400, a_seed=404, policy="evacuate"),
            station_timeout=dict(n_envs=8, T=70, seed0=500, a_seed=405, policy="keep", max_steps=20),
            station_overrun=dict(n_envs=8, T=400, seed0=600, a_seed=406, policy="hash", autoreset=False))
# recorded later than RUNS, for the branches of csrc/space_station_env.hpp that those leave unentered (tests/test_lane_env_branch_coverage.py)
NEW_RUNS = dict(station_poked=dict(n_envs=4, T=18, seed0=700, a_seed=407, policy="poked"))


def check_one(name, ev):
    """the conditions a fixture is recorded for (tests/test_space_station_cpu.py asserts them again)"""
    if name == "station_hash":
        return ev["crew_dead"] >= 1 and ev["cascade"] >= 1 and ev["carried_angle"] >= 1 and ev["backup_used"] >= 1 and ev["backup_gone"] >= 1
    if name == "station_keep":
        return (min(ev[k] for k in KINDS) >= 1 and ev["failure_critical"] >= 1 and ev["failure_noncritical"] >= 1 and ev["choice_rejected"] >= 1)
    if name == "station_idle":
        return ev["cascade"] >= 16 and ev["thermal_drift"] >= 16
    if name == "station_evacuate":
        return ev["docking_after_reset"] >= 8
    if name == "station_poked":
        return (min(ev[k] for k in NEW_EVENTS) >= 1 and ev["end_air"] == ev["end_pressure"] == ev["end_crew"] == 1 and ev["oxygen_exactly_19"] == 4
                and ev["uninhabitable"] == 2 and ev["crew_dead"] == 1 and ev["cascade"] == 0 and ev["water_short"] == ev["food_short"] == ev["waste_short"] == 4)
    if name == "station_timeout":
        return ev["timeout"] >= 8 and ev["both_flags"] == ev["timeout"] == ev["mission_success"]
    return True


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--search":
        name = sys.argv[2]
        for seed0 in range(int(sys.argv[3]) if len(sys.argv) > 3 else 0, 100000, RUNS[name]["n_envs"]):
            _, ev = make(name, **dict(RUNS[name], seed0=seed0))
            print(seed0, {k: v for k, v in ev.items() if v})
            if check_one(name, ev):
                print("found", name, seed0)
                break
        sys.exit(0)
    assert O2_JUST_ABOVE_19 - 1 * 0.01 == 19.0
    made = {name: make(name, **kw) for name, kw in (NEW_RUNS if "--new" in sys.argv[1:] else RUNS).items()}
    for name, (_, ev) in made.items():                                    # nothing is written unless the runs hold what they are for
        assert check_one(name, ev), (name, ev)
    for name, (arrays, _) in made.items():
        save(name, arrays)
