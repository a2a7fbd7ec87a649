"""Golden vectors for AgriculturalFarmEnv, produced by running the reference's own agricultural_farm_env/farm_env.py (unmodified,
imported from the reference checkout under the stub gymnasium / pygame).  Run it in a process of its own.

Seeding protocol: the env draws from the process-global NumPy legacy stream (`np.random.uniform / random / randint / normal`) and, for
the crop it plants, from CPython's global `random` (`random.choice`); it seeds neither (`super().reset(seed=)` seeds the unused
np_random).  So env i is `random.seed(s); np.random.seed(s); AgriculturalFarmEnv()` — the constructor draws the fields, the equipment
and the market — and `env.reset(seed=s)`, which draws them again, with s = seed0 + i.  The envs of a fixture run one after the other, so
each has both global streams to itself.  On `terminated` the terminal observation is recorded and `env.reset()` continues both streams
(auto-reset), the legacy Gaussian's cached second value included, and keeps what reset() does not touch: `water_quality`.
`farm_overrun` never resets and steps the reference on past `terminated`.  `farm_two_years` sets `env.max_years = 2` after construction.
`farm_poked` sets plain state attributes of the env object between steps, where the reference's own arithmetic keeps a state out of
reach from reset() (a machine's maintenance_needed above 0.5, six days of excessive rain, a pest level above 1, a yield potential above
1 at a harvest by hand); the reference's code stays untouched.  Its `pokes` table holds (env, step, index into `poke_fields`, value):
the field, named as csrc/farm_env.hpp names it, is set to the value before the action of that step.

Policies: "hash" = the counter hash over 0..44; "bankrupt" = action 40 only; "orchard" = action 3 and action 8 in turn, and action 3 alone in
every second hundred of steps, where a ripe crop is left to the automatic harvest; "chores" = on
even steps the cycle over CHORES in order, on odd steps a hashed pick from CHORES (a field is then fertilised or sprayed twice inside
the waiting time), with action 3 at steps 31 and 211 so that action 43 sees a third crop type; "soil" = action 3 once, forty times action 42 (organic
matter down to its floor in every field that holds a truthy crop), then action 41 (biodiversity above 0.7); "poked" = plan_poked().
The event counters are taken by watching the env from outside: its methods are wrapped per instance, its code is not touched.
`obs_xor` is the per-step observation's 134 live columns as uint32 bit patterns [env, element, step], each step XORed with the step
before it; farm_model.fixture_obs() undoes it.  Columns 134..619 are asserted to be zero in every recorded row.  `info` holds the eleven
scalar info values in the reference's order (`season` as 0..3), then `field_status` as crop (-1 for "None"), stage, health and
yield_potential of the four fields.
Outputs: tests/golden/farm_hash.npz, farm_bankrupt.npz, farm_orchard.npz, farm_chores.npz, farm_overrun.npz, farm_two_years.npz (RUNS) and
farm_soil.npz, farm_poked.npz (NEW_RUNS; `python gen_farm.py --new` writes these alone and leaves the others' bytes as they are).
"""
import json
import os
import random
import re
import sys

import numpy as np

import common

common.use_stubs()
common.add_reference_dir("agricultural_farm_env")
import farm_env as reference  # noqa: E402  (reference code)
from farm_env import AgriculturalFarmEnv  # noqa: E402

INFO = ("day", "season", "year", "cash_flow", "total_revenue", "total_expenses", "profit_margin", "carbon_sequestered",
        "water_conservation_score", "biodiversity_index", "soil_health_trend")
FIELD_INFO = ("field_crop", "field_stage", "field_health", "field_yield_potential")
SEASONS = ("spring", "summer", "fall", "winter")
CROPS = ("Wheat", "Corn", "Tomatoes", "Apples", "Soybeans")
EVENTS = ("year_end", "bankrupt", "soil_end", "choice_spring", "choice_summer", "choice_fall", "plant_winter", "frost_high", "drought_long",
          "excessive_rain", "negative_health", "carried_water_quality", "harvest_action", "harvest_auto", "replant_bonus", "replant_no_bonus",
          "replant_after_wheat", "fert_refused", "over_fertilised", "pest_refused", "equipment_refused", "maintenance_repair", "sale_taken",
          "sale_refused", "rotation_three", "rotation_fewer", "climate_temperature", "invalid_fifth_field")
# counted in the runs of NEW_RUNS only (the older files' `events` have the keys above)
NEW_EVENTS = ("soil_low", "biodiversity_high", "maintenance_refused", "maintenance_cost", "rain_protection", "excessive_rain_penalty", "severe_pest",
              "harvest_5000", "harvest_2000", "harvest_1000", "harvest_poor", "harvest_field_3", "harvest_other_field")
OBS, LIVE = 620, 134
CHORES = tuple(list(range(10, 14)) + list(range(15, 19)) + list(range(20, 24)) + list(range(25, 30)) + list(range(30, 34)) + list(range(35, 40))
               + list(range(41, 45)))


def action(policy, a_seed, i, t):
    if policy == "bankrupt":
        return 40
    if policy == "orchard":
        return 3 if t % 2 == 0 or (t // 100) % 2 == 1 else 8
    if policy == "chores":
        if t in (31, 211):
            return 3
        return CHORES[(t // 2) % len(CHORES)] if t % 2 == 0 else CHORES[common.hash_action(a_seed, i, t, len(CHORES))]
    if policy == "soil":
        return 3 if t == 0 else 42 if t <= 40 else 41
    return common.hash_action(a_seed, i, t, 45)


def set_field(env, name, value):
    """a poke: the header's name of a plain state field -> the reference's attribute"""
    m = re.fullmatch(r"f(\d)\.(yp|health|pest)", name)
    if m:
        setattr(env.field_sections[int(m.group(1))], dict(yp="yield_potential", health="health", pest="pest_level")[m.group(2)], float(value))
    elif re.fullmatch(r"maint\d", name):
        env.equipment[int(name[5:])].maintenance_needed = float(value)
    elif name == "rain_days":
        env.weather.excessive_rain_days = int(value)
    else:
        raise KeyError(name)


def plan_poked(env, i, t, state):
    """-> (action, [(field, value)]) of step t of env i: field 3 is planted at step 0 and harvested by hand as soon as it is ripe, with
    the yield potential poked to 1.4, 1.0 or 0.8 by env (env 3: as it is), so that every arm of the harvest reward is taken; steps 10 to
    12 poke two machines' maintenance_needed, operate the worse one (refused), pay for both and repair both; step 14 sprays field 1
    at a pest level of 1.5; steps 16 to 27 hold excessive_rain_days at 7 under action 40."""
    f3 = env.field_sections[3]
    if f3.growth_stage == reference.CropStage.HARVEST_READY and not state.get("harvested"):
        state["harvested"] = True
        return 8, ([("f3.yp", (1.4, 1.0, 0.8)[i]), ("f3.health", 1.0)] if i < 3 else [])
    if t == 0:
        return 3, []
    if t == 10:
        return 26, [("maint0", 0.6), ("maint1", 0.9)]
    if t == 11:
        return 43, []
    if t == 12:
        return 44, []
    if t == 14:
        return 21, [("f1.pest", 1.5)]
    if 16 <= t <= 27:
        return 40, [("rain_days", 7.0)]
    return 43, []


def xor_time(obs):
    """float32 [n, T, 134] -> uint32 [n, 134, T], every step XORed with its predecessor (np.bitwise_xor.accumulate along the last axis undoes it)"""
    x = np.ascontiguousarray(obs.transpose(0, 2, 1)).view(np.uint32).copy()
    x[:, :, 1:] ^= x[:, :, :-1].copy()
    return x


def watch(env, ev):
    """count what the fixtures are for, from outside the env"""
    act, harvest = env._process_action, env._harvest_crop
    inside = [False]

    def _harvest(field):
        if field.crop_type is not None:
            ev["harvest_action" if inside[0] else "harvest_auto"] += 1
            if "harvest_5000" in ev:                                  # the arm of :821-828, in the reference's own arithmetic
                base = reference.CROP_DATA[field.crop_type].yield_per_hectare * (field.size / 625.0)
                ratio = base * field.yield_potential * field.health / base
                ev["harvest_5000" if ratio > 1.2 else "harvest_2000" if ratio > 0.9 else "harvest_1000" if ratio > 0.7 else "harvest_poor"] += 1
                ev["harvest_field_3" if field is env.field_sections[3] else "harvest_other_field"] += 1
        return harvest(field)

    def _act(a):
        season = int(env.current_season)
        if 0 <= a <= 3:
            f = env.field_sections[a]
            if f.crop_type is None:
                ev[("choice_spring", "choice_summer", "choice_fall", "plant_winter")[season]] += 1
        if a in (4, 9, 14, 19, 24, 34):
            ev["invalid_fifth_field"] += 1
        if 10 <= a <= 13:
            f = env.field_sections[a - 10]
            ev["fert_refused"] += int(not env.current_day - f.last_fertilized_day > 14)
        if 20 <= a <= 23:
            f = env.field_sections[a - 20]
            ev["pest_refused"] += int(not env.current_day - f.last_pesticide_day > 21)
        if 25 <= a <= 29:
            q = env.equipment[a - 25]
            ev["equipment_refused"] += int(not (q.fuel_level > 0.1 and q.maintenance_needed < 0.8))
            if "maintenance_refused" in ev:
                ev["maintenance_refused"] += int(q.fuel_level > 0.1 and not q.maintenance_needed < 0.8)
        if a == 40 and "rain_protection" in ev:
            ev["rain_protection"] += int(not env.weather.frost_risk > 0.5 and env.weather.excessive_rain_days > 3)
        if 35 <= a <= 39:
            ev["sale_taken" if env.cash_flow < 10000 else "sale_refused"] += 1
        if a == 43:
            kinds = {f.crop_type for f in env.field_sections if f.crop_type}
            ev["rotation_three" if len(kinds) >= 3 else "rotation_fewer"] += 1
        if a == 44:
            ev["maintenance_repair"] += sum(1 for q in env.equipment if q.maintenance_needed > 0.5)
        last = [f.last_crop for f in env.field_sections]
        inside[0] = True
        reward = act(a)
        inside[0] = False
        if 0 <= a <= 3 and reward >= 50 and last[a] is not None:
            ev["replant_bonus" if reward == 150 else "replant_no_bonus"] += 1
            ev["replant_after_wheat"] += int(last[a] == 0 and reward == 50 and env.field_sections[a].crop_type != 0)
        if 10 <= a <= 13:
            ev["over_fertilised"] += int(reward == -80)
        if 20 <= a <= 23 and "severe_pest" in ev:
            ev["severe_pest"] += int(reward == 150)
        return reward

    env._process_action, env._harvest_crop = _act, _harvest


def info_row(info):
    assert list(info) == list(INFO) + ["field_status"] and len(info["field_status"]) == 4
    row = [float(SEASONS.index(info[k])) if k == "season" else float(info[k]) for k in INFO]
    fs = info["field_status"]
    row += [float(CROPS.index(f["crop"])) if f["crop"] != "None" else -1.0 for f in fs]
    row += [float(reference.CropStage[f["stage"]].value) for f in fs]
    row += [float(f["health"]) for f in fs] + [float(f["yield_potential"]) for f in fs]
    return row


def run_env(seed, T, a_seed, i, policy, autoreset, ev, max_years=None):
    random.seed(seed)
    np.random.seed(seed)
    env = AgriculturalFarmEnv()
    if max_years is not None:
        env.max_years = max_years
    watch(env, ev)
    obs, info = env.reset(seed=seed)
    assert obs.shape == (OBS,) and obs.dtype == np.float32 and not obs[LIVE:].any()
    out = dict(obs0=obs[:LIVE], info0=info_row(info), A=np.zeros(T, np.int8), R=np.zeros(T, np.float64), TM=np.zeros(T, np.uint8),
               I=np.zeros((T, len(INFO) + 16), np.float64), O=np.zeros((T, LIVE), np.float32), resets=[], pokes=[])
    state = {}
    for t in range(T):
        if policy == "poked":
            a, pokes = plan_poked(env, i, t, state)
            for name, value in pokes:
                set_field(env, name, value)
                out["pokes"].append((i, t, name, value))
        else:
            a = action(policy, a_seed, i, t)
        year = env.year
        obs, rew, term, trunc, info = env.step(a)
        assert obs.dtype == np.float32 and rew == int(rew) and not trunc and not obs[LIVE:].any()
        ev["negative_health"] += int((obs[2:60:15] < 0).any())
        ev["frost_high"] += int(env.weather.frost_risk > 0.5)
        ev["drought_long"] += int(env.weather.drought_days > 20)
        ev["excessive_rain"] += int(env.weather.excessive_rain_days > 5)
        ev["climate_temperature"] += int(year >= 2 and env.climate_change_factor == 0.05)
        if "soil_low" in ev:
            ev["soil_low"] += int(np.mean([f.soil_organic_matter for f in env.field_sections]) < 0.02)
            ev["biodiversity_high"] += int(env.biodiversity_index > 0.7)
            ev["maintenance_cost"] += sum(1 for q in env.equipment if q.maintenance_needed > 0.5)
            ev["excessive_rain_penalty"] += sum(1 for f in env.field_sections if f.crop_type and env.weather.excessive_rain_days > 5)
        out["A"][t] = a; out["R"][t] = rew; out["TM"][t] = term; out["O"][t] = obs[:LIVE]
        out["I"][t] = info_row(info)
        if term and autoreset:
            kind = "year_end" if env.year > env.max_years else "bankrupt" if env.cash_flow < -50000 else "soil_end"
            ev[kind] += 1
            quality = env.water_quality
            obs, _ = env.reset()
            assert not obs[LIVE:].any() and obs[122] == np.float32(quality)
            ev["carried_water_quality"] += int(obs[122] != np.float32(0.9))
            out["resets"].append((t, obs[:LIVE]))
    return env, out


def make(name, n_envs, T, seed0, a_seed, policy, autoreset=True, max_years=None):
    ev = dict.fromkeys(EVENTS + (NEW_EVENTS if name in NEW_RUNS else ()), 0)
    rows = [run_env(seed0 + i, T, a_seed, i, policy, autoreset, ev, max_years) for i in range(n_envs)]
    env = rows[0][0]
    rows = [r[1] for r in rows]
    ridx = [(i, t) for i, r in enumerate(rows) for t, _ in r["resets"]]
    sp = dict(action=dict(kind=type(env.action_space).__name__, n=int(env.action_space.n)),
              observation=dict(kind=type(env.observation_space).__name__, shape=list(env.observation_space.shape), dtype=str(env.observation_space.dtype),
                               low=float(env.observation_space.low.min()), high=float(env.observation_space.high.max()), live=LIVE))
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), autoreset=np.int64(autoreset),
                  max_years=np.int64(env.max_years),
                  actions=np.stack([r["A"] for r in rows]), obs0=np.stack([r["obs0"] for r in rows]), info0=np.array([r["info0"] for r in rows], np.float64),
                  obs_xor=xor_time(np.stack([r["O"] for r in rows])),
                  reward=np.stack([r["R"] for r in rows]), terminated=np.stack([r["TM"] for r in rows]),
                  info=np.stack([r["I"] for r in rows]),
                  info_keys=np.array(json.dumps(INFO + tuple(f"{k}_{f}" for k in FIELD_INFO for f in range(4)))),
                  reset_index=np.array(ridx, np.int32).reshape(-1, 2),
                  reset_obs=np.array([ob for r in rows for _, ob in r["resets"]], np.float32).reshape(-1, LIVE),
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


# seed0: found by a search on the CPU (`--search NAME`) for runs that hold what check_one() asks of them
RUNS = dict(farm_hash=dict(n_envs=8, T=400, seed0=0, a_seed=501, policy="hash"),
            farm_bankrupt=dict(n_envs=8, T=100, seed0=100, a_seed=502, policy="bankrupt"),
            farm_orchard=dict(n_envs=4, T=400, seed0=200, a_seed=503, policy="orchard"),
            farm_chores=dict(n_envs=4, T=400, seed0=300, a_seed=504, policy="chores"),
            farm_overrun=dict(n_envs=4, T=400, seed0=400, a_seed=505, policy="hash", autoreset=False),
            farm_two_years=dict(n_envs=4, T=730, seed0=500, a_seed=506, policy="hash", max_years=2))
# recorded later than RUNS, for the branches of csrc/farm_env.hpp that those leave unentered (tests/test_lane_env_branch_coverage.py)
NEW_RUNS = dict(farm_soil=dict(n_envs=4, T=64, seed0=600, a_seed=507, policy="soil"),
                farm_poked=dict(n_envs=4, T=80, seed0=700, a_seed=508, policy="poked"))


def check_one(name, ev):
    """the conditions a fixture is recorded for (tests/test_farm_cpu.py asserts them again).  `maintenance_repair` is asked of
    farm_poked alone: a machine's maintenance_needed starts below 0.2 and grows by 0.02 per operation, each of which takes 0.1 of at
    most 1.0 fuel, so it stays below 0.5 and action 44 repairs nothing unless the attribute is set from outside."""
    if name == "farm_hash":
        return (ev["year_end"] >= 1 and min(ev["choice_spring"], ev["choice_summer"], ev["choice_fall"]) >= 1 and ev["frost_high"] >= 1
                and ev["drought_long"] >= 1 and ev["negative_health"] >= 1 and ev["carried_water_quality"] >= 1)
    if name == "farm_bankrupt":
        return ev["bankrupt"] == 8
    if name == "farm_orchard":
        return min(ev["harvest_action"], ev["harvest_auto"], ev["replant_bonus"], ev["replant_no_bonus"], ev["replant_after_wheat"]) >= 1
    if name == "farm_chores":
        return (min(ev["fert_refused"], ev["over_fertilised"], ev["pest_refused"], ev["equipment_refused"], ev["sale_taken"], ev["sale_refused"],
                    ev["rotation_three"], ev["rotation_fewer"]) >= 1 and ev["year_end"] >= 1 and ev["carried_water_quality"] >= 1)
    if name == "farm_two_years":
        return ev["climate_temperature"] >= 1 and ev["year_end"] >= 1
    if name == "farm_soil":
        return ev["soil_low"] >= 1 and ev["biodiversity_high"] >= 1
    if name == "farm_poked":
        return (min(ev["maintenance_repair"], ev["maintenance_refused"], ev["maintenance_cost"], ev["rain_protection"], ev["excessive_rain_penalty"],
                    ev["severe_pest"], ev["harvest_5000"], ev["harvest_2000"], ev["harvest_1000"], ev["harvest_poor"]) >= 1
                and ev["harvest_action"] == 4 and ev["harvest_field_3"] == 4)
    return True


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--search":
        name = sys.argv[2]
        RUNS.update(NEW_RUNS)
        for seed0 in range(int(sys.argv[3]) if len(sys.argv) > 3 else 0, 100000, RUNS[name]["n_envs"]):
            _, ev = make(name, **dict(RUNS[name], seed0=seed0))
            print(seed0, {k: v for k, v in ev.items() if v})
            if check_one(name, ev):
                print("found", name, seed0)
                break
        sys.exit(0)
    made = {name: make(name, **kw) for name, kw in (NEW_RUNS if "--new" in sys.argv[1:] else RUNS).items()}
    for name, (_, ev) in made.items():                                    # nothing is written unless the runs hold what they are for
        assert check_one(name, ev), (name, ev)
    for name, (arrays, _) in made.items():
        save(name, arrays)
