"""The action streams of the oracle-lockstep GPU tests, in one place.

Every stream is a named, seeded generator: `STREAMS[name](env type, ctor kwargs, n, T)` yields the actions of step 0 .. T - 1 in the
form the oracle's `step()` takes (climate: a tuple `(ac_temp, lights)`).  The GPU tests iterate these; the CPU coverage test
(test_oracle_branch_coverage.py) replays the same streams on the oracles alone, through `REPLAYS`, to find the dynamics branches
they never reach.  A stream draws from its own `np.random.default_rng(seed)` in a fixed call order: changing a stream changes what
every test that uses it covers, so `stream_sha256()` lets a change be seen.

`HASH_ROLLOUTS` lists the `(a_seed, t0, env0, k)` tuples of the tests' hash-action rollouts (the actions themselves are the counter
hash of tests/_hash_actions.py), and `FIXTURES` the `tests/golden/*.npz` action fixtures the GPU tests replay.
"""
import hashlib

import numpy as np

# env type -> (oracle class, VectorEnv class)
ENV_TYPES = {"snake": ("SnakeOracle", "SnakeVectorEnv"), "crypto": ("CryptoOracle", "CryptoVectorEnv"),
             "traffic": ("TrafficOracle", "TrafficVectorEnv"), "parking": ("ParkingOracle", "ParkingVectorEnv"),
             "climate": ("ClimateOracle", "ClimateVectorEnv"), "fleet": ("FleetOracle", "FleetVectorEnv"),
             "manufacturing": ("ManufacturingOracle", "ManufacturingVectorEnv"), "hospital": ("HospitalOracle", "HospitalVectorEnv")}
NACT = {"snake": 4, "crypto": 5, "traffic": 3, "parking": 8, "fleet": 8, "manufacturing": 25, "hospital": 35}


def traffic_ni(ctor):
    """num_intersections = min(num_intersections, rows * cols) (environment.py:79)"""
    rows, cols = ctor.get("grid_size", (5, 5))
    return min(ctor.get("num_intersections", 9), rows * cols)


# ------------------------------------------------------------------------------------------ test_<env>_gpu.py: step() in lockstep
def hospital_biased(env, ctor, n, T, seed=3):
    """test_hospital_gpu.py::test_step_matches_oracle_all_modes"""
    rng = np.random.default_rng(seed)
    bias = rng.integers(0, 3, n)                                   # a third each: uniform / mass-casualty heavy / staffing heavy
    for t in range(T):
        a = rng.integers(0, 35, n).astype(np.int32)
        r = rng.random(n)
        a = np.where((bias == 1) & (r < 0.5), 33, a)
        a = np.where((bias == 2) & (r < 0.5), rng.integers(0, 12, n), a).astype(np.int32)
        if t % 13 == 0:
            a[rng.random(n) < 0.02] = 40                            # out of range: no-op
        yield a


def manufacturing_biased(env, ctor, n, T, seed=3):
    """test_manufacturing_gpu.py::test_step_matches_oracle_all_modes"""
    rng = np.random.default_rng(seed)
    bias = rng.integers(0, 4, n)                                   # a quarter of the envs each: uniform / type A heavy / start heavy / quality mode
    for t in range(T):
        a = rng.integers(0, 25, n).astype(np.int32)
        r = rng.random(n)
        a = np.where((bias == 1) & (r < 0.7), 0, a)
        a = np.where((bias == 2) & (r < 0.6), rng.integers(0, 6, n), a)
        a = np.where((bias == 3) & (r < 0.3), 23, a).astype(np.int32)
        if t % 13 == 0:
            a[rng.random(n) < 0.02] = 31                            # out of range: no branch taken
        yield a


def fleet_uniform(env, ctor, n, T, seed=3):
    """test_fleet_gpu.py::test_step_matches_oracle_all_modes"""
    rng = np.random.default_rng(seed)
    for t in range(T):
        a = rng.integers(0, 8, (n, 3)).astype(np.int32)
        if t % 11 == 0:
            a[rng.random((n, 3)) < 0.02] = 9                      # invalid action: -10
        yield a


def parking_assign_biased(env, ctor, n, T, seed=6):
    """test_parking_gpu.py::test_step_matches_oracle_all_modes"""
    rng = np.random.default_rng(seed)
    for t in range(T):
        a = rng.integers(0, 8, n).astype(np.int32)
        a[rng.random(n) < 0.5] = rng.integers(1, 4)            # bias toward assignments so the lot fills up
        yield a


def snake_uniform(env, ctor, n, T, seed=1):
    """test_snake_gpu.py::test_step_matches_oracle_all_modes"""
    rng = np.random.default_rng(seed)
    for t in range(T):
        yield rng.integers(0, 4, n).astype(np.int32)


def crypto_uniform(env, ctor, n, T, seed=2):
    """test_crypto_gpu.py::test_step_matches_oracle (seed 2) and ::test_config_knobs_step_and_rollout_match_oracle (seed 5)"""
    rng = np.random.default_rng(seed)
    kind = ctor.get("action_type", "discrete")
    for t in range(T):
        yield (rng.uniform(-1, 1, (n, 2)).astype(np.float32) if kind == "continuous" else rng.integers(0, 5, n).astype(np.int32))


def traffic_sparse(env, ctor, n, T, seed=4):
    """test_traffic_gpu.py::test_step_matches_oracle_all_modes (seed 4) and ::test_layouts_and_knobs_match_oracle (seed 8)"""
    rng = np.random.default_rng(seed)
    ni = traffic_ni(ctor)
    for t in range(T):
        a = rng.integers(0, 3, (n, ni)).astype(np.int32)
        if t % 3:
            a[rng.random((n, ni)) < 0.8] = 0            # long stretches on the lights' own random timers
        yield a


def climate_uniform(env, ctor, n, T, seed=8):
    """test_climate_gpu.py::test_step_matches_oracle_all_modes (seed 8) and ::test_constructor_knobs_match_oracle (seed 3)"""
    rng = np.random.default_rng(seed)
    for t in range(T):
        ac = rng.uniform(10, 38, (n, 1)).astype(np.float32)
        li = rng.integers(0, 2, (n, 4)).astype(np.int8)
        yield ac, li


# ------------------------------------------------------------------------------------------ test_edges_gpu.py
def edge_actions(name, rng, lead, nact, ashape):
    """One block of uniform actions with leading shape `lead` (test_edges_gpu.py, test_facade_contract_gpu.py); name is the
    capitalised env type."""
    if name == "Climate":
        return rng.uniform(10, 38, lead + (1,)).astype(np.float32), rng.integers(0, 2, lead + (4,)).astype(np.int8)
    return rng.integers(0, nact, lead + ashape).astype(np.int32)


# env type -> (n_actions, action shape) as test_edges_gpu.SHORT gives them
EDGE_SHAPES = {"snake": (4, ()), "crypto": (5, ()), "traffic": (3, (9,)), "parking": (8, ()), "climate": (None, None), "fleet": (8, (3,)),
               "manufacturing": (25, ()), "hospital": (35, ())}


def edges_trajectory_block(name, K, n, nact, ashape):
    """test_edges_gpu.py::test_rollout_trajectory_equals_stepping_the_oracle: all K steps drawn as one block"""
    return edge_actions(name, np.random.default_rng(7), (K, n), nact, ashape)


def edges_short_limit(name, limit, n, T, nact, ashape):
    """test_edges_gpu.py::test_short_time_limit_step_api_all_modes: one draw per step, seeded by the time limit"""
    rng = np.random.default_rng(limit)
    for t in range(T):
        yield edge_actions(name, rng, (n,), nact, ashape)


def _at(a, t):
    return tuple(x[t] for x in a) if isinstance(a, tuple) else a[t]


def edges_block(env, ctor, n, T):
    acts = edges_trajectory_block(env.capitalize(), T, n, *EDGE_SHAPES[env])
    for t in range(T):
        yield _at(acts, t)


def edges_steps(env, ctor, n, T, limit=None):
    yield from edges_short_limit(env.capitalize(), limit, n, T, *EDGE_SHAPES[env])


# ------------------------------------------------------------------------------------------ test_final_obs_oracle_gpu.py
def final_obs_actions(name, hkw, k, n, rng):
    """test_final_obs_oracle_gpu.py::_random_actions: all k steps drawn as one block"""
    if name == "climate":
        return rng.uniform(10, 38, (k, n)).astype(np.float32), rng.integers(0, 2, (k, n, 4)).astype(np.int8)
    if name == "crypto" and hkw.get("continuous"):
        return rng.uniform(-1, 1, (k, n, 2)).astype(np.float32)
    shape = {"traffic": (hkw.get("ni", 9),), "fleet": (3,)}.get(name, ())
    return rng.integers(0, NACT[name], (k, n) + shape).astype(np.int32)


def final_obs_block(env, ctor, n, T, seed=None):
    """the explicit-action runs of test_final_obs_oracle_gpu.py: seeded by k (the matrix) or by the grid (snake's episode ends)"""
    hkw = dict(continuous=ctor.get("action_type") == "continuous", ni=traffic_ni(ctor))
    acts = final_obs_actions(env, hkw, T, n, np.random.default_rng(T if seed is None else seed))
    for t in range(T):
        yield _at(acts, t)


STREAMS = {f.__name__: f for f in (hospital_biased, manufacturing_biased, fleet_uniform, parking_assign_biased, snake_uniform, crypto_uniform,
                                   traffic_sparse, climate_uniform, edges_block, edges_steps, final_obs_block)}

# ------------------------------------------------------------------------------------------ the hash-action rollouts
# test -> (a_seed, t0, env0, k) of its oracle-checked hash rollouts; k is a dict by env type where the types differ
HASH_ROLLOUTS = {
    "config5": dict(a_seed=123, t0=0, k={"hospital": 200, "manufacturing": 300, "fleet": 300, "parking": 400, "climate": 300}),
    "edges_ragged": dict(a_seed=9, t0=0, env0=5, k=150),
    "edges_short_limit": dict(a_seed=21, env0=3),                 # t0 = T = 4 * limit + 5, k = 6 * limit
    "final_obs": dict(a_seed=0x5EED, t0=777, env0=3),             # k = 80 (the matrix), 40 (snake's episode ends), 100 (overflow)
}

# ------------------------------------------------------------------------------------------ the reference fixtures the GPU tests replay
FIXTURES = {"snake": ["snake_g10_hash.npz", "snake_g10_greedy.npz", "snake_g20_greedy.npz", "snake_g10_short.npz", "snake_g15_greedy.npz"],
            "crypto": ["crypto_discrete.npz", "crypto_continuous.npz", "crypto_config.npz"],
            "traffic": ["traffic_hash.npz", "traffic_lazy.npz", "traffic_3x3.npz", "traffic_6x6.npz"],
            "climate": ["climate_hash.npz", "climate_small.npz"],
            "hospital": ["hospital_hash.npz", "hospital_surge.npz"],
            "manufacturing": ["manufacturing_hash.npz", "manufacturing_biased.npz", "manufacturing_typea.npz"],
            "fleet": ["fleet_hash.npz", "fleet_courier.npz"],
            "parking": ["parking_hash.npz", "parking_busy.npz"]}

# ------------------------------------------------------------------------------------------ the replay table
SNAKE_GRIDS = [(10, 1000), (6, 77), (16, 130), (20, 65), (15, 200), (4, 70), (5, 129), (7, 300), (13, 66), (23, 65), (30, 70)]
TRAFFIC_LAYOUTS = [dict(grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4),          # simple_test.py:71-76
                   dict(grid_size=(6, 6), num_intersections=16, max_vehicles=80, spawn_rate=0.5),         # USAGE_EXAMPLES.md:32-38
                   dict(grid_size=(2, 7), num_intersections=9, max_vehicles=5, spawn_rate=0.9),           # a non-square grid, a tight vehicle cap
                   dict(grid_size=(2, 2), num_intersections=9, max_vehicles=127, spawn_rate=1.0),         # clamped to 4 intersections; always spawns
                   dict(grid_size=(5, 5), num_intersections=9, max_vehicles=50, spawn_rate=0.0),          # never spawns
                   # intersection counts none of the reference's scripts use (run-time-NI kernels, one per slot count): np.var's pairwise order
                   # below 8 terms, at 8, and with a remainder after the 8-accumulator block; route lengths 2, 2..3, 2..5
                   dict(grid_size=(1, 2), num_intersections=2, max_vehicles=30, spawn_rate=0.6),
                   dict(grid_size=(2, 3), num_intersections=3, max_vehicles=30, spawn_rate=0.5),
                   dict(grid_size=(4, 4), num_intersections=5, max_vehicles=40, spawn_rate=0.5),
                   dict(grid_size=(3, 3), num_intersections=7, max_vehicles=40, spawn_rate=0.5),
                   dict(grid_size=(3, 3), num_intersections=8, max_vehicles=40, spawn_rate=0.5),
                   dict(grid_size=(5, 4), num_intersections=12, max_vehicles=60, spawn_rate=0.5),
                   dict(grid_size=(4, 5), num_intersections=13, max_vehicles=60, spawn_rate=0.5),
                   dict(grid_size=(5, 5), num_intersections=15, max_vehicles=60, spawn_rate=0.5)]
EDGE_LIMITS = {"snake": 7, "crypto": 13, "traffic": 11, "parking": 17, "climate": 9, "fleet": 15, "manufacturing": 19, "hospital": 12}
EDGE_CTOR = {"snake": dict(grid=10), "crypto": dict(action_type="discrete")}
MODES = {"NextStep": 0, "SameStep": 1, "Disabled": 2}


# ------------------------------------------------------------------------------------------ the runs
# test -> batch size, steps, reset seed and env_index0 (and the hash rollout (a_seed, t0, env0, k) run on top).  The GPU tests read their
# sizes and seeds from here and the replay table below is built from the same entries, so the coverage test replays what they run.
RUNS = {
    "hospital_all_modes": dict(n=300, T=1600, T_disabled=1300, seed=30, env0=1),
    "manufacturing_all_modes": dict(n=300, T=1700, T_disabled=1400, seed=30, env0=1),
    "fleet_all_modes": dict(n=400, T=900, seed=30, env0=1),
    "parking_all_modes": dict(n=300, T=1600, seed=60, env0=4),
    "traffic_all_modes": dict(n=333, T=1100, seed=40, env0=2),
    "climate_all_modes": dict(n=500, T=1500, seed=80, env0=6),
    "snake_all_modes": dict(T=300, seed=900, env0=5),                                   # n: SNAKE_GRIDS
    "crypto_step": dict(n=200, T=1100, seed=70, env0=3),
    "crypto_config_knobs": dict(n=257, T=300, limit=120, seed=11, env0=0, rollout=(9, 0, 0, 200)),
    "traffic_layouts": dict(n=200, limit=90, seed=21, env0=5, rollout=(9, 3, 5, 150)),   # T = 2 * limit + 10
    "climate_knobs": dict(n=300, seed=19, env0=2, cases=[(1, 77), (15, 200)], rollout=(4, 1, 2, 150)),   # T = 2 * minutes + 5
    "edges_trajectory": dict(n=150, T=160, seed=41, env0=2),
    "edges_short_limit": dict(n=257, T=lambda limit: 4 * limit + 5, rollout_k=lambda limit: 6 * limit, seed=17, env0=3),
    "edges_ragged": dict(ns=[1, 63, 65], seed=77, env0=5),
    "final_obs": dict(seed=19, env0=3, k=80),
}


def _replays():
    """Every run of a stream above as the GPU tests make it: (id, stream, env type, oracle ctor kwargs, n, T, seed0, mode, stream
    kwargs, hash rollout (a_seed, t0, env0, k) run after the stream or None).  seed0 is the seed of env 0 (reset seed + env_index0)."""
    R = []
    all_modes = ("NextStep", "SameStep", "Disabled")

    def seed0(r):
        return r["seed"] + r["env0"]
    for m in all_modes:
        for env, stream in [("hospital", "hospital_biased"), ("manufacturing", "manufacturing_biased"), ("fleet", "fleet_uniform"),
                            ("parking", "parking_assign_biased"), ("traffic", "traffic_sparse"), ("climate", "climate_uniform")]:
            r = RUNS[env + "_all_modes"]
            R.append((f"{env}_all_modes[{m}]", stream, env, {}, r["n"], r["T_disabled"] if m == "Disabled" and "T_disabled" in r else r["T"], seed0(r), m, {}, None))
        r = RUNS["snake_all_modes"]
        for g, n in SNAKE_GRIDS:
            R.append((f"snake_all_modes[{m}-{g}]", "snake_uniform", "snake", dict(grid=g), n, r["T"], seed0(r), m, {}, None))
    r = RUNS["crypto_step"]
    for kind, m in [("discrete", "SameStep"), ("discrete", "NextStep"), ("discrete", "Disabled"), ("continuous", "SameStep")]:
        R.append((f"crypto_step[{kind}-{m}]", "crypto_uniform", "crypto", dict(action_type=kind), r["n"], r["T"], seed0(r), m, {}, None))
    r = RUNS["crypto_config_knobs"]
    for m in ("SameStep", "NextStep"):
        R.append((f"crypto_config_knobs[{m}]", "crypto_uniform", "crypto", dict(action_type="discrete", max_steps=r["limit"], config="knobs"), r["n"],
                  r["T"], seed0(r), m, dict(seed=5), r["rollout"]))
    r = RUNS["traffic_layouts"]
    for c in TRAFFIC_LAYOUTS:
        R.append((f"traffic_layouts[{c['grid_size']}-{c['num_intersections']}]", "traffic_sparse", "traffic", dict(c, max_steps=r["limit"]), r["n"],
                  2 * r["limit"] + 10, seed0(r), "SameStep", dict(seed=8), r["rollout"]))
    r = RUNS["climate_knobs"]
    for occ, minutes in r["cases"]:
        R.append((f"climate_knobs[{occ}]", "climate_uniform", "climate", dict(max_occupancy=occ, max_steps=minutes), r["n"], 2 * minutes + 5, seed0(r),
                  "SameStep", dict(seed=3), r["rollout"]))
    for env, limit in EDGE_LIMITS.items():
        base = EDGE_CTOR.get(env, {})
        r = RUNS["edges_trajectory"]
        for m in ("NextStep", "SameStep"):
            for short in (False, True):
                R.append((f"edges_trajectory[{env}-{m}-{short}]", "edges_block", env, dict(base, **(dict(max_steps=limit) if short else {})), r["n"], r["T"],
                          seed0(r), m, {}, None))
        r, h = RUNS["edges_short_limit"], HASH_ROLLOUTS["edges_short_limit"]
        for m in all_modes:
            T = r["T"](limit)
            R.append((f"edges_short_limit[{env}-{m}]", "edges_steps", env, dict(base, max_steps=limit), r["n"], T, seed0(r), m, dict(limit=limit),
                      None if m == "Disabled" else (h["a_seed"], T, h["env0"], r["rollout_k"](limit))))
        r, h = RUNS["edges_ragged"], HASH_ROLLOUTS["edges_ragged"]
        for n in r["ns"]:
            R.append((f"edges_ragged[{env}-{n}]", None, env, base, n, 0, seed0(r), "SameStep", {}, (h["a_seed"], h["t0"], h["env0"], h["k"])))
    r, h = RUNS["final_obs"], HASH_ROLLOUTS["final_obs"]
    fin_hash = (h["a_seed"], h["t0"], h["env0"])
    cases = dict(FINAL_OBS_CASES, **{f"snake{g or 'default'}": ("snake", dict(grid=g or 20, max_steps=15)) for g in list(range(4, 31)) + [None]})
    for cid, (env, okw) in cases.items():
        seg = FINAL_OBS_SEGMENT.get(env, 64)
        n = 3 * seg + 37 % seg
        R.append((f"final_obs[{cid}-explicit]", "final_obs_block", env, okw, n, r["k"], seed0(r), "SameStep", {}, None))
        R.append((f"final_obs[{cid}-hash]", None, env, okw, n, 0, seed0(r), "SameStep", {}, fin_hash + (r["k"],)))
    for g in (4, 5, 6, 8):
        okw = dict(grid=g, max_steps=6)
        R.append((f"final_obs_snake_ends[{g}-explicit]", "final_obs_block", "snake", okw, 2048 + 29, 40, seed0(r), "SameStep", dict(seed=g), None))
        R.append((f"final_obs_snake_ends[{g}-hash]", None, "snake", okw, 2048 + 29, 0, seed0(r), "SameStep", {}, fin_hash + (40,)))
    h = HASH_ROLLOUTS["config5"]
    for env, m in [("hospital", 1000), ("manufacturing", 1500), ("fleet", 2500), ("parking", 2000), ("climate", 3000)]:
        for lo in (0, (1 << 17) - m):
            R.append((f"config5[{env}-{lo}]", None, env, {}, m, 0, lo, "SameStep", {}, (h["a_seed"], h["t0"], lo, h["k"][env])))
    return R


# test_final_obs_oracle_gpu.py's CASES as (env type, oracle kwargs), and the device's envs per side-output segment (n = 3 segments + a
# ragged remainder: cge_<env>_final_obs_segment; 64 unless listed)
FINAL_OBS_SEGMENT = {"hospital": 16, "traffic": 16}
FINAL_OBS_CASES = {
    "snake10": ("snake", dict(grid=10, max_steps=9)),
    "crypto": ("crypto", dict(action_type="discrete", max_steps=13)),
    "crypto_continuous": ("crypto", dict(action_type="continuous", max_steps=13)),
    "crypto_config": ("crypto", dict(action_type="discrete", max_steps=13, config="golden")),
    "traffic3x3_4": ("traffic", dict(max_steps=11, grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4)),
    "traffic9": ("traffic", dict(max_steps=11)),
    "traffic4x4_16": ("traffic", dict(max_steps=11, grid_size=(4, 4), num_intersections=16)),
    "traffic4x5_13": ("traffic", dict(max_steps=11, grid_size=(4, 5), num_intersections=13, max_vehicles=60, spawn_rate=0.5)),
    "parking": ("parking", dict(max_steps=17)),
    "climate": ("climate", dict(max_steps=9)),
    "climate_occ1": ("climate", dict(max_steps=9, max_occupancy=1)),
    "climate_occ15": ("climate", dict(max_steps=9, max_occupancy=15)),
    "fleet": ("fleet", dict(max_steps=15)),
    "manufacturing": ("manufacturing", dict(max_steps=19)),
    "hospital": ("hospital", dict(max_steps=12)),
}


REPLAYS = _replays()
CRYPTO_KNOBS = dict(initial_balance=400.0, trading_fee_rate=0.004, slippage_rate=0.002, min_price=5000.0, max_price=80000.0,
                    volatility_base=0.05, market_psychology_factor=0.3)


def make_oracle(oracle, env, okw, n, mode):
    """The oracle of `env` with keyword constructor arguments (snake: grid; crypto: action_type, config)."""
    kw = dict(okw)
    if env == "snake":
        return oracle.SnakeOracle(n, kw.pop("grid"), mode, **kw)
    if env == "crypto":
        if kw.get("config") == "knobs":
            kw["config"] = CRYPTO_KNOBS
        elif kw.get("config") == "golden":                        # the TradingConfig of tests/golden/crypto_config.npz
            import json
            import os
            with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crypto_config.npz")) as z:
                kw["config"] = json.loads(str(z["config"]))
        return oracle.CryptoOracle(n, kw.pop("action_type", "discrete"), mode, **kw)
    return getattr(oracle, ENV_TYPES[env][0])(n, mode, **kw)


def orc_step(o, a, want_final=False):
    return o.step(*a, want_final=want_final) if isinstance(a, tuple) else o.step(a, want_final=want_final)


def stream_sha256(it):
    """SHA-256 over the bytes of every step's action array(s), in order"""
    h = hashlib.sha256()
    for a in it:
        for x in (a if isinstance(a, tuple) else (a,)):
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def pinned_streams():
    """(name, stream) for every stream at the sizes the GPU tests use; tests/golden/action_stream_sha256.json pins their SHA-256
    (recorded from the generators as they stood inside the tests, before they moved here)."""
    yield "hospital_biased n=300 T=1600", hospital_biased("hospital", {}, 300, 1600)
    yield "hospital_biased n=300 T=1300", hospital_biased("hospital", {}, 300, 1300)
    yield "manufacturing_biased n=300 T=1700", manufacturing_biased("manufacturing", {}, 300, 1700)
    yield "manufacturing_biased n=300 T=1400", manufacturing_biased("manufacturing", {}, 300, 1400)
    yield "fleet_uniform n=400 T=900", fleet_uniform("fleet", {}, 400, 900)
    yield "parking_assign_biased n=300 T=1600", parking_assign_biased("parking", {}, 300, 1600)
    for g, n in SNAKE_GRIDS:
        yield f"snake_uniform G={g} n={n} T=300", snake_uniform("snake", dict(grid=g), n, 300)
    for kind in ("discrete", "continuous"):
        yield f"crypto_uniform {kind} n=200 T=1100", crypto_uniform("crypto", dict(action_type=kind), 200, 1100)
    yield "crypto_uniform knobs seed=5 n=257 T=300", crypto_uniform("crypto", dict(action_type="discrete"), 257, 300, seed=5)
    yield "traffic_sparse n=333 T=1100", traffic_sparse("traffic", {}, 333, 1100)
    for c in TRAFFIC_LAYOUTS:
        yield f"traffic_sparse layout {c['grid_size']}/{c['num_intersections']} seed=8 n=200 T=190", traffic_sparse("traffic", c, 200, 190, seed=8)
    yield "climate_uniform n=500 T=1500", climate_uniform("climate", {}, 500, 1500)
    for occ, minutes in [(1, 77), (15, 200)]:
        yield (f"climate_uniform knobs occ={occ} seed=3 n=300 T={2 * minutes + 5}",
               climate_uniform("climate", dict(max_occupancy=occ), 300, 2 * minutes + 5, seed=3))
    for env, limit in EDGE_LIMITS.items():
        yield f"edges_block {env.capitalize()} K=160 n=150", edges_block(env, {}, 150, 160)
        T = 4 * limit + 5
        yield f"edges_steps {env.capitalize()} limit={limit} n=257 T={T}", edges_steps(env, {}, 257, T, limit=limit)
    for cid, (env, okw) in FINAL_OBS_CASES.items():
        seg = FINAL_OBS_SEGMENT.get(env, 64)
        n = 3 * seg + 37 % seg
        yield f"final_obs_block {cid} k=80 n={n}", final_obs_block(env, okw, n, 80)
    for g in (4, 5, 6, 8):
        yield f"final_obs_block snake ends G={g} k=40 n=2077", final_obs_block("snake", dict(grid=g), 2077, 40, seed=g)
    yield "final_obs_block snake every grid k=80 n=229", final_obs_block("snake", dict(grid=7), 229, 80)
