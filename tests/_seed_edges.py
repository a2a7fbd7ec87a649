"""What tests/test_seed_edges_cpu.py and tests/test_seed_edges_gpu.py share: the fifteen env types by seeding family, the edge seeds,
the step count K of every type, and ONE way to produce the data a seeding test compares, from the reference side (`reference`) and
from a device batch (`device`), as a dict of numpy arrays with the same keys.

The eight types with a CPU oracle compare what tests/test_edges_gpu.py::test_per_env_seed_lists compares: the reset rows, and the
final rows, float64 reward sums and done counts of a K-step hash-action rollout.  The seven types with a Python model
(tests/*_model.py: a real random.Random(int(s)) / np.random.RandomState(int(s)) per env) compare the reset rows and every step of the
K-step rollout: rows, rewards and the flag the type raises; the four record-lane types also the info columns after the last step.
Test infrastructure only: the product never imports it."""
import types

import numpy as np

import _lane_kit as kit
from _lane_model import SAME_STEP

A_SEED = 5                                                                # the hash actions' seed, everywhere
ORACLE = {"Snake": (dict(grid_size=10), "SnakeOracle", (10,)), "Crypto": (dict(action_type="discrete"), "CryptoOracle", ("discrete",)),
          "Traffic": ({}, "TrafficOracle", ()), "Parking": ({}, "ParkingOracle", ()), "Climate": ({}, "ClimateOracle", ()),
          "Fleet": ({}, "FleetOracle", ()), "Manufacturing": ({}, "ManufacturingOracle", ()), "Hospital": ({}, "HospitalOracle", ())}
SLAB = ("Bus", "WorldBuilder", "Restaurant")
LANE = ("Airline", "Emergency", "SpaceStation", "Farm")
TYPES = tuple(ORACLE) + SLAB + LANE
# The seeding family decides where the key grows from one 32-bit limb to two and what the largest seed is.  NumPy legacy
# (np.random.seed -> init_genrand) takes 32 bits and raises above; crypto, fleet and farm seed a CPython stream with the same s_i too.
FAMILY = {"Snake": "cpython", "Traffic": "cpython", "Parking": "cpython", "Hospital": "cpython", "Bus": "cpython", "Restaurant": "cpython",
          "Airline": "cpython", "Emergency": "cpython", "Climate": "seedsequence", "Manufacturing": "seedsequence",
          "Crypto": "numpy_legacy", "Fleet": "numpy_legacy", "WorldBuilder": "numpy_legacy", "SpaceStation": "numpy_legacy", "Farm": "numpy_legacy"}
LEGACY32 = tuple(t for t in TYPES if FAMILY[t] == "numpy_legacy")
WIDE64 = tuple(t for t in TYPES if FAMILY[t] != "numpy_legacy")
ENV_CLASS = {t: t + "VectorEnv" for t in TYPES}
ENV_CLASS["Farm"] = "AgriculturalFarmVectorEnv"


def bits_of(name):
    return 32 if name in LEGACY32 else 64


# The edge seeds of the 64-bit types.  Neighbours alternate between one-limb (< 2**32) and two-limb keys, so that tiling the list
# over a batch puts a key-length switch between every two lanes of a wave.
E = [0, 2 ** 32, 1, 2 ** 32 + 1, 2 ** 31 - 1, 2 ** 33 - 1, 2 ** 31, 7 << 32, 2 ** 32 - 1, 0xFFFFFFFF00000000, 2 ** 40 + 17, 2 ** 63 - 1,
     2 ** 63, 2 ** 64 - 1]
E32 = [s for s in E if s < 2 ** 32]
# what a device that kept only the low (or only the high) word would confuse
TRUNCATION_PAIRS = [(2 ** 32, 0), (2 ** 32 + 1, 1), (7 << 32, 0), (2 ** 64 - 1, 2 ** 32 - 1)]


def edge_seeds(name, n=None):
    """the edge list of the type's width as Python ints, tiled to n"""
    e = E32 if name in LEGACY32 else E
    return list(e) if n is None else [e[i % len(e)] for i in range(n)]


# K per type: the smallest number of hash-action steps (A_SEED) after which the compared reference data of every two distinct edge
# seeds of the type differ, but no fewer than K_FLOOR, so that every type's step kernels draw from the seeded streams a few times
# also where the reset rows alone tell the seeds apart.  tests/test_seed_edges_cpu.py asserts the condition at K and, above the floor,
# that K - 1 steps do not meet it.
K_FLOOR = 8
# The smallest counts themselves: 0 for crypto, climate, fleet, manufacturing, space station and farm (the reset rows differ), 1 for
# snake, traffic, hospital, world builder, airline and emergency, 6 for bus, 15 for parking, 38 for restaurant.
K = {"Snake": 8, "Crypto": 8, "Traffic": 8, "Parking": 15, "Climate": 8, "Fleet": 8, "Manufacturing": 8, "Hospital": 8, "Bus": 8,
     "WorldBuilder": 8, "Restaurant": 38, "Airline": 8, "Emergency": 8, "SpaceStation": 8, "Farm": 8}
K_MAX = 40


def _spec(name):
    """the names of a record-lane type that _lane_kit.make / model / info_of read"""
    import airline_model, emergency_model, farm_model, space_station_model
    return {"Airline": types.SimpleNamespace(m=airline_model, env="AirlineVectorEnv", model=airline_model.AirlineModel, limit=None, info=airline_model.INFO),
            "Emergency": types.SimpleNamespace(m=emergency_model, env="EmergencyVectorEnv", model=emergency_model.EmergencyModel, limit="max_timesteps",
                                               info=emergency_model.INFO),
            "SpaceStation": types.SimpleNamespace(m=space_station_model, env="SpaceStationVectorEnv", model=space_station_model.SpaceStationModel,
                                                  limit="max_steps", info=space_station_model.INFO + ("system_failure_mask",)),
            "Farm": types.SimpleNamespace(m=farm_model, env="AgriculturalFarmVectorEnv", model=farm_model.FarmModel, limit="max_years",
                                          info=farm_model.INFO + farm_model.FIELD_INFO)}[name]


def env_kwargs(name):
    """constructor keywords of the device batch a seeding test makes (beside num_envs, autoreset_mode and env_index0)"""
    if name in ORACLE:
        return dict(ORACLE[name][0])
    return dict(flatten_obs=True) if name == "WorldBuilder" else {}


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the reference side
def reference(name, seeds, k, env0=0, oracle=None, history=None):
    """The compared data of env i seeded with seeds[i] (Python ints), SameStep, stepped k times under the hash actions of envs
    env0 .. env0 + n - 1.  `oracle`: the built CPU oracle module, for the eight types that have one.  history = (seed, steps,
    action seed), oracle types only: the batch was first reset with that base seed and ran that many hash-action steps."""
    seeds = [int(s) for s in seeds]
    n = len(seeds)
    if name in ORACLE:
        _, oname, oargs = ORACLE[name]
        o = getattr(oracle, oname)(n, *oargs, oracle.SAME_STEP)
        if history is not None:
            o.seed(np.arange(n, dtype=np.uint64) + np.uint64(history[0] + env0))
            o.reset()
            o.rollout(history[1], history[2], env0=env0)
        o.seed(np.array(seeds, dtype=np.uint64))
        reset = o.reset()
        out = {"reset": reset}
        if k:
            out["final"], out["reward_sum"], out["done_count"] = o.rollout(k, A_SEED, env0=env0)
        return out
    assert history is None
    if name in LANE:
        spec = _spec(name)
        m = kit.model(spec, seeds, SAME_STEP)
        acts = spec.m.hash_actions(A_SEED, k, n, env0=env0) if k else []
        reset = m.reset()
        steps = [m.step(acts[t])[:3] for t in range(k)]
        return _stacked(reset, steps, info=m.info())
    if name == "Bus":
        import bus_model as bm
        m, acts = bm.BusModel(seeds, bm.MAX_TIMESTEPS, SAME_STEP), bm.hash_actions(A_SEED, max(k, 1), n, env0=env0)
        reset = m.reset()
        steps = [(lambda r: (r[0], r[1], r[3]))(m.step(acts[t])) for t in range(k)]        # bus raises `truncated`
        return _stacked(reset, steps)
    if name == "Restaurant":
        import restaurant_model as rm
        m, acts = rm.RestaurantModel(seeds, 500, SAME_STEP), rm.hash_actions(A_SEED, max(k, 1), n, env0=env0)
        reset = m.reset()
        steps = [(lambda r: (r[0], r[1], r[3]))(m.step(acts[t])) for t in range(k)]        # restaurant raises `truncated`
        return _stacked(reset, steps)
    import world_builder_model as wm
    m, acts = wm.WorldBuilderModel(seeds, 10, SAME_STEP), wm.hash_actions(A_SEED, max(k, 1), n, env0=env0)
    reset = wm.flatten(m.reset())
    steps = [(lambda r: (wm.flatten(r[0]), r[1], r[2]))(m.step(acts[t])) for t in range(k)]
    return _stacked(reset, steps)


def _stack(rows):
    return {key: np.stack([r[key] for r in rows]) for key in rows[0]} if isinstance(rows[0], dict) else np.stack(rows)


def _stacked(reset, steps, info=None):
    out = {"reset": reset}
    if steps:
        out["obs"] = _stack([s[0] for s in steps])
        out["reward"] = np.stack([f32(s[1]) for s in steps])
        out["flag"] = np.stack([np.asarray(s[2], bool) for s in steps])
    if info is not None:
        out["info"] = info
    return out


def truncated_to(ref, k):
    """the data of a k-step run cut from that of a longer run of a MODEL type (whose steps are compared one by one; `info` goes)"""
    cut = lambda v: {key: x[:k] for key, x in v.items()} if isinstance(v, dict) else v[:k]
    out = {"reset": ref["reset"]}
    if k:
        out.update({key: cut(ref[key]) for key in ("obs", "reward", "flag")})
    return out


def per_env_bytes(data):
    """uint8 [n, bytes]: everything the dict holds about env i in row i (the env axis is 0, or 1 under a leading step axis)"""
    n = len(data["reset"][next(iter(data["reset"]))]) if isinstance(data["reset"], dict) else len(data["reset"])
    parts = []

    def take(key, v):
        if isinstance(v, dict):
            for sub in v:
                take(key, v[sub])
            return
        v = np.ascontiguousarray(v if key in ("reset", "final", "reward_sum", "done_count", "info") else np.moveaxis(v, 1, 0))
        assert v.shape[0] == n, (key, v.shape)
        parts.append(v.reshape(n, -1).view(np.uint8))
    for key in data:
        take(key, data[key])
    return np.concatenate(parts, 1)


def all_rows_differ(data):
    rows = per_env_bytes(data)
    return len(np.unique(rows, axis=0)) == len(rows)


# ---------------------------------------------------------------------------------------------------------------- the device side
def make_env(cge, name, n, env_index0=0, **kw):
    return getattr(cge, ENV_CLASS[name])(n, autoreset_mode="SameStep", env_index0=env_index0, **env_kwargs(name), **kw)


def _host(env, name, obs):
    """a device observation (or trajectory) as the reference side holds it"""
    if name in ("Bus", "Restaurant"):
        from _slab_kit import host
        return host(env, obs)                                                  # ONE copy of the slab behind the dict of views
    return obs.cpu().numpy()


def device(env, name, seed, k):
    """reset(seed=seed), then k hash-action steps as ONE fused rollout: the data `reference` returns, from the device"""
    obs, _ = env.reset(seed=seed)
    return device_steps(env, name, k, {"reset": _host(env, name, obs)})


def device_steps(env, name, k, out=None):
    """k hash-action steps from step 0 of the action stream; with `out` (a reset's rows) the whole compared data"""
    out = {} if out is None else out
    if name in ORACLE:
        obs, rs, dc = env.rollout(k, action_seed=A_SEED)
        out["final"], out["reward_sum"], out["done_count"] = obs.cpu().numpy(), rs.cpu().numpy(), dc.cpu().numpy()
        return out
    traj, rt, ft, _, _ = env.rollout(k, action_seed=A_SEED, trajectory=True, per_step=True)
    out["obs"], out["reward"], out["flag"] = _host(env, name, traj), rt.cpu().numpy(), ft.cpu().numpy()
    if name in LANE:
        out["info"] = kit.info_of(_spec(name), env)
    return out


def concat_envs(parts):
    """the data of consecutive shards as that of one batch"""
    def cat(key, vs):
        if isinstance(vs[0], dict):
            return {sub: cat(key, [v[sub] for v in vs]) for sub in vs[0]}
        return np.concatenate(vs, 1 if key in ("obs", "reward", "flag") else 0)
    return {key: cat(key, [p[key] for p in parts]) for key in parts[0]}


def continue_equally(a, b, k=10, t0=1000):
    """two handles in the same state make the same k further steps: torch.equal on every output of a per-step trajectory rollout"""
    import torch
    for x, y in zip(a.rollout(k, action_seed=A_SEED + 1, t0=t0, trajectory=True, per_step=True), b.rollout(k, action_seed=A_SEED + 1, t0=t0, trajectory=True, per_step=True)):
        if isinstance(x, dict):
            assert list(x) == list(y) and all(torch.equal(x[key], y[key]) for key in x)
        else:
            assert x.dtype == y.dtype and torch.equal(x, y)


def assert_same(dev, ref, what):
    """array_equal on bit patterns, dtypes and shapes included; no row is skipped"""
    assert list(dev) == list(ref), (what, list(dev), list(ref))
    for key in ref:
        if isinstance(ref[key], dict):
            assert_same(dev[key], ref[key], (what, key))
            continue
        a, b = np.asarray(dev[key]), np.asarray(ref[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        same = kit.bits(a) == kit.bits(b)
        assert same.all(), (what, key, np.argwhere(~same)[:5])
