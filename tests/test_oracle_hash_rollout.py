"""tests/_hash_actions.py against the oracles (no GPU): for every env type and the config variants the GPU side-output tests run,
stepping an oracle with the helper's actions ends in the same last observation, reward sums and done counts as that oracle's own
hash-action rollout (oracle/orc_*.c) from the same state, with a nonzero t0 and env_index0.  The GPU tests step the oracle with
these actions to get the terminal rows a hash-action rollout must deliver; this pins the helper before any of them relies on it."""
import numpy as np
import pytest

from _hash_actions import at, hash_actions

# id: (env type, oracle class, oracle kwargs with a short time limit, helper kwargs)
CASES = {
    "snake4": ("snake", "SnakeOracle", dict(grid=4, max_steps=9), {}),
    "snake20": ("snake", "SnakeOracle", dict(grid=20, max_steps=25), {}),
    "snake23": ("snake", "SnakeOracle", dict(grid=23, max_steps=25), {}),
    "crypto": ("crypto", "CryptoOracle", dict(action_type="discrete", max_steps=13), {}),
    "crypto_continuous": ("crypto", "CryptoOracle", dict(action_type="continuous", max_steps=13), dict(continuous=True)),
    "crypto_config": ("crypto", "CryptoOracle", dict(action_type="discrete", max_steps=13, config="golden"), {}),
    "traffic3x3_4": ("traffic", "TrafficOracle", dict(max_steps=11, grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4), dict(ni=4)),
    "traffic9": ("traffic", "TrafficOracle", dict(max_steps=11), dict(ni=9)),
    "traffic4x4_16": ("traffic", "TrafficOracle", dict(max_steps=11, grid_size=(4, 4), num_intersections=16), dict(ni=16)),
    "traffic4x5_13": ("traffic", "TrafficOracle", dict(max_steps=11, grid_size=(4, 5), num_intersections=13, max_vehicles=60, spawn_rate=0.5), dict(ni=13)),
    "parking": ("parking", "ParkingOracle", dict(max_steps=17), {}),
    "climate": ("climate", "ClimateOracle", dict(max_steps=9), {}),
    "climate_occ1": ("climate", "ClimateOracle", dict(max_steps=9, max_occupancy=1), {}),
    "climate_occ15": ("climate", "ClimateOracle", dict(max_steps=9, max_occupancy=15), {}),
    "fleet": ("fleet", "FleetOracle", dict(max_steps=15), {}),
    "manufacturing": ("manufacturing", "ManufacturingOracle", dict(max_steps=19), {}),
    "hospital": ("hospital", "HospitalOracle", dict(max_steps=12), {}),
}


def crypto_config():
    import json
    from conftest import golden
    return json.loads(str(golden("crypto_config.npz")["config"]))


def make_oracle(oracle, cls, kw, n, mode):
    kw = dict(kw)
    if cls == "SnakeOracle":
        return oracle.SnakeOracle(n, kw.pop("grid"), mode, **kw)
    if cls == "CryptoOracle":
        if kw.get("config") == "golden":
            kw["config"] = crypto_config()
        return oracle.CryptoOracle(n, kw.pop("action_type"), mode, **kw)
    return getattr(oracle, cls)(n, mode, **kw)


def _step(o, a):
    return o.step(*a) if isinstance(a, tuple) else o.step(a)


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
@pytest.mark.parametrize("case", list(CASES))
def test_stepping_with_the_helpers_actions_equals_the_hash_rollout(oracle, case, mode):
    name, cls, kw, hkw = CASES[case]
    code = {"SameStep": oracle.SAME_STEP, "NextStep": oracle.NEXT_STEP}[mode]
    n, k, a_seed, t0, env0 = 37, 60, 0xC0FFEE, 1234, 3
    ref, stepped = make_oracle(oracle, cls, kw, n, code), make_oracle(oracle, cls, kw, n, code)
    for o in (ref, stepped):
        o.seed(np.arange(n, dtype=np.uint64) + np.uint64(env0 + 29))
        o.reset()
    obs_r, rs_r, dc_r = ref.rollout(k, a_seed, t0=t0, env0=env0)
    acts = hash_actions(name, a_seed, k, n, t0=t0, env0=env0, **hkw)
    rs = np.zeros(n, np.float32 if name == "snake" else np.float64)
    dc = np.zeros(n, np.int32)
    for t in range(k):
        obs, r, te, tr = _step(stepped, at(acts, t))
        rs += r if name == "snake" else stepped.last_reward64          # the rollouts sum snake's float32 rewards, the others' float64
        dc += (te | tr).astype(np.int32)
    assert obs.dtype == obs_r.dtype and np.array_equal(obs.view(np.uint8), obs_r.view(np.uint8)), case
    assert rs.dtype == rs_r.dtype and np.array_equal(rs, rs_r), case
    assert np.array_equal(dc, dc_r), case
    assert dc.min() >= 2, "every env ends episodes inside the run"
    # a different seed, t0 or env_index0 gives different actions: the helper really depends on all three
    base = hash_actions(name, a_seed, 4, n, t0=t0, env0=env0, **hkw)
    for other in (dict(a_seed=a_seed + 1, t0=t0, env0=env0), dict(a_seed=a_seed, t0=t0 + 1, env0=env0), dict(a_seed=a_seed, t0=t0, env0=env0 + 1)):
        b = hash_actions(name, other.pop("a_seed"), 4, n, **other, **hkw)
        assert any(not np.array_equal(x, y) for x, y in zip(base if isinstance(base, tuple) else (base,), b if isinstance(b, tuple) else (b,)))
