"""The explicit actions a hash-action rollout stands for.

`rollout(k, action_seed=a_seed, t0=t0)` on a batch created with `env_index0=env0` draws the action of env i at step t from the
counter hash u = action_hash(a_seed, env0 + i, t0 + t, j) (tests/golden/gen/common.py; oracle/orc_*.c for each env type).  The
helper below rebuilds those actions as arrays in the layout the oracles' step() takes, so that a test can step the oracle in
SAME_STEP with `want_final=True` and get the terminal rows a hash-action rollout must deliver.  test_oracle_hash_rollout.py pins it
against the oracles' own hash-action rollouts."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_golden_gen_common", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen", "common.py"))
common = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(common)

# env type -> (number of actions per component, components per env step); the components are j = 0, 1, ... of the hash
DISCRETE = {"snake": (4, 1), "crypto": (5, 1), "parking": (8, 1), "fleet": (8, 3), "manufacturing": (25, 1), "hospital": (35, 1)}


def hash_actions(name, a_seed, k, n, t0=0, env0=0, continuous=False, ni=9):
    """Actions of steps t0 .. t0 + k - 1 for envs env0 .. env0 + n - 1, indexed [t, i, ...]:
    int32 [k, n] (snake, crypto, parking, manufacturing, hospital), int32 [k, n, 3] (fleet), int32 [k, n, ni] (traffic: j is the
    intersection), float32 [k, n, 2] (continuous crypto) and (ac_temp float32 [k, n], lights int8 [k, n, 4]) for climate."""
    name = name.lower()
    env = np.arange(env0, env0 + n, dtype=np.uint64)
    if name == "climate":
        from oracle import ClimateOracle
        ac = np.zeros((k, n), np.float32)
        li = np.zeros((k, n, 4), np.int8)
        for t in range(k):
            for i in range(n):
                ac[t, i], li[t, i] = ClimateOracle.hash_action(a_seed, env0 + i, t0 + t)
        return ac, li
    if name == "crypto" and continuous:
        # the two components in [-1, 1): the top 24 bits of the hash of j = 0 and j = 1, scaled in float64, rounded to float32
        out = np.zeros((k, n, 2), np.float32)
        for t in range(k):
            for i in range(n):
                for j in range(2):
                    out[t, i, j] = np.float32((common.action_hash(a_seed, env0 + i, t0 + t, j) >> 40) / 2.0**23 - 1.0)
        return out
    if name == "traffic":
        nact, comps = 3, ni
    else:
        nact, comps = DISCRETE[name]
    a = np.stack([np.stack([common.hash_actions_np(a_seed, env, t0 + t, nact, j) for j in range(comps)], axis=-1) for t in range(k)])
    return a[..., 0] if comps == 1 and name != "traffic" else a


def at(acts, t):
    """Step t of hash_actions()'s result, in the form the oracles' step() takes (climate: a tuple of two arguments)."""
    return tuple(x[t] for x in acts) if isinstance(acts, tuple) else acts[t]
