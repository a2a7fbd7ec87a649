"""Golden vectors for BusSystemEnv, produced by running the reference's own bus_system_env/*.py (unmodified, imported from the
reference checkout under the stub gymnasium).  Run it in a process of its own: the reference's module names `config`, `utils` and
`environment` collide with the traffic env's.

Protocol: the env never seeds `random` (reset(seed) only reaches the unused gymnasium generator, environment.py:127), so env i is a
fresh BusSystemEnv run alone after `random.seed(seed0 + i)`; on `truncated` the terminal observation is recorded and `env.reset()`
continues the same stream (auto-reset).  Actions: the counter hash (hash_action(a_seed, i, t, 11, bus)), or a dwell mix: env i holds
constant 0 (i % 3 == 0), constant 10 (i % 3 == 1) or hashed dwell times (i % 3 == 2).
Outputs: tests/golden/bus_hash.npz, bus_dwell.npz, bus_short.npz (the reference constructed with max_timesteps=9: a reset every nine
steps, which pins the reset ordering).
"""
import json
import os
import random

import numpy as np

import common

common.use_stubs()
common.add_reference_dir("bus_system_env")
from environment import BusSystemEnv  # noqa: E402  (reference code)

KEYS = ("bus_stops", "bus_states", "bus_remaining_times", "bus_capacities", "bus_passenger_destinations", "stop_waiting_counts",
        "stop_destination_distributions", "timestep", "total_delivered", "total_waiting", "total_onboard")


def action(policy, a_seed, i, t):
    if policy == "dwell" and i % 3 == 0:
        return [0, 0, 0, 0]
    if policy == "dwell" and i % 3 == 1:
        return [10, 10, 10, 10]
    return [common.hash_action(a_seed, i, t, 11, j) for j in range(4)]


def run_env(seed, T, a_seed, i, policy, max_timesteps):
    random.seed(seed)
    env = BusSystemEnv(max_timesteps=max_timesteps)
    obs, info = env.reset(seed=seed)
    out = dict(obs0=obs, A=np.zeros((T, 4), np.int32), R=np.zeros(T, np.float64), TE=np.zeros(T, np.uint8), TR=np.zeros(T, np.uint8),
               C=np.zeros((T, 4), np.int32), O={k: [] for k in KEYS}, resets=[], info_keys=list(info))
    for t in range(T):
        a = action(policy, a_seed, i, t)
        obs, rew, term, trunc, info = env.step(np.array(a, np.int64))
        out["A"][t] = a; out["R"][t] = rew; out["TE"][t] = term; out["TR"][t] = trunc
        out["C"][t] = [info["timestep"], info["total_delivered"], info["total_waiting"], info["total_onboard"]]
        assert list(info["bus_positions"]) == list(obs["bus_stops"]) and list(info["bus_capacities"]) == list(obs["bus_capacities"])
        assert [s == "stopped" for s in info["bus_states"]] == [bool(v) for v in obs["bus_states"]]
        assert list(info["stop_waiting"]) == list(obs["stop_waiting_counts"])
        for k in KEYS:
            out["O"][k].append(np.asarray(obs[k]))
        if term or trunc:
            obs, _ = env.reset()
            out["resets"].append((t, obs))
    return env, out


def space_record(env):
    """keys, shapes, dtypes and bounds of the reference's spaces (settings only)."""
    rec = {}
    for k, sp in env.observation_space.spaces.items():
        kind = type(sp).__name__
        d = dict(kind=kind, shape=list(sp.shape), dtype=str(sp.dtype))
        if kind == "Box":
            d.update(low=float(sp.low.min()), high=float(sp.high.max()))
        elif kind == "MultiDiscrete":
            d.update(nvec=[int(v) for v in sp.nvec])
        elif kind == "Discrete":
            d.update(n=int(sp.n))
        elif kind == "MultiBinary":
            d.update(n=int(sp.n))
        rec[k] = d
    return dict(observation=rec, action=dict(kind=type(env.action_space).__name__, nvec=[int(v) for v in env.action_space.nvec]))


def make(name, n_envs, T, seed0, a_seed, policy, max_timesteps=500):
    rows = [run_env(seed0 + i, T, a_seed, i, policy, max_timesteps) for i in range(n_envs)]
    env = rows[0][0]
    rows = [r[1] for r in rows]
    ridx = [(i, t) for i, r in enumerate(rows) for t, _ in r["resets"]]
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), max_timesteps=np.int64(max_timesteps),
                  actions=np.stack([r["A"] for r in rows]), reward=np.stack([r["R"] for r in rows]),
                  terminated=np.stack([r["TE"] for r in rows]), truncated=np.stack([r["TR"] for r in rows]),
                  counters=np.stack([r["C"] for r in rows]).astype(np.int16), reset_index=np.array(ridx, np.int32).reshape(-1, 2),
                  spaces=np.array(json.dumps(space_record(env))), info_keys=np.array(json.dumps(rows[0]["info_keys"])),
                  versions=np.array(json.dumps(common.versions())))
    for k in KEYS:      # every value is below 2**15 (counts <= 150, timestep <= 500): int16 keeps the files small
        arrays["obs0_" + k] = np.stack([np.asarray(r["obs0"][k]) for r in rows]).astype(np.int16)
        arrays["obs_" + k] = np.stack([np.stack(r["O"][k]) for r in rows]).astype(np.int16)
        shape = arrays["obs0_" + k].shape[1:]
        arrays["reset_" + k] = np.array([np.asarray(ob[k]) for r in rows for _, ob in r["resets"]], np.int16).reshape((-1,) + shape)
    out = os.path.join(common.GOLDEN, name + ".npz")
    np.savez_compressed(out, **arrays)
    print(name, "episodes", len(ridx), "sum reward", arrays["reward"].sum(), "max waiting at a stop", arrays["obs_stop_waiting_counts"].max(),
          "delivered", arrays["counters"][:, :, 1].max(), os.path.getsize(out), "bytes")


if __name__ == "__main__":
    make("bus_hash", 16, 1100, seed0=900, a_seed=123, policy="hash")
    make("bus_dwell", 12, 1100, seed0=950, a_seed=31, policy="dwell")
    make("bus_short", 8, 300, seed0=980, a_seed=77, policy="hash", max_timesteps=9)
