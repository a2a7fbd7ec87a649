"""Golden vectors for WorldBuilderEnv, produced by running the reference's own world_builder_env/src/environment/*.py (unmodified,
imported from the reference checkout under the stub gymnasium / pygame).

Protocol: the env never seeds the generator it draws from (reset(seed) reaches only the unused np_random; _try_build uses the global
np.random.randint, game_logic.py:130), so env i is a fresh WorldBuilderEnv run alone after `np.random.seed(seed0 + i)`; on
`terminated` the terminal observation is recorded and `env.reset()` continues the same stream (auto-reset; reset() draws nothing).

Policies (they read the env's internals; the fixture records the resulting actions and the tests replay those):
  hash     hash_action(a_seed, i, t, 5)
  builder  a scripted builder that reaches 20 population; one step in four is replaced by a hashed action
  nohouse  farms until 2 * farms >= population + 2, then 3 lumberyards, 2 quarries, then a hashed BUILD action every step, also when
           the grid is full or the building unaffordable: the grid fills, no episode of a 10 x 10 grid ends

Per fixture: seed0, a_seed, grid_size, flatten_obs, actions, reward (float64), terminated, the reset observation obs0_*, the per-step
observation obs_* as its four pieces (grid int8; resources, population_capacity, win_steps int32: the reference's float32 values
are whole numbers, asserted here), reset_index [m, 2] = (env, step) with the post-reset observations reset_*, info [n, T, 12]
(INFO_KEYS order), words [n, T] uint8 = generator words the step consumed (np.random.get_state()[2] deltas), the spaces record of both
layouts, versions.  wb_flat additionally holds the flattened float32 observations exactly as the reference returned them.

State checkpoints (wb_hash, wb_fill): ck_steps [S] (sorted; s = the state after s steps, after the auto-reset when step s - 1 ended
an episode) and, per env and checkpoint, ck_header int32 [n, S, 16] in the order of the canonical record (include/cge_amd.h),
ck_grid int8 [n, S, G * G] and ck_key uint32 [n, S, 624]; (ck_key, header int 13) = np.random.get_state()[1:3].  The steps are the union over the envs
of a fixed list and of the steps just before and just after the env's first two regenerations of the generator (the one the first draw
after seeding causes, pos 624, and the first crossing of word 624 after it, where the stream gets that far).  Stored env-major, so the
unchanged keys of consecutive checkpoints deflate to almost nothing.
"""
import json
import os

import numpy as np

import common

common.use_stubs()
common.add_reference_dir("world_builder_env")
from src.environment.world_builder_env import WorldBuilderEnv  # noqa: E402  (reference code)

INFO_KEYS = ("steps", "win_steps", "reached_win_population", "food", "wood", "stone", "population", "population_capacity", "farm",
             "lumberyard", "quarry", "house")
PIECES = ("grid", "resources", "population_capacity", "win_steps")


def builder(env):
    g = env.game_logic
    r, c = g.resources, g.building_counts
    prod_food = 2 * c["farm"]
    target = min(g.population_capacity, 20)
    if prod_food < g.population + 1 and r["wood"] >= 5:
        return 1
    if c["lumberyard"] < 2 + c["farm"] // 3 and r["stone"] >= 3:
        return 2
    if c["quarry"] < 1 + c["farm"] // 4 and r["wood"] >= 5:
        return 3
    if prod_food < target + 2 and r["wood"] >= 5:
        return 1
    if g.population_capacity < 20 and r["wood"] >= 10 and r["stone"] >= 5 and prod_food >= g.population_capacity:
        return 4
    return 0


def nohouse(env, a_seed, i, t):
    g = env.game_logic
    r, c = g.resources, g.building_counts
    if 2 * c["farm"] < g.population + 2 and r["wood"] >= 5:
        return 1
    if c["lumberyard"] < 3 and r["stone"] >= 3:
        return 2
    if c["quarry"] < 2 and r["wood"] >= 5:
        return 3
    return 1 + common.hash_action(a_seed, i, t, 3)


def action(policy, env, a_seed, i, t):
    if policy == "hash":
        return common.hash_action(a_seed, i, t, 5)
    if policy == "builder":
        return builder(env) if common.hash_action(a_seed, i, t, 4) else common.hash_action(a_seed, i, t, 5, 1)
    return nohouse(env, a_seed, i, t)


def pieces(env, obs):
    """The observation as (grid int8 [G, G], resources int32 [4], capacity int32, win_steps int32); whole numbers, asserted."""
    G = env.grid_size
    if env.flatten_obs:
        assert obs.dtype == np.float32 and obs.shape == (G * G + 6,)
        grid, res, cap, win = obs[:G * G].reshape(G, G), obs[G * G:G * G + 4], obs[G * G + 4:G * G + 5], obs[G * G + 5:]
    else:
        assert list(obs) == list(PIECES)
        grid, res, cap, win = (obs[k] for k in PIECES)
        assert grid.dtype == np.int8 and res.dtype == np.float32 and cap.dtype == np.float32 and win.dtype == np.int32
    out = grid.astype(np.int8), res.astype(np.int32), np.int32(cap[0]), np.int32(win[0])
    assert np.array_equal(out[0], grid) and np.array_equal(out[1], res) and out[2] == cap[0] and out[3] == win[0]
    return out


def info_row(info):
    r, c = info["resources"], info["building_counts"]
    return [info["steps"], info["win_steps"], int(info["reached_win_population"]), r["food"], r["wood"], r["stone"], info["population"],
            info["population_capacity"], c["farm"], c["lumberyard"], c["quarry"], c["house"]]


def checkpoint(env):
    g = env.game_logic
    st = np.random.get_state()
    assert st[0] == "MT19937"
    c = g.building_counts
    hdr = [g.resources["food"], g.resources["wood"], g.resources["stone"], g.population, g.population_capacity, c["farm"], c["lumberyard"],
           c["quarry"], c["house"], env.steps, env.win_steps, int(env.reached_win_population), 0, int(st[2]), 0, 0]
    return np.array(hdr, np.int32), g.grid.reshape(-1).astype(np.int8), np.asarray(st[1], np.uint32).copy()


def run_env(seed, T, a_seed, i, policy, G, flat, ck_steps=None):
    """ck_steps None: no checkpoints are kept, the regeneration steps are returned; else checkpoints at those steps."""
    np.random.seed(seed)
    env = WorldBuilderEnv(grid_size=G, flatten_obs=flat)
    obs, info = env.reset(seed=seed)
    assert list(info) == ["steps", "win_steps", "reached_win_population", "resources", "population", "population_capacity", "building_counts"]
    out = dict(obs0=pieces(env, obs), raw0=obs, A=np.zeros(T, np.int32), R=np.zeros(T, np.float64), TE=np.zeros(T, np.uint8), W=np.zeros(T, np.uint8),
               I=np.zeros((T, 12), np.int32), O=[], raw=[], resets=[], regen=[], ck={})
    if ck_steps is not None and 0 in ck_steps:
        out["ck"][0] = checkpoint(env)
    for t in range(T):
        a = action(policy, env, a_seed, i, t)
        p0 = np.random.get_state()[2]
        obs, rew, term, trunc, info = env.step(a)
        p1 = np.random.get_state()[2]
        assert not trunc and float(rew) == int(rew)
        words = (p1 - p0) % 624                                  # pos stays at 624 until the next draw regenerates the key
        if p1 < p0:
            out["regen"].append(t)
        out["A"][t] = a; out["R"][t] = rew; out["TE"][t] = term; out["W"][t] = words; out["I"][t] = info_row(info)
        out["O"].append(pieces(env, obs)); out["raw"].append(obs)
        if term:
            obs, _ = env.reset()
            out["resets"].append((t, pieces(env, obs), obs))
        if ck_steps is not None and t + 1 in ck_steps:
            out["ck"][t + 1] = checkpoint(env)
    return env, out


def space_record(G):
    """keys, shapes, dtypes and bounds of the reference's spaces in both layouts (settings only)."""
    d = WorldBuilderEnv(grid_size=G).observation_space
    f = WorldBuilderEnv(grid_size=G, flatten_obs=True)
    rec = {k: dict(kind=type(sp).__name__, shape=list(sp.shape), dtype=str(sp.dtype), low=float(sp.low.min()), high=float(sp.high.max()))
           for k, sp in d.spaces.items()}
    fo = f.observation_space
    return dict(dict_keys=list(d.spaces), observation=rec,
                flat=dict(kind=type(fo).__name__, shape=list(fo.shape), dtype=str(fo.dtype), low=float(fo.low.min()), high=float(fo.high.max())),
                action=dict(kind=type(f.action_space).__name__, n=int(f.action_space.n)))


def make(name, n_envs, T, seed0, a_seed, policy, G=10, flat=False, ck_fixed=None):
    ck_steps = None
    if ck_fixed is not None:
        steps = set(ck_fixed)
        for i in range(n_envs):
            regen = run_env(seed0 + i, T, a_seed, i, policy, G, flat)[1]["regen"]
            for t in regen[:2]:
                steps.update((t, t + 1))
        ck_steps = sorted(s for s in steps if s <= T)
    rows = [run_env(seed0 + i, T, a_seed, i, policy, G, flat, ck_steps)[1] for i in range(n_envs)]
    ridx = [(i, t) for i, r in enumerate(rows) for t, _, _ in r["resets"]]
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), grid_size=np.int64(G), flatten_obs=np.bool_(flat),
                  actions=np.stack([r["A"] for r in rows]), reward=np.stack([r["R"] for r in rows]), terminated=np.stack([r["TE"] for r in rows]),
                  words=np.stack([r["W"] for r in rows]), info=np.stack([r["I"] for r in rows]), info_keys=np.array(json.dumps(INFO_KEYS)),
                  reset_index=np.array(ridx, np.int32).reshape(-1, 2), spaces=np.array(json.dumps(space_record(G))),
                  versions=np.array(json.dumps(common.versions())))
    shapes = ((G, G), (4,), (), ())
    for j, k in enumerate(PIECES):
        dt = np.int8 if k == "grid" else np.int32
        arrays["obs0_" + k] = np.stack([r["obs0"][j] for r in rows]).astype(dt)
        arrays["obs_" + k] = np.stack([np.stack([o[j] for o in r["O"]]) for r in rows]).astype(dt)
        arrays["reset_" + k] = np.array([ob[j] for r in rows for _, ob, _ in r["resets"]], dt).reshape((-1,) + shapes[j])
    if flat:
        arrays["obs0_flat"] = np.stack([r["raw0"] for r in rows])
        arrays["obs_flat"] = np.stack([np.stack(r["raw"]) for r in rows])
        arrays["reset_flat"] = np.array([raw for r in rows for _, _, raw in r["resets"]], np.float32).reshape(-1, G * G + 6)
        assert arrays["obs_flat"].dtype == np.float32 and arrays["obs0_flat"].dtype == np.float32
    if ck_steps is not None:
        arrays["ck_steps"] = np.array(ck_steps, np.int32)
        for j, k in enumerate(("ck_header", "ck_grid", "ck_key")):
            arrays[k] = np.stack([np.stack([r["ck"][s][j] for s in ck_steps]) for r in rows])
    out = os.path.join(common.GOLDEN, name + ".npz")
    np.savez_compressed(out, **arrays)
    print(name, "episodes", len(ridx), "rewards", sorted(set(arrays["reward"].ravel().tolist()))[:3], "...", arrays["reward"].max(), "max words",
          arrays["words"].max(), "words per env", arrays["words"].sum(1).min(), "-", arrays["words"].sum(1).max(), "max resource",
          arrays["obs_resources"].max(), "checkpoints", None if ck_steps is None else len(ck_steps), os.path.getsize(out), "bytes")


if __name__ == "__main__":
    make("wb_hash", 16, 2400, seed0=100, a_seed=7, policy="hash", ck_fixed=(0, 1, 7, 500, 1999))
    make("wb_builder", 12, 400, seed0=200, a_seed=7, policy="builder")
    make("wb_fill", 8, 400, seed0=300, a_seed=5, policy="nohouse", ck_fixed=(0, 1, 7, 99, 100, 399))
    make("wb_g7", 8, 300, seed0=300, a_seed=5, policy="nohouse", G=7)
    make("wb_g3", 4, 200, seed0=300, a_seed=5, policy="nohouse", G=3)
    make("wb_g2", 4, 100, seed0=300, a_seed=5, policy="nohouse", G=2)
    make("wb_flat", 4, 200, seed0=200, a_seed=7, policy="builder", flat=True)
