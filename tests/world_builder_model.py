"""NumPy model of n independent WorldBuilderEnv instances (world_builder_env/src/environment/world_builder_env.py, game_logic.py).

tests/test_world_builder_cpu.py pins it, value for value, to fixtures recorded from the unmodified reference (tests/golden/wb_*.npz);
the GPU tests then use it where the fixtures cannot reach (large batches, other grid sizes, the three autoreset modes).  Test
infrastructure only: the product never imports it.

Env i draws from `np.random.RandomState(seeds[i])`: the legacy stream `np.random.seed(seeds[i])` gives the reference when it runs alone
(its _try_build calls the global np.random.randint, game_logic.py:130).  reset() draws nothing.
"""
import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP  # noqa: F401

KEYS = ("grid", "resources", "population_capacity", "win_steps")
MAX_POPULATION, WIN_STEPS = 20, 50                                         # world_builder_env.py:45-46
COST_WOOD = np.array([0, 5, 0, 5, 10])                                      # game_logic.py:15-20, by action
COST_STONE = np.array([0, 0, 3, 0, 5])
BUILD_REWARD = np.array([0, 3, 2, 2, 4])                                    # :74-81
HEADER_INTS, KEY_WORDS = 16, 624


def state_bytes(grid_size):
    """Bytes of one canonical record (include/cge_amd.h): 16 int32, the grid as int8 padded to a multiple of 4, uint32 key[624]."""
    return 4 * HEADER_INTS + (grid_size * grid_size + 3) // 4 * 4 + 4 * KEY_WORDS


def pack_state(header, grid, key):
    """header int32 [n, 16], grid int8 [n, G * G], key uint32 [n, 624] -> uint8 [n, state_bytes]."""
    n, gg = grid.shape
    rec = np.zeros((n, 4 * HEADER_INTS + (gg + 3) // 4 * 4 + 4 * KEY_WORDS), np.uint8)
    rec[:, :64] = np.ascontiguousarray(header, "<i4").view(np.uint8).reshape(n, 64)
    rec[:, 64:64 + gg] = np.ascontiguousarray(grid, np.int8).view(np.uint8)
    rec[:, -4 * KEY_WORDS:] = np.ascontiguousarray(key, "<u4").view(np.uint8).reshape(n, 4 * KEY_WORDS)
    return rec


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None):
    """int32 [k, n]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for: hash_action(a_seed, env0 + i, t0 + t, 5, 0)."""
    return _lane_model.hash_actions(a_seed, k, n, 5, t0, env0, envs)


def flatten(obs):
    """The reference's flatten_obs=True layout (world_builder_env.py:205-216) of a dict observation: float32 [..., G * G + 6]."""
    g = obs["grid"]
    lead = g.shape[:-2]
    return np.concatenate([g.reshape(lead + (-1,)).astype(np.float32), obs["resources"].astype(np.float32),
                           obs["population_capacity"].astype(np.float32), obs["win_steps"].astype(np.float32)], axis=-1)


class WorldBuilderModel:
    def __init__(self, seeds, grid_size=10, mode=SAME_STEP, flatten_obs=False):
        self.n = n = len(seeds)
        self.G, self.mode, self.flat = int(grid_size), mode, bool(flatten_obs)
        self.rng = [np.random.RandomState(int(s)) for s in seeds]
        i64 = np.int64
        self.grid = np.zeros((n, self.G * self.G), np.int8)
        self.food, self.wood, self.stone = np.zeros(n, i64), np.zeros(n, i64), np.zeros(n, i64)
        self.pop, self.cap = np.zeros(n, i64), np.zeros(n, i64)
        self.counts = np.zeros((n, 5), i64)                                 # by building id; column 0 unused
        self.steps, self.win = np.zeros(n, i64), np.zeros(n, i64)
        self.latch = np.zeros(n, bool)
        self.needs_reset = np.zeros(n, bool)
        self.ret = np.zeros(n, np.float64)
        self.ep_r, self.ep_l = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self.invalid = 0
        self.words = np.zeros(n, np.int64)                                  # generator words the last step() consumed
        self._reset(np.ones(n, bool))

    def _reset(self, m):                                                    # game_logic.py:31-54, world_builder_env.py:99-121
        self.grid[m] = 0
        self.food[m], self.wood[m], self.stone[m] = 25, 20, 10
        self.pop[m], self.cap[m] = 3, 10
        self.counts[m] = 0
        self.steps[m] = 0; self.win[m] = 0; self.latch[m] = False
        self.needs_reset[m] = False
        self.ret[m] = 0.0

    def reset(self, mask=None):
        self._reset(np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool))
        return self.obs()

    def obs(self):
        d = {"grid": self.grid.reshape(self.n, self.G, self.G).copy(),
             "resources": np.stack([self.food, self.wood, self.stone, self.pop], 1).astype(np.float32),
             "population_capacity": self.cap[:, None].astype(np.float32), "win_steps": self.win[:, None].astype(np.int32)}
        return flatten(d) if self.flat else d

    def info(self):
        """int64 [n, 12] in the fixtures' INFO_KEYS order."""
        return np.stack([self.steps, self.win, self.latch.astype(np.int64), self.food, self.wood, self.stone, self.pop, self.cap,
                         self.counts[:, 1], self.counts[:, 2], self.counts[:, 3], self.counts[:, 4]], 1)

    def _pos(self, i):
        return int(self.rng[i].get_state()[2])

    def step(self, actions):
        """-> (obs, reward float64, terminated, final_obs): final_obs is the observation before the SAME_STEP reset (the reference's
        own step() output); obs == final_obs where no reset happened."""
        a = np.asarray(actions).astype(np.int64)
        n = self.n
        reset_now = self.needs_reset.copy() if self.mode == NEXT_STEP else np.zeros(n, bool)
        valid = (a >= 0) & (a <= 4)
        self.invalid += int((~valid & ~reset_now).sum())
        go = valid & ~reset_now
        a = np.where(go, a, 0)
        reward = np.zeros(n, np.int64)
        self.words[:] = 0
        self.steps[go] += 1
        prev_pop, prev_cap = self.pop.copy(), self.cap.copy()
        build = go & (a > 0)
        afford = build & (self.wood >= COST_WOOD[a]) & (self.stone >= COST_STONE[a])
        ok = np.zeros(n, bool)
        for i in np.flatnonzero(afford):                                    # _try_build :118-150
            empty = np.flatnonzero(self.grid[i] == 0)
            if len(empty) == 0:
                continue
            p0 = self._pos(i)
            idx = self.rng[i].randint(len(empty))
            self.words[i] = (self._pos(i) - p0) % 624
            self.grid[i, empty[idx]] = a[i]
            ok[i] = True
        self.wood -= np.where(ok, COST_WOOD[a], 0)
        self.stone -= np.where(ok, COST_STONE[a], 0)
        self.counts[np.flatnonzero(ok), a[ok]] += 1
        self.cap += np.where(ok & (a == 4), 5, 0)
        reward += np.where(ok, BUILD_REWARD[a], 0) + np.where(ok & (a == 4) & (prev_pop >= prev_cap - 1), 10, 0) - np.where(build & ~ok, 3, 0)
        g = go.astype(np.int64)
        self.food += 2 * self.counts[:, 1] * g                              # _process_production :164-174
        self.wood += 3 * self.counts[:, 2] * g
        self.stone += 2 * self.counts[:, 3] * g
        starve = go & (self.food < self.pop)                                # _process_consumption :176-183
        self.food -= np.where(go & ~starve, self.pop, 0)
        self.pop[starve] = 0
        grow = go & (self.pop > 0) & (self.food > 2) & (self.pop < self.cap)   # _process_population_growth :185-194
        self.pop += grow
        self.food -= grow
        shaping = (5 * (self.pop > prev_pop) - 50 * (self.pop < prev_pop) + (self.food > 2 * self.pop) - 2 * (self.food < self.pop)
                   - 5 * (self.food < np.maximum(2, self.pop)) + (np.abs(self.wood - self.stone) < 5) - ((a == 1) & (self.food > 3 * self.pop)))
        reward += shaping * g                                               # :95-114
        self.latch |= go & (self.pop >= MAX_POPULATION)                     # world_builder_env.py:141-146
        self.win += go & self.latch
        lose = go & (self.pop <= 0)
        won = go & ~lose & self.latch & (self.win >= WIN_STEPS)
        term = lose | won
        reward = np.where(lose, -100, np.where(won, 100, reward))           # :153-159 (the -50 branch is unreachable)
        self.ret += reward
        self.ep_r[term] = self.ret[term]
        self.ep_l[term] = self.steps[term]
        final = self.obs()
        if self.mode == SAME_STEP:
            self._reset(term)
        elif self.mode == NEXT_STEP:
            self._reset(reset_now)
            self.needs_reset |= term
        return self.obs(), reward.astype(np.float64), term, final

    def get_state(self):
        hdr = np.zeros((self.n, HEADER_INTS), np.int64)
        hdr[:, :13] = np.stack([self.food, self.wood, self.stone, self.pop, self.cap, self.counts[:, 1], self.counts[:, 2], self.counts[:, 3],
                                self.counts[:, 4], self.steps, self.win, self.latch, self.needs_reset], 1)
        st = [r.get_state() for r in self.rng]
        hdr[:, 13] = [s[2] for s in st]
        return pack_state(hdr.astype(np.int32), self.grid, np.stack([s[1] for s in st]))

    def set_state(self, rec):
        """the inverse of get_state(); the running return restarts at zero, as the device's does"""
        rec = np.ascontiguousarray(rec, np.uint8)
        gg = self.G * self.G
        hdr = rec[:, :64].copy().view("<i4").astype(np.int64)
        self.food, self.wood, self.stone, self.pop, self.cap = (hdr[:, k].copy() for k in range(5))
        self.counts[:, 1:5] = hdr[:, 5:9]
        self.steps, self.win = hdr[:, 9].copy(), hdr[:, 10].copy()
        self.latch, self.needs_reset = hdr[:, 11].astype(bool), hdr[:, 12].astype(bool)
        self.grid = rec[:, 64:64 + gg].copy().view(np.int8)
        key = rec[:, -4 * KEY_WORDS:].copy().view("<u4")
        for i, r in enumerate(self.rng):
            r.set_state(("MT19937", key[i], int(hdr[i, 13]), 0, 0.0))
        self.ret[:] = 0.0
