"""Counts-and-lists model of the reference's RestaurantEnv (restaurant_env_updated/restaurant_env.py, entities.py) in plain Python.

What the reference keeps as objects reduces to small lists: a waiting customer is (tag, wait_time); a busy waiter is (task, remaining,
table) plus, for a seating task, the customer it carries; a table is (occupied, dirty) plus its guest's state (ORDERED or EATING, when
eating started, the guest's frozen wait_time); a cooking order is (tag, table, progress, order_time), a ready one (tag, table,
order_time).  A customer whose seating failed (the table was taken first) stays WAITING in the reference's `customers` forever: only
_get_info sees such ghosts, so a count and a wait sum stand for them.  The id columns are the serial-number convention of
tests/golden/gen/gen_restaurant.py: one counter per env, restarted by every reset, taken by arrivals and by Kitchen.add_order.

tests/test_restaurant_cpu.py pins the model to fixtures recorded from the unmodified reference; the GPU tests then use it where the
fixtures cannot reach (other batch sizes, other autoreset modes).  Test infrastructure only: the product never imports it.

Env i draws from `random.Random(seeds[i])`, the stream `random.seed(seeds[i])` gives the reference when it runs alone.
"""
import random

import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP  # noqa: F401

KEYS = ("waiting_customers", "waiter_status", "table_occupancy", "table_cleanliness", "kitchen_queue", "ready_orders", "current_timestep")
KEY_SHAPES = {"waiting_customers": (50, 2), "waiter_status": (10, 3), "table_occupancy": (10,), "table_cleanliness": (10,),
              "kitchen_queue": (50, 3), "ready_orders": (20, 2), "current_timestep": (1,)}
ACTION_KEYS = ("type", "waiter_id", "customer_id", "table_id")
NVEC = (4, 10, 50, 10)
INFO = ("current_timestep", "waiting_customers", "idle_waiters", "kitchen_queue_length", "ready_orders", "dirty_tables", "customers_served",
        "customers_left", "tables_cleaned", "orders_served", "wait_time_sum", "num_customers")
SEAT, SERVE, CLEAN = 1, 2, 3
DURATION = {SEAT: 2, SERVE: 1, CLEAN: 3}


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None, nvec=NVEC):
    """int32 [k, n, 4]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for — column c of env i at step t is
    hash_action(a_seed, env0 + i, t0 + t, nvec[c], c).  envs: global env indices instead of env0 .. env0 + n - 1."""
    return _lane_model.hash_actions(a_seed, k, n, nvec, t0, env0, envs)


def busy_actions(a_seed, k, n, t0=0, env0=0):
    """The fixtures' `busy` policy: type and customer_id over 0..2, waiter_id and table_id over 0..9."""
    return hash_actions(a_seed, k, n, t0, env0, nvec=(3, 10, 3, 10))


class _Env:
    def __init__(self, seed):
        self.rng = random.Random(int(seed))
        self.needs_reset = False
        self.ret, self.ep_r, self.ep_l = 0.0, 0.0, 0
        self.clear()

    def clear(self):                                                  # reset :74-93
        self.waiting = []                                             # [tag, wait]
        self.waiters = [[0, 0, 0, None] for _ in range(10)]           # [task, remaining, table, carried customer]
        self.occ, self.dirty = [False] * 10, [False] * 10
        self.guest = [None] * 10                                      # [eating, eating_start, wait]
        self.cooking, self.ready = [], []                             # [tag, table, progress, order_time] / [tag, table, order_time]
        self.t, self.total, self.serial = 0, 0.0, 0
        self.served = self.left = self.cleaned = self.orders = 0
        self.ghosts = self.ghost_wait = 0
        self.needs_reset = False
        self.ret = 0.0

    def step(self, a, max_steps):
        """-> (reward float64, truncated, invalid)"""
        reward = 0.0
        typ, wid, cid, tid = (int(v) for v in a)
        invalid = not (0 <= typ < 4 and 0 <= wid < 10 and 0 <= cid < 50 and 0 <= tid < 10)   # outside the action space: no effect
        if not invalid and self.waiters[wid][0] == 0:                 # :103-166
            w = self.waiters[wid]
            if typ == 0:
                if cid < len(self.waiting):
                    if self.dirty[tid]:
                        reward += -1.5
                    elif not self.occ[tid]:
                        w[:] = [SEAT, DURATION[SEAT], tid, self.waiting.pop(cid)]
            elif typ == 1:
                if self.occ[tid] and not self.guest[tid][0] and any(o[1] == tid for o in self.ready):
                    w[:] = [SERVE, DURATION[SERVE], tid, None]
            elif typ == 2:
                if not self.occ[tid] and self.dirty[tid]:
                    w[:] = [CLEAN, DURATION[CLEAN], tid, None]
        for w in self.waiters:                                        # _update_waiters :285-350
            if w[0]:
                w[1] -= 1
                if w[1] <= 0:
                    task, _, tb, cust = w
                    w[:] = [0, 0, 0, None]
                    if task == SEAT:
                        if not self.occ[tb] and not self.dirty[tb]:
                            self.occ[tb] = True
                            self.guest[tb] = [False, 0, cust[1]]
                            self.cooking.append([self.serial % 100, tb, 0, self.t])
                            self.serial += 1
                            self.total += 2.0
                            self.served += 1
                        else:                                         # the table was taken first: a ghost
                            self.ghosts += 1
                            self.ghost_wait += cust[1]
                    elif task == SERVE:
                        order = next((o for o in self.ready if o[1] == tb), None)
                        if self.occ[tb] and order is not None:
                            self.guest[tb][0], self.guest[tb][1] = True, self.t
                            self.ready.remove(order)
                            self.total += 1.5 + (0.5 if self.t - order[2] <= 5 else 0.0)
                            self.orders += 1
                    elif not self.occ[tb] and self.dirty[tb]:
                        self.dirty[tb] = False
                        self.total += 1.0
                        self.cleaned += 1
        for c in self.waiting:                                        # _update_customers :352-372
            c[1] += 1
        for w in self.waiters:
            if w[0] == SEAT:
                w[3][1] += 1
        self.ghost_wait += self.ghosts
        for tb in range(10):
            if self.occ[tb] and self.guest[tb][0] and self.t - self.guest[tb][1] >= 10:
                self.occ[tb], self.dirty[tb], self.guest[tb] = False, True, None
        for o in self.cooking:                                        # Kitchen.update_cooking
            o[2] += 1
        for o in [o for o in self.cooking if o[2] >= 4]:
            self.cooking.remove(o)
            self.ready.append([o[0], o[1], o[3]])
        p = 0.12 if 1 <= self.t <= 150 else 0.20 if 151 <= self.t <= 350 else 0.08 if 351 <= self.t <= 500 else 0.0   # :374-387
        if self.rng.random() < p:
            self.waiting.append([self.serial % 100, 0])
            self.serial += 1
        for c in [c for c in self.waiting if c[1] >= 20]:             # _handle_impatient_customers :389-405
            self.waiting.remove(c)
            self.total += -5.0
            self.left += 1
        eff = 0.0                                                     # _calculate_efficiency_rewards :407-424
        if not any(self.dirty):
            eff += 0.5
        if not self.waiting:
            eff += 0.3
        if len(self.cooking) <= 2:
            eff += 0.2
        reward += eff
        self.t += 1
        reward += -0.1
        self.total += reward
        return reward, self.t >= max_steps, invalid

    def obs(self):
        o = {k: np.zeros(s, np.int32) for k, s in KEY_SHAPES.items()}
        for j, c in enumerate(self.waiting):
            o["waiting_customers"][j] = c
        for j, w in enumerate(self.waiters):
            o["waiter_status"][j] = [1 if w[0] else 0, w[0], w[1]]
        o["table_occupancy"][:] = self.occ
        o["table_cleanliness"][:] = self.dirty
        for j, c in enumerate(self.cooking):
            o["kitchen_queue"][j] = c[:3]
        for j, c in enumerate(self.ready):
            o["ready_orders"][j] = c[:2]
        o["current_timestep"][0] = self.t
        return o

    def info(self):
        guests = [g for g in self.guest if g is not None]
        carried = [w[3] for w in self.waiters if w[0] == SEAT]
        wsum = sum(c[1] for c in self.waiting) + sum(c[1] for c in carried) + sum(g[2] for g in guests) + self.ghost_wait
        num = len(self.waiting) + len(carried) + len(guests) + self.ghosts
        return [self.t, len(self.waiting), sum(1 for w in self.waiters if not w[0]), len(self.cooking), len(self.ready), sum(self.dirty),
                self.served, self.left, self.cleaned, self.orders, wsum, num]


class RestaurantModel:
    def __init__(self, seeds, max_episode_steps=500, mode=SAME_STEP):
        self.n = len(seeds)
        self.max_steps, self.mode = int(max_episode_steps), mode
        self.envs = [_Env(s) for s in seeds]
        self.invalid = 0

    def reset(self, mask=None):
        for i, e in enumerate(self.envs):
            if mask is None or mask[i]:
                e.clear()
        return self.obs()

    def obs(self):
        per = [e.obs() for e in self.envs]
        return {k: np.stack([o[k] for o in per]) for k in KEYS}

    def info(self):
        """int64 [n, len(INFO)] in the order of INFO."""
        return np.array([e.info() for e in self.envs], np.int64)

    def total_reward(self):
        return np.array([e.total for e in self.envs], np.float64)

    @property
    def needs_reset(self):
        return np.array([e.needs_reset for e in self.envs])

    def episode_stats(self):
        return np.array([e.ep_r for e in self.envs], np.float64), np.array([e.ep_l for e in self.envs], np.int32)

    def step(self, actions):
        """-> (obs, reward float64 [n], terminated, truncated, final_obs); final_obs (SAME_STEP only) is a dict whose rows are
        meaningful where truncated."""
        a = np.asarray(actions, np.int64).reshape(self.n, 4)
        reward, truncated = np.zeros(self.n, np.float64), np.zeros(self.n, bool)
        resetting = [self.mode == NEXT_STEP and e.needs_reset for e in self.envs]
        for i, e in enumerate(self.envs):
            if resetting[i]:
                continue
            reward[i], truncated[i], bad = e.step(a[i], self.max_steps)
            self.invalid += bool(bad)
            e.ret += float(np.float32(reward[i]))                   # episode statistics: the float64 sum of the returned float32 rewards
            if truncated[i]:
                e.ep_r, e.ep_l = e.ret, e.t
        final = None
        if self.mode == SAME_STEP:
            final = self.obs()
            for i in np.flatnonzero(truncated):
                self.envs[i].clear()
        elif self.mode == NEXT_STEP:
            for i, e in enumerate(self.envs):
                if resetting[i]:
                    e.clear()
                elif truncated[i]:
                    e.needs_reset = True
        return self.obs(), reward, np.zeros(self.n, bool), truncated, final
