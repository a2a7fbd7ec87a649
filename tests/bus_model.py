"""Counts-only model of the reference's BusSystemEnv (bus_system_env/environment.py, utils.py) in plain Python / NumPy.

A passenger is only its destination and waits at its source, so the reference's passenger lists reduce to 16 waiting counts
[stop, destination] and 16 onboard counts [bus, destination]; `_calculate_boarding_priority` (:278-294) depends only on
(destination - stop) mod 4 (next stop 0, previous stop 1, opposite stop 2), so its stable sort + pop(0) until full boards
min(free seats, count) for destinations c+1, then c+3, then c+2.  tests/test_bus_cpu.py pins the model to fixtures recorded from the
unmodified reference; the GPU tests then use it where the fixtures cannot reach (large batches, other autoreset modes).  Test
infrastructure only: the product never imports it.

Env i draws its passengers from `random.Random(seeds[i])`, the stream `random.seed(seeds[i])` gives the reference when it runs alone.
"""
import random

import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP  # noqa: F401

NUM_STOPS, NUM_BUSES, BUS_CAPACITY, MAX_PASSENGERS, MAX_TIMESTEPS, MAX_DWELL_TIME, TRAVEL = 4, 4, 20, 150, 500, 10, 5
KEYS = ("bus_stops", "bus_states", "bus_remaining_times", "bus_capacities", "bus_passenger_destinations", "stop_waiting_counts",
        "stop_destination_distributions", "timestep", "total_delivered", "total_waiting", "total_onboard")
KEY_SHAPES = {"bus_stops": (4,), "bus_states": (4,), "bus_remaining_times": (4,), "bus_capacities": (4,), "bus_passenger_destinations": (4, 4),
              "stop_waiting_counts": (4,), "stop_destination_distributions": (4, 4), "timestep": (), "total_delivered": (), "total_waiting": (),
              "total_onboard": ()}


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None):
    """int32 [k, n, 4]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for — bus j of env i at step t takes
    hash_action(a_seed, env0 + i, t0 + t, 11, j).  envs: global env indices instead of env0 .. env0 + n - 1."""
    return _lane_model.hash_actions(a_seed, k, n, (MAX_DWELL_TIME + 1,) * NUM_BUSES, t0, env0, envs)


class BusModel:
    def __init__(self, seeds, max_timesteps=MAX_TIMESTEPS, mode=SAME_STEP):
        self.n = n = len(seeds)
        self.max_timesteps, self.mode = int(max_timesteps), mode
        self.rng = [random.Random(int(s)) for s in seeds]
        self.wait = np.zeros((n, NUM_STOPS, NUM_STOPS), np.int64)
        self.onb = np.zeros((n, NUM_BUSES, NUM_STOPS), np.int64)
        self.stop = np.tile(np.arange(NUM_BUSES) % NUM_STOPS, (n, 1)).astype(np.int64)
        self.stopped = np.ones((n, NUM_BUSES), np.int64)
        self.rem = np.zeros((n, NUM_BUSES), np.int64)
        self.t = np.zeros(n, np.int64)
        self.delivered = np.zeros(n, np.int64)
        self.needs_reset = np.zeros(n, bool)
        self.ret = np.zeros(n, np.float64)          # the running episode's return
        self.ep_r = np.zeros(n, np.float64)         # return / length of the last finished episode
        self.ep_l = np.zeros(n, np.int32)
        self.invalid = 0

    # ------------------------------------------------------------------ reset :125-151 + generate_passengers utils.py:22-46
    def _reset_env(self, i):
        r = self.rng[i]
        w = np.zeros((NUM_STOPS, NUM_STOPS), np.int64)
        for _ in range(r.randint(50, MAX_PASSENGERS)):
            source = r.randint(0, NUM_STOPS - 1)
            destination = r.randint(0, NUM_STOPS - 1)
            while destination == source:
                destination = r.randint(0, NUM_STOPS - 1)
            w[source, destination] += 1
        self.wait[i] = w
        self.onb[i] = 0
        self.stop[i] = np.arange(NUM_BUSES) % NUM_STOPS
        self.stopped[i] = 1
        self.rem[i] = 0
        self.t[i] = 0
        self.delivered[i] = 0
        self.needs_reset[i] = False
        self.ret[i] = 0.0

    def reset(self, mask=None):
        for i in range(self.n):
            if mask is None or mask[i]:
                self._reset_env(i)
        return self.obs()

    # ------------------------------------------------------------------ _get_observation :301-337
    def obs(self, rows=None):
        s = slice(None) if rows is None else rows
        i32 = np.int32
        return {
            "bus_stops": self.stop[s].astype(i32), "bus_states": self.stopped[s].astype(i32), "bus_remaining_times": self.rem[s].astype(i32),
            "bus_capacities": (BUS_CAPACITY - self.onb[s].sum(-1)).astype(i32), "bus_passenger_destinations": self.onb[s].astype(i32),
            "stop_waiting_counts": self.wait[s].sum(-1).astype(i32), "stop_destination_distributions": self.wait[s].astype(i32),
            "timestep": self.t[s].astype(i32), "total_delivered": self.delivered[s].astype(i32),
            "total_waiting": self.wait[s].sum((-1, -2)).astype(i32), "total_onboard": self.onb[s].sum((-1, -2)).astype(i32),
        }

    # ------------------------------------------------------------------ step :153-186
    def step(self, actions):
        """-> (obs, reward float64 [n], terminated, truncated, final_obs); final_obs (SAME_STEP only) is a dict whose rows are
        meaningful where truncated."""
        a = np.asarray(actions, np.int64).reshape(self.n, NUM_BUSES)
        idx = np.arange(self.n)
        resetting = self.needs_reset.copy() if self.mode == NEXT_STEP else np.zeros(self.n, bool)
        valid = ((a >= 0) & (a <= MAX_DWELL_TIME)).all(1)            # else the reference raises ValueError (:160-161): env untouched
        act = valid & ~resetting
        self.invalid += int((~valid & ~resetting).sum())
        saved = [x.copy() for x in (self.wait, self.onb, self.stop, self.stopped, self.rem, self.t, self.delivered)]
        r2 = np.zeros(self.n, np.int64)
        every3 = self.t % 3 == 0                                      # current_timestep before the increment (:223)
        for b in range(NUM_BUSES):                                    # _update_buses :188-237
            rem, st, sp = self.rem[:, b].copy(), self.stop[:, b].copy(), self.stopped[:, b].copy()
            load = self.onb[:, b].sum(1)
            dec = rem > 0
            rem = rem - dec
            hit = dec & (rem == 0)
            depart, arrive = hit & (sp == 1), hit & (sp == 0)
            sp = np.where(depart, 0, np.where(arrive, 1, sp))
            st = np.where(depart, (st + 1) % NUM_STOPS, st)
            rem = np.where(depart, TRAVEL, rem)
            rem = np.where(arrive & (a[:, b] > 0), a[:, b], rem)
            nobody = self.wait[idx, st].sum(1) == 0
            leave = (sp == 1) & (rem == 0) & ((load >= BUS_CAPACITY) | nobody | every3)
            sp = np.where(leave, 0, sp)
            st = np.where(leave, (st + 1) % NUM_STOPS, st)
            rem = np.where(leave, TRAVEL, rem)
            r2 -= load
            self.rem[:, b], self.stop[:, b], self.stopped[:, b] = rem, st, sp
        for b in range(NUM_BUSES):                                    # _process_passenger_movements :239-276
            m = self.stopped[:, b] == 1
            c = self.stop[:, b]
            al = self.onb[idx, b, c] * m
            r2 += 10 * al
            self.delivered += al
            self.onb[idx, b, c] -= al
            load = self.onb[:, b].sum(1)
            for off in (1, 3, 2):
                d = (c + off) % NUM_STOPS
                mv = np.minimum(self.wait[idx, c, d], BUS_CAPACITY - load) * m
                self.wait[idx, c, d] -= mv
                self.onb[idx, b, d] += mv
                load = load + mv
        self.t += 1
        for cur, old in zip((self.wait, self.onb, self.stop, self.stopped, self.rem, self.t, self.delivered), saved):
            cur[~act] = old[~act]
        reward = np.where(act, 0.5 * r2, 0.0)
        truncated = act & (self.t >= self.max_timesteps)
        self.ret += reward
        self.ep_r[truncated] = self.ret[truncated]
        self.ep_l[truncated] = self.t[truncated]
        final = None
        if self.mode == SAME_STEP:
            final = self.obs()
            for i in np.flatnonzero(truncated):
                self._reset_env(i)
        elif self.mode == NEXT_STEP:
            for i in np.flatnonzero(resetting):
                self._reset_env(i)
            self.needs_reset |= truncated
        return self.obs(), reward, np.zeros(self.n, bool), truncated, final
