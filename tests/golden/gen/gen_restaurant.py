"""Golden vectors for RestaurantEnv, produced by running the reference's own restaurant_env_updated/restaurant_env.py and entities.py
(unmodified, imported from the reference checkout under the stub gymnasium).  Run it in a process of its own: the reference's module
names `entities` and `utils` are generic.

Protocol: the env draws one `random.random()` per step from the global `random` and never seeds it, so env i is a fresh RestaurantEnv
run alone after `random.seed(seed0 + i)`; on `truncated` the terminal observation is recorded and `env.reset()` continues the same
stream (auto-reset).  `max_episode_steps` is the attribute the reference's inference.py:14-17 sets after construction.

The id columns: the reference shows `hash(str(uuid.uuid4())) % 100`, OS randomness through a salted hash.  Here `uuid.uuid4` is replaced
(the reference's files are not edited) by a factory whose `__str__` returns a `str` subclass that hashes to a serial number; the serial
restarts at 0 before every `reset()`.  Customers take one at arrival, orders one in Kitchen.add_order, so the columns hold
`serial % 100` — the convention RestaurantVectorEnv writes.

Policies: "hash" = the counter hash over the four components (4, 10, 50, 10); "busy" = type hashed over 0..2, customer_id over 0..2,
waiter_id and table_id over 0..9 — the one under which customers are seated, served and tables cleaned.
Outputs: tests/golden/restaurant_hash.npz, restaurant_busy.npz, restaurant_short.npz (time limit 9), restaurant_short40.npz (time
limit 40), restaurant_long.npz (time limit 1000).
"""
import json
import os
import random
import uuid

import numpy as np

import common

common.use_stubs()
common.add_reference_dir("restaurant_env_updated")
from restaurant_env import RestaurantEnv  # noqa: E402  (reference code)
from entities import CustomerState, TaskType  # noqa: E402

KEYS = ("waiting_customers", "waiter_status", "table_occupancy", "table_cleanliness", "kitchen_queue", "ready_orders", "current_timestep")
INFO = ("current_timestep", "waiting_customers", "idle_waiters", "kitchen_queue_length", "ready_orders", "dirty_tables", "customers_served",
        "customers_left", "tables_cleaned", "orders_served", "wait_time_sum", "num_customers")
EVENTS = ("seat_completed", "serve_with_bonus", "serve_without_bonus", "clean_completed", "customer_left", "dirty_table_penalty",
          "waiter_busy_refused", "ghost_seating", "serve_to_served_table", "reward_minus_0_1")
NVEC = (4, 10, 50, 10)


class _Id(str):
    """A string that hashes to its serial number."""
    def __new__(cls, serial):
        s = super().__new__(cls, f"id-{serial}")
        s.serial = serial
        return s

    def __hash__(self):
        return self.serial

    def __eq__(self, other):
        return str.__eq__(self, other)


class _Uuid:
    def __init__(self, serial):
        self.serial = serial

    def __str__(self):
        return _Id(self.serial)


class Serial:
    n = 0

    @classmethod
    def uuid4(cls):
        cls.n += 1
        return _Uuid(cls.n - 1)


uuid.uuid4 = Serial.uuid4


def action(policy, a_seed, i, t):
    n = (3, 10, 3, 10) if policy == "busy" else NVEC
    return [common.hash_action(a_seed, i, t, n[c], c) for c in range(4)]


def info_row(env, info):
    st = info["episode_stats"]
    assert st["total_wait_time"] == 0 and st["average_wait_time"] == 0.0          # the reference never updates the two
    wsum = sum(c.wait_time for c in env.customers.values())
    assert info["average_wait_time"] == wsum / max(len(env.customers), 1)
    return [info["current_timestep"], info["waiting_customers"], info["idle_waiters"], info["kitchen_queue_length"], info["ready_orders"],
            info["dirty_tables"], st["customers_served"], st["customers_left"], st["tables_cleaned"], st["orders_served"], wsum, len(env.customers)]


def run_env(seed, T, a_seed, i, policy, max_steps, events):
    random.seed(seed)
    env = RestaurantEnv()
    env.max_episode_steps = max_steps
    Serial.n = 0
    obs, info = env.reset()
    out = dict(obs0=obs, A=np.zeros((T, 4), np.int32), R=np.zeros(T, np.float64), TR=np.zeros(T, np.uint8), I=np.zeros((T, len(INFO)), np.int32),
               W=np.zeros(T, np.float64), TOT=np.zeros(T, np.float64), O={k: [] for k in KEYS}, resets=[], info_keys=list(info), stat_keys=list(info["episode_stats"]))
    for t in range(T):
        a = action(policy, a_seed, i, t)
        # what is about to happen, read from the reference's own objects
        seats_due = sum(1 for w in env.waiters if w.task_type == TaskType.SEAT_CUSTOMER and w.task_remaining_time == 1)
        tb = env.tables[a[3]]
        eating = tb.occupied and env.customers[tb.customer_id].state == CustomerState.EATING
        before = dict(env.episode_stats)
        tot = env.total_reward
        obs, rew, term, trunc, info = env.step(dict(type=a[0], waiter_id=a[1], customer_id=a[2], table_id=a[3]))
        assert not term
        st = env.episode_stats
        d = {k: st[k] - before[k] for k in ("customers_served", "customers_left", "tables_cleaned", "orders_served")}
        result = env.last_action_details[0]["result"]
        events["seat_completed"] += d["customers_served"]
        events["clean_completed"] += d["tables_cleaned"]
        events["customer_left"] += d["customers_left"]
        events["ghost_seating"] += seats_due - d["customers_served"]
        if d["orders_served"]:
            assert d["orders_served"] == 1
            part = (env.total_reward - tot) - rew - 2.0 * d["customers_served"] - 1.0 * d["tables_cleaned"] + 5.0 * d["customers_left"]
            assert abs(part - 2.0) < 1e-9 or abs(part - 1.5) < 1e-9, part
            events["serve_with_bonus" if part > 1.75 else "serve_without_bonus"] += 1
        events["dirty_table_penalty"] += result == "table_dirty"
        events["waiter_busy_refused"] += result == "waiter_not_idle"
        events["serve_to_served_table"] += a[0] == 1 and result == "invalid_serve" and bool(eating)
        events["reward_minus_0_1"] += rew == -0.1
        out["A"][t] = a; out["R"][t] = rew; out["TR"][t] = trunc
        out["I"][t] = info_row(env, info); out["W"][t] = info["average_wait_time"]; out["TOT"][t] = info["total_reward"]
        for k in KEYS:
            out["O"][k].append(np.asarray(obs[k]))
        if trunc:
            Serial.n = 0
            obs, _ = env.reset()
            out["resets"].append((t, obs))
    return env, out


def space_record(env):
    """keys, shapes, dtypes and bounds of the reference's spaces (settings only)."""
    def rec(sp):
        kind = type(sp).__name__
        d = dict(kind=kind, shape=list(sp.shape), dtype=str(sp.dtype))
        if kind == "Box":
            d.update(low=float(sp.low.min()), high=float(sp.high.max()))
        elif kind == "Discrete":
            d.update(n=int(sp.n))
        return d
    return dict(observation={k: rec(s) for k, s in env.observation_space.spaces.items()}, action={k: rec(s) for k, s in env.action_space.spaces.items()})


def make(name, n_envs, T, seed0, a_seed, policy, max_steps=500, need_events=False):
    events = dict.fromkeys(EVENTS, 0)
    rows = [run_env(seed0 + i, T, a_seed, i, policy, max_steps, events) for i in range(n_envs)]
    env = rows[0][0]
    rows = [r[1] for r in rows]
    if need_events:
        missing = [k for k, v in events.items() if v < 1]
        assert not missing, f"{name}: the recorded steps hold no {missing}; change seeds or add envs"
    ridx = [(i, t) for i, r in enumerate(rows) for t, _ in r["resets"]]
    arrays = dict(seed0=np.int64(seed0), a_seed=np.int64(a_seed), policy=np.array(policy), max_episode_steps=np.int64(max_steps),
                  actions=np.stack([r["A"] for r in rows]).astype(np.int8), reward=np.stack([r["R"] for r in rows]),
                  truncated=np.stack([r["TR"] for r in rows]), info=np.stack([r["I"] for r in rows]), info_fields=np.array(json.dumps(INFO)),
                  average_wait_time=np.stack([r["W"] for r in rows]), total_reward=np.stack([r["TOT"] for r in rows]),
                  reset_index=np.array(ridx, np.int32).reshape(-1, 2), spaces=np.array(json.dumps(space_record(env))),
                  info_keys=np.array(json.dumps(rows[0]["info_keys"])), stat_keys=np.array(json.dumps(rows[0]["stat_keys"])),
                  events=np.array(json.dumps(events)), versions=np.array(json.dumps(common.versions())))
    for k in KEYS:      # every value is at most 1000 (the timestep): int16 keeps the files small
        arrays["obs0_" + k] = np.stack([np.asarray(r["obs0"][k]) for r in rows]).astype(np.int16)
        arrays["obs_" + k] = np.stack([np.stack(r["O"][k]) for r in rows]).astype(np.int16)
        shape = arrays["obs0_" + k].shape[1:]
        arrays["reset_" + k] = np.array([np.asarray(ob[k]) for r in rows for _, ob in r["resets"]], np.int16).reshape((-1,) + shape)
    out = os.path.join(common.GOLDEN, name + ".npz")
    np.savez_compressed(out, **arrays)
    print(name, "episodes", len(ridx), "sum reward", arrays["reward"].sum(), "events", events, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 614 * 1024, "larger than the largest fixture already committed: cut envs"


if __name__ == "__main__":
    make("restaurant_hash", 6, 1100, seed0=1300, a_seed=123, policy="hash")
    make("restaurant_busy", 12, 1100, seed0=1350, a_seed=31, policy="busy", need_events=True)
    make("restaurant_short", 4, 1100, seed0=1380, a_seed=77, policy="busy", max_steps=9)
    make("restaurant_short40", 4, 1100, seed0=1390, a_seed=78, policy="busy", max_steps=40)
    make("restaurant_long", 3, 1010, seed0=1395, a_seed=79, policy="busy", max_steps=1000)
