"""RestaurantVectorEnv — batched drop-in for RestaurantEnv (restaurant_env_updated/restaurant_env.py:11-494, entities.py)."""
from collections.abc import Mapping

import numpy as np
import torch

from . import _native
from ._spaces import Box, Dict, Discrete
from ._slab import SlabVectorEnv, packed_planes
from .vector_env import TRUNCATED

INFO_FIELDS = {"timestep": 0, "waiting_customers": 1, "idle_waiters": 2, "kitchen_queue_length": 3, "ready_orders": 4, "dirty_tables": 5,
               "customers_served": 6, "customers_left": 7, "tables_cleaned": 8, "orders_served": 9, "wait_time_sum": 10, "num_customers": 11,
               "total_reward": 12, "needs_reset": 13}
NUM_TABLES, NUM_WAITERS = 10, 10                                                       # :19-20
# the planes of one observation slab, in the order of include/cge_amd.h (the reference's key order, :47-55): key, per-env shape, high
PLANES = (("waiting_customers", (50, 2)), ("waiter_status", (10, 3)), ("table_occupancy", (10,)), ("table_cleanliness", (10,)),
          ("kitchen_queue", (50, 3)), ("ready_orders", (20, 2)), ("current_timestep", (1,)))
_HIGH = {"waiting_customers": 100, "waiter_status": 10, "table_occupancy": 1, "table_cleanliness": 1, "kitchen_queue": 100, "ready_orders": 100,
         "current_timestep": 500}
OBS_INTS = sum(int(np.prod(s)) for _, s in PLANES)                                     # 341
# the columns of a packed action, in the reference's key order (:41-46), and their bounds
ACTION_KEYS = ("type", "waiter_id", "customer_id", "table_id")
ACTION_NVEC = (4, NUM_WAITERS, 50, NUM_TABLES)
MAX_EPISODE_STEPS = 1000                                                               # the reference's own inference.py:14-17 runs 1000


def make_spaces():
    """(observation_space, action_space) of ONE RestaurantEnv (:41-55).  `current_timestep` keeps the reference's declared bound of
    500 whatever max_episode_steps is — the reference declares 500 and runs 1000 too."""
    observation = Dict({k: Box(0, _HIGH[k], shape, np.int32) for k, shape in PLANES})
    return observation, Dict({k: Discrete(n) for k, n in zip(ACTION_KEYS, ACTION_NVEC)})


class RestaurantVectorEnv(SlabVectorEnv):
    """N independent RestaurantEnv instances (10 tables, 10 waiters, a waiting line and a kitchen, 500 steps) stepped by one HIP
    kernel launch.  Spaces as the reference: the `Dict` action {type: Discrete(4), waiter_id: Discrete(10), customer_id: Discrete(50),
    table_id: Discrete(10)} (:41-46) and the `Dict` observation of :47-55 with its seven int32 keys.

    Bit-exact with the reference (the reward is its float64 sum, rounded to float32 on output) EXCEPT the three id columns
    `waiting_customers[:, 0]`, `kitchen_queue[:, 0]` and `ready_orders[:, 0]`: the reference shows `hash(str(uuid.uuid4())) % 100` —
    OS randomness through a per-process salted hash, which nothing can reproduce and no agent can use.  Here each env keeps one
    counter, restarted at 0 by every episode reset; every `uuid.uuid4()` call of the reference (a customer's at arrival, an order's in
    Kitchen.add_order) takes its value and increments it, and the column holds that serial number mod 100.

    Actions: step() takes the packed int32 tensor [N, 4] with columns (type, waiter_id, customer_id, table_id) as it is — the form
    for graph capture — or a mapping of four integer tensors / arrays [N] under the reference's keys (what `action_space.sample()` and
    `action_sampler()` give), stacked into the packed form by one extra launch; rollout() the same with a leading [k].  An action
    outside the action space — a component negative or not below its bound (4, 10, 50, 10) — has no effect, like the reference's
    "invalid_waiter" / "invalid_seat" / "unknown_action" results (the reference would index from the end with a negative value and
    ignore a customer_id of 50 or more on a serve or clean action); the step itself runs, and `invalid_action_count()` counts them.

    Observations are dicts of int32 device tensors, one per key, in gymnasium's batched-Dict layout ([N, 50, 2], [N, 10], ...); all
    are views of ONE slab the kernel writes key by key (`obs_slab(obs)` gives it back).  `terminated` is never set (:100);
    `truncated` after `max_episode_steps` steps (1..1000; the reference sets 500 and its inference script 1000).  The timestep
    saturates at 65,535, which only a Disabled-mode batch that is never reset can reach (it stays truncated).  In SameStep mode
    `infos["final_obs"]` is valid where `truncated`; its other rows are unspecified.

    The reference draws one `random.random()` per step from the process-global `random` and never seeds it, so env i owns the stream
    `random.seed(seed + env_index0 + i)`, as BusVectorEnv, ParkingVectorEnv and SnakeVectorEnv do; reset() draws nothing and an
    auto-reset continues the stream.

    rollout(k): k fused step()s in one launch (the record stays in registers).  actions: None -> counter-hash actions (column c is
    cge_hash_action(action_seed, env_index0 + i, t0 + t, (4, 10, 50, 10)[c], c)), the packed int32 [k, N, 4] or the mapping form.
    Returns (obs, reward_sum, done_count) with obs a dict of views [k, N, ...] if trajectory else the last step's [N, ...]; with
    per_step=True (obs, reward[k, N], truncated[k, N], reward_sum, done_count) — the outputs of k step() calls (a SAME_STEP trajectory
    holds the reset observation at a truncated step, as step()'s `obs` does; the terminal observations of a fused rollout go to a side
    output once `collect_final_obs()` has registered one: `final_obs()` returns them as a dict of per-key tensors [m, ...] with their
    steps and envs, `final_obs_dropped()` what did not fit; segments of 64 envs)."""

    _abi = "cge_restaurant"
    INFO_FIELDS = INFO_FIELDS
    _action_shape = (4,)
    _flags = TRUNCATED
    # an env-step whose action had a component that was negative or not below its bound (it had no effect; the step itself ran)
    _invalid_action_text = f"Invalid action in {{n}} env-step(s): (type, waiter_id, customer_id, table_id) must lie below {ACTION_NVEC}"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_episode_steps=500, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.max_episode_steps = int(max_episode_steps)
        self.single_observation_space, self.single_action_space = make_spaces()
        self._init_slab(*packed_planes(PLANES, self.num_envs), torch.int32)   # int32 [341 * N] per step
        self._create(_native.RestaurantConfig(self.max_episode_steps, self._mode_code), info_fields, record_episode_statistics, reference_info)

    def _create_error(self, status):
        if status == -1 and not 1 <= self.max_episode_steps <= MAX_EPISODE_STEPS:
            return ValueError(f"max_episode_steps must be in 1..{MAX_EPISODE_STEPS}, got {self.max_episode_steps}")
        return None

    def _rows_layout(self, num_rows):
        return packed_planes(PLANES, num_rows)

    # ------------------------------------------------------------------ actions
    def _device_actions(self, actions, k=None):
        """The packed int32 [N, 4] ([k, N, 4]) as it is, or the Dict form stacked into it."""
        shape = self._actions_shape if k is None else (k,) + self._actions_shape
        if isinstance(actions, Mapping):
            if set(actions) != set(ACTION_KEYS):
                raise ValueError(f"a Dict action has the keys {ACTION_KEYS}, got {sorted(actions)}")
            cols = [self._as_device(actions[key], torch.int32, shape[:-1], f"actions[{key!r}]") for key in ACTION_KEYS]
            return (torch.stack(cols, -1),)
        t = self._as_device(actions, torch.int32, shape, "actions")
        if t.data_ptr() % 16:                                   # the kernel loads an env's four components as one 16-byte piece
            raise ValueError("packed actions must start at a 16-byte boundary (a view at an odd offset of its storage: clone it)")
        return (t,)

    def action_sampler(self, seed=None, dtype=None):
        """A DeviceSpaceSampler over the batched Dict action space; its samples are int32, the form step() stacks with no conversion."""
        return super().action_sampler(seed, {key: torch.int32 for key in ACTION_KEYS} if dtype is None else dtype)

    # ------------------------------------------------------------------ extras
    def reference_info(self):
        """The reference's `info` dict under ITS keys (_get_info, :478-494), one float64 tensor [N] per value; `episode_stats` is the
        nested dict of :84-91, whose `total_wait_time` and `average_wait_time` the reference never updates (zeros).
        `average_wait_time` = wait_time_sum / max(num_customers, 1) in float64.  `reference_info=True` in the constructor merges it
        into every step's / reset's infos (a dozen small kernels per call: not for the hot loop)."""
        zero = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
        return {"total_reward": self.info("total_reward"), "current_timestep": self.info("timestep"),
                "waiting_customers": self.info("waiting_customers"), "idle_waiters": self.info("idle_waiters"),
                "kitchen_queue_length": self.info("kitchen_queue_length"), "ready_orders": self.info("ready_orders"),
                "dirty_tables": self.info("dirty_tables"),
                "episode_stats": {"customers_served": self.info("customers_served"), "customers_left": self.info("customers_left"),
                                  "tables_cleaned": self.info("tables_cleaned"), "orders_served": self.info("orders_served"),
                                  "total_wait_time": zero, "average_wait_time": zero.clone()},
                "average_wait_time": self.info("wait_time_sum") / self.info("num_customers").clamp(min=1.0)}
