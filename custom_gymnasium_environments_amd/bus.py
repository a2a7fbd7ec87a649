"""BusVectorEnv — batched drop-in for BusSystemEnv (bus_system_env/environment.py:44-383)."""
import numpy as np
import torch

from . import _native
from ._spaces import Box, Dict, Discrete, MultiBinary, MultiDiscrete
from ._slab import SlabVectorEnv, packed_planes
from .vector_env import TRUNCATED

INFO_FIELDS = {"timestep": 0, "total_delivered": 1, "total_waiting": 2, "total_onboard": 3, "bus_position": 4, "bus_stopped": 5,
               "bus_capacity": 6, "stop_waiting": 7, "needs_reset": 8}
NUM_STOPS, NUM_BUSES, BUS_CAPACITY, MAX_DWELL_TIME = 4, 4, 20, 10                     # config.py:6-11
# the planes of one observation slab, in the order of include/cge_amd.h: key, per-env shape
PLANES = (("bus_stops", (4,)), ("bus_states", (4,)), ("bus_remaining_times", (4,)), ("bus_capacities", (4,)),
          ("bus_passenger_destinations", (4, 4)), ("stop_waiting_counts", (4,)), ("stop_destination_distributions", (4, 4)),
          ("timestep", ()), ("total_delivered", ()), ("total_waiting", ()), ("total_onboard", ()))
OBS_INTS = sum(int(np.prod(s)) for _, s in PLANES)                                     # 56


def make_spaces(max_timesteps=500):
    """(observation_space, action_space) of ONE BusSystemEnv: _create_observation_space (:94-123) and :82."""
    observation = Dict({
        "bus_stops": MultiDiscrete([NUM_STOPS] * NUM_BUSES),
        "bus_states": MultiBinary(NUM_BUSES),
        "bus_remaining_times": Box(0, 50, (NUM_BUSES,), np.int32),
        "bus_capacities": Box(0, BUS_CAPACITY, (NUM_BUSES,), np.int32),
        "bus_passenger_destinations": Box(0, 50, (NUM_BUSES, NUM_STOPS), np.int32),
        "stop_waiting_counts": Box(0, 100, (NUM_STOPS,), np.int32),
        "stop_destination_distributions": Box(0, 50, (NUM_STOPS, NUM_STOPS), np.int32),
        "timestep": Discrete(int(max_timesteps)),
        "total_delivered": Discrete(1000),
        "total_waiting": Discrete(1000),
        "total_onboard": Discrete(1000),
    })
    return observation, MultiDiscrete([MAX_DWELL_TIME + 1] * NUM_BUSES)


class BusVectorEnv(SlabVectorEnv):
    """N independent BusSystemEnv instances (4 buses on a ring of 4 stops, 50..150 passengers per episode, 500 steps) stepped by one
    HIP kernel launch.  Spaces as the reference: `MultiDiscrete([11] * 4)` actions (the dwell time each bus takes when it next
    arrives at a stop, :82) and the `Dict` observation of :94-123 with its eleven keys and bounds.  Bit-exact with the reference.

    Observations are dicts of int32 device tensors, one per key, in gymnasium's batched-Dict layout ([N, 4], [N, 4, 4] or [N]); all
    are views of ONE slab the kernel writes key by key (`obs_slab(obs)` gives it back).  The reference's `bus_states` is int8 and
    its four scalars are Python ints; here everything is int32.  `terminated` is never set (:156); `truncated`
    after `max_timesteps` steps.

    The reference never seeds `random` (reset(seed) reaches np_random only, :127) while generate_passengers (utils.py:22-46) draws
    from it, so env i owns the stream `random.seed(seed + env_index0 + i)`, as ParkingVectorEnv and SnakeVectorEnv do.  A new batch
    holds empty stops until its first reset().

    rollout(k): k fused step()s in one launch (the record stays in registers).  actions: None -> counter-hash dwell times
    (cge_hash_action(action_seed, env_index0 + i, t0 + t, 11, bus)) or int32 [k, N, 4].  Returns (obs, reward_sum, done_count)
    with obs a dict of views [k, N, ...] if trajectory else the last step's [N, ...]; with per_step=True
    (obs, reward[k, N], truncated[k, N], reward_sum, done_count) — the outputs of k step() calls (a SAME_STEP trajectory holds
    the reset observation at a truncated step, as step()'s `obs` does; the terminal observations of a fused rollout go to a side output
    once `collect_final_obs()` has registered one: `final_obs()` returns them as a dict of per-key tensors [m, ...] with their steps and
    envs, `final_obs_dropped()` what did not fit; segments of 64 envs)."""

    _abi = "cge_bus"
    INFO_FIELDS = INFO_FIELDS
    _action_shape = (NUM_BUSES,)
    _flags = TRUNCATED
    _info_dtype, _info_indexed = torch.int32, True
    # an env-step refused for a dwell time outside 0..10 (reference: ValueError, :160-161)
    _invalid_action_text = f"Invalid action in {{n}} env-step(s): must be {NUM_BUSES} integers 0-{MAX_DWELL_TIME}"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_timesteps=500, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.max_timesteps = int(max_timesteps)
        self.single_observation_space, self.single_action_space = make_spaces(self.max_timesteps)
        self._init_slab(*packed_planes(PLANES, self.num_envs), torch.int32)   # int32 [56 * N] per step
        self._create(_native.BusConfig(self.max_timesteps, self._mode_code), info_fields, record_episode_statistics, reference_info)

    def _rows_layout(self, num_rows):
        return packed_planes(PLANES, num_rows)

    # ------------------------------------------------------------------ extras
    def reference_info(self):
        """The reference's `info` dict under ITS keys (_get_info, :339-350), one int32 tensor per key: [N] for the four counters,
        [N, 4] for the per-bus / per-stop lists; `bus_states` is 1 for "stopped" and 0 for "traveling".  `reference_info=True` in
        the constructor merges it into every step's / reset's infos (twenty small kernels per call: not for the hot loop)."""
        def per(f):
            return torch.stack([self.info(f, j) for j in range(4)], 1)

        return {"timestep": self.info("timestep"), "total_delivered": self.info("total_delivered"),
                "total_waiting": self.info("total_waiting"), "total_onboard": self.info("total_onboard"),
                "bus_positions": per("bus_position"), "bus_states": per("bus_stopped"), "bus_capacities": per("bus_capacity"),
                "stop_waiting": per("stop_waiting")}
