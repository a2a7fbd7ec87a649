"""AirlineVectorEnv — batched drop-in for AirlineOperationsEnv (airline_operations_env/airline_env.py:123-686)."""
import numpy as np

from . import _native
from ._spaces import Box, Discrete
from .vector_env import DeviceVectorEnv

INFO_FIELDS = {"on_time_performance": 0, "passenger_satisfaction": 1, "daily_revenue": 2, "daily_costs": 3, "current_hour": 4, "timestep": 5,
               "needs_reset": 6, "flights_in_air": 7, "delay_compensation": 8, "fuel_costs": 9}
REFERENCE_INFO_KEYS = ("on_time_performance", "passenger_satisfaction", "daily_revenue", "daily_costs", "current_hour")   # :435-441, in its order
OBS_DIM, NUM_ACTIONS = 160, 45
RECORD_BYTES, GENERATOR_BYTES = 1656, 2560                                             # device bytes per env; + 8 per batch (the error counter)


class AirlineVectorEnv(DeviceVectorEnv):
    """N independent AirlineOperationsEnv instances (25 aircraft, 15 airports, 150 flights, 40 crew sets, up to 3 weather systems; a
    step is a quarter of an hour from 6.0) stepped by one HIP kernel launch.  Spaces as the reference: `Discrete(45)` actions (:144)
    and a `Box(-inf, inf, (160,), float32)` observation (:148-150).

    Bit-exact with the reference — observations, the integer-valued reward (its float64 value, rounded to float32 on output), flags
    and the float64 info values — with one stated departure: a weather system's distance to an airport is sqrt(dx*dx + dy*dy) where
    the reference evaluates `dx**2` through libm pow, which differs in the last float64 place in 0.07 % of its evaluations; the value is
    seen only through the float32 `weather_severity` and the `dist < radius` test, and no recorded observation differs.

    The reference's quirks are kept, each is observable: `daily_revenue` is 0.0 for ever (passengers_onboard is zeroed before it is
    paid), crews only rest, "the ten priority flights" are flights 0..9, a boarding aircraft can be taken by a second flight, a flight
    delayed by `scheduled + 0.25` counts as on time where float64 rounding makes the difference smaller than 0.25, `daily_costs`
    re-adds the cumulative delay compensation every step, aircraft keep their airport across episodes.

    `terminated` when the clock reaches 23.75 (71 steps) or passenger_satisfaction falls below 0.6; `truncated` never.  In Disabled
    mode the reference may be stepped on past termination (the hour wraps at 24, maintenance events and the fuel floor appear); so may
    this.  In SameStep mode `infos["final_obs"]` is valid where `terminated`; its other rows are unspecified.

    Streams: the reference draws from the process-global `random` and never seeds it, so env i owns the stream
    `random.seed(seed + env_index0 + i)`.  The NETWORK — aircraft bases, the 150-flight schedule, crews — is drawn once by the
    reference's constructor, which also calls reset() itself, and survives every reset().  `reset(seed=s)` is therefore
    `random.seed(s_i); env = AirlineOperationsEnv(); env.reset(seed=s_i)`: a new network, the constructor's discarded reset, then the
    visible one.  A reset() without a seed, `reset_mask` and every autoreset continue the stream and keep the network.  A new batch
    is seeded with 0.

    Actions: int32 [N].  An action below 0 or above 44 skips `_process_action`; the rest of the step runs, and
    `invalid_action_count()` counts it (the reference would index its aircraft list from the back for -25..-1 and do nothing for any
    other value).

    rollout(k): k fused step()s in one launch.  actions: None -> counter-hash actions cge_hash_action(action_seed, env_index0 + i,
    t0 + t, 45, 0), or int32 [k, N].  Returns (obs, reward_sum, done_count) with obs [k, N, 160] if trajectory else the last step's
    [N, 160]; with per_step=True (obs, reward[k, N], terminated[k, N], reward_sum, done_count).  A SAME_STEP trajectory holds the reset
    observation at a terminated step, as step()'s `obs` does; the terminal rows of a fused rollout are not delivered.

    Not built: a registry id, rendering, terminal rows of fused SameStep rollouts, a bench workload, canonical get_state / set_state
    records (`snapshot()` / `restore()` checkpoint the whole batch)."""

    _abi = "cge_airline"
    INFO_FIELDS = INFO_FIELDS
    _invalid_action_text = "Invalid action in {n} env-step(s): must be an integer 0-44"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, reuse_buffers=False, info_fields=(),
                 record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.single_action_space = Discrete(NUM_ACTIONS)
        self.single_observation_space = Box(-np.inf, np.inf, (OBS_DIM,), np.float32)
        self._obs_shape = (self.num_envs, OBS_DIM)
        self._create(_native.AirlineConfig(self._mode_code, 0), info_fields, record_episode_statistics, reference_info)

    def reference_info(self):
        """The reference's `info` dict (:435-441): its five keys in its order, one float64 tensor [N] per key."""
        return {key: self.info(key) for key in REFERENCE_INFO_KEYS}
