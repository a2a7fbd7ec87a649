"""SpaceStationVectorEnv — batched drop-in for SpaceStationEnv (space_station_env/station_env.py:46-797)."""
import numpy as np

from . import _native
from ._spaces import Box, Discrete
from .vector_env import TERMINATED_AT_LIMIT, DeviceVectorEnv

INFO_FIELDS = {"time_step": 0, "day": 1, "crew_alive": 2, "system_failures": 3, "emergency_count": 4, "mission_success": 5, "episode_reward": 6,
               "battery_level": 7, "avg_crew_health": 8, "system_failure_mask": 9, "needs_reset": 10, "crew_casualties": 11, "evacuated": 12}
REFERENCE_INFO_KEYS = ("time_step", "day", "crew_alive", "system_failures", "emergency_count", "mission_success", "episode_reward", "battery_level",
                       "avg_crew_health")                                               # :787-797, in its order
SYSTEMS = ("Oxygen Generation", "CO2 Scrubbing", "Water Recycling", "Power Grid", "Thermal Control", "Atmospheric Pressure", "Nitrogen Supply",
           "Waste Processing", "Fire Suppression", "Radiation Shielding", "Communications", "Artificial Gravity")   # bit s of `system_failure_mask`
OBS_DIM, DECLARED_OBS_DIM, NUM_ACTIONS, MAX_STEPS = 120, 110, 40, 65535
RECORD_BYTES, GENERATOR_BYTES = 752, 2560                                                # device bytes per env; + 8 per batch (the error counter)


class SpaceStationVectorEnv(DeviceVectorEnv):
    """N independent SpaceStationEnv instances (six crew members, twelve systems, eight modules in orbit; a step is five minutes) stepped
    by one HIP kernel launch.  Actions as the reference: `Discrete(40)` (:123).  The reference declares `Box(-inf, inf, (110,))`
    (:126-131) and returns 120 float32 values (24 crew + 36 systems + 32 modules + 10 power + 8 resources + 4 orbit + 6 alerts); the
    space here is `Box(-inf, inf, (120,), float32)`, what is returned.

    Bit-exact with the reference: observations, the integer-valued reward (its float64 value, rounded to float32 on output), both
    flags and the float64 info values.  One caveat: the 32 Gaussian draws of a reset go through `log`, and where the device's float64
    `log` differs from glibc's in the last place the float64 module state after that reset does too (it has to cross a float32
    rounding boundary or a threshold to show in an output; profiles/space_station_timing.txt has the measured count).

    The reference's quirks are kept, each is observable: reset() does not touch `episode_reward` (info), `last_emergency_time` (the
    reward's "+500 while handling"), the crew's `current_module` (after action 38 everybody stays in Docking for good), `solar_angle`,
    `radiation_level` and `total_power_consumption` (elements 111, 113 and 94 of a reset observation are the previous episode's last
    values); `crew_casualties` grows by one per dead member per step, so the reward's `-5000 * casualties` grows without bound; a
    medical emergency leaves a negative health in that step's observation; `system_failures` is a list of names in the reference
    and its length here, with the 12-bit `system_failure_mask` (`SYSTEMS`) beside it.

    `terminated` when all six healths are <= 0, three critical systems are below 10 % efficiency, the mean oxygen is below 15 or the
    mean pressure below 80, or `max_steps` (the reference's attribute, 8640; 1..65535) is reached — which raises `truncated` too and
    sets `mission_success`.  In Disabled mode the reference may be stepped on past termination; so may this.  In SameStep mode
    `infos["final_obs"]` is valid where `terminated`; its other rows are unspecified.

    Streams: the reference draws from the process-global `np.random` and never seeds it, so env i owns the stream
    `np.random.seed(seed + env_index0 + i)`.  `reset(seed=s)` is `np.random.seed(s_i); env = SpaceStationEnv(); env.reset(seed=s_i)`
    (the constructor draws nothing): a fresh object, with the fields above at the constructor's values.  A reset() without a seed,
    `reset_mask` and every autoreset continue the stream and keep them.  A new batch is seeded with 0.

    Actions: int32 [N].  An action of 40 or above falls through every branch of `_process_action` in the reference, a negative one
    would index its systems from the back or raise; here both skip `_process_action`, the rest of the step runs, and
    `invalid_action_count()` counts them.

    rollout(k): k fused step()s in one launch.  actions: None -> counter-hash actions cge_hash_action(action_seed, env_index0 + i,
    t0 + t, 40, 0), or int32 [k, N].  Returns (obs, reward_sum, done_count) with obs [k, N, 120] if trajectory else the last step's
    [N, 120]; with per_step=True (obs, reward[k, N], terminated[k, N], reward_sum, done_count).  A SAME_STEP trajectory holds the reset
    observation at a terminated step, as step()'s `obs` does; the terminal rows of a fused rollout go to a side
    output once `collect_final_obs()` has registered one (`final_obs()`, `final_obs_dropped()`; segments of 64 envs).  Its per-step
    `truncated` (terminated in the step that reaches `max_steps`) is not delivered.

    Not built: a registry id, rendering, a bench workload, canonical get_state / set_state
    records (`snapshot()` / `restore()` checkpoint the whole batch)."""

    _abi = "cge_space_station"
    _seed_bits = 32   # np.random.seed(s_i)
    INFO_FIELDS = INFO_FIELDS
    _flags = TERMINATED_AT_LIMIT
    _invalid_action_text = "Invalid action in {n} env-step(s): must be an integer 0-39"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_steps=8640, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.max_steps = int(max_steps)
        self.single_action_space = Discrete(NUM_ACTIONS)
        self.single_observation_space = Box(-np.inf, np.inf, (OBS_DIM,), np.float32)
        self._obs_shape = (self.num_envs, OBS_DIM)
        self._create(_native.SpaceStationConfig(self._mode_code, self.max_steps), info_fields, record_episode_statistics, reference_info)

    def _create_error(self, status):
        if status == -1 and not 1 <= self.max_steps <= MAX_STEPS:
            return ValueError(f"max_steps must be in 1..{MAX_STEPS}, got {self.max_steps}")
        return None

    def reference_info(self):
        """The reference's `info` dict (:787-797): its nine keys in its order, one float64 tensor [N] per key (`system_failures` is the
        length of the reference's list; `info("system_failure_mask")` says which systems it names)."""
        return {key: self.info(key) for key in REFERENCE_INFO_KEYS}
