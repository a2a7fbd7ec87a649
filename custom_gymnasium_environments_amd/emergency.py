"""EmergencyVectorEnv — batched drop-in for EmergencyResponseEnv (emergency_response_env/emergency_env.py:106-922)."""
import numpy as np

from . import _native
from ._spaces import Box, Discrete
from .vector_env import DeviceVectorEnv

INFO_FIELDS = {"active_emergencies": 0, "total_casualties": 1, "lives_saved": 2, "emergencies_resolved": 3, "avg_response_time": 4,
               "termination_reason": 5, "timestep": 6, "needs_reset": 7, "busy_units": 8, "mutual_aid_requested": 9, "national_guard_active": 10,
               "state_of_emergency": 11}
REFERENCE_INFO_KEYS = ("active_emergencies", "total_casualties", "lives_saved", "emergencies_resolved", "avg_response_time",
                       "termination_reason")                                            # :913-920, in its order
TERMINATION_REASONS = (None, "success", "casualties", "overwhelmed", "timeout")           # what the code of `termination_reason` stands for
OBS_DIM, NUM_ACTIONS, MAX_TIMESTEPS = 276, 50, 65535
RECORD_BYTES, GENERATOR_BYTES = 808, 2560                                                # device bytes per env; + 8 per batch (the error counter)


class EmergencyVectorEnv(DeviceVectorEnv):
    """N independent EmergencyResponseEnv instances (a 30 x 30 city, up to 20 incidents, 40 response units, 8 hospitals, weather and 25
    traffic segments; a step is a minute) stepped by one HIP kernel launch.  Spaces as the reference: `Discrete(50)` actions (:190)
    and a `Box(0, 10, (276,), float32)` observation (:182-187).

    Bit-exact with the reference: observations, the integer-valued reward (its float64 value, rounded to float32 on output), flags
    and the float64 info values; `termination_reason` is carried as a code (0 none, 1 success, 2 casualties, 3 overwhelmed,
    4 timeout: `TERMINATION_REASONS`).

    The reference's quirks are kept, each is observable: actions 0..19 dispatch the twelve fire trucks and eight police cars, nothing
    dispatches the other twenty units, so an incident that needs only ambulances is never resolved; a freed unit stays at the
    incident's cell until its next arrival; an incident's required units are computed at its creation and at an escalation only, not
    when work lowers its severity; a contained incident still counts for the step's traffic; the readiness bonuses of actions 44 and
    47 last for the step they are taken in; the reward's `_prev_` counters survive reset(), so the first step of a later episode pays
    no reward for what the counters had reached; termination is tested before the clock moves, the observation taken after.

    `terminated` on success (no incident after minute 60), more than 50 casualties, a mean response time above 45 minutes, or
    `max_timesteps` (the reference's attribute, 1440; 1..65535) reached; `truncated` never.  In Disabled mode the reference may be
    stepped on past termination; so may this.  In SameStep mode `infos["final_obs"]` is valid where `terminated`; its other rows are
    unspecified.

    Streams: the reference draws from the process-global `random` and never seeds it, so env i owns the stream
    `random.seed(seed + env_index0 + i)`.  The NETWORK — population densities, the stations of units 30..39, the hospitals — is drawn
    once by the reference's constructor, which does not reset, and survives every reset().  `reset(seed=s)` is therefore
    `random.seed(s_i); env = EmergencyResponseEnv(); env.reset(seed=s_i)`.  A reset() without a seed, `reset_mask` and every
    autoreset continue the stream and keep the network.  A new batch is seeded with 0 and holds no incident before its first reset.

    Actions: int32 [N].  An action below 0 or above 49 falls through every branch of `_execute_action`, as it does in the reference;
    the rest of the step runs, and `invalid_action_count()` counts it.

    rollout(k): k fused step()s in one launch.  actions: None -> counter-hash actions cge_hash_action(action_seed, env_index0 + i,
    t0 + t, 50, 0), or int32 [k, N].  Returns (obs, reward_sum, done_count) with obs [k, N, 276] if trajectory else the last step's
    [N, 276]; with per_step=True (obs, reward[k, N], terminated[k, N], reward_sum, done_count).  A SAME_STEP trajectory holds the reset
    observation at a terminated step, as step()'s `obs` does; the terminal rows of a fused rollout go to a side
    output once `collect_final_obs()` has registered one (`final_obs()`, `final_obs_dropped()`; segments of 64 envs).

    Not built: a registry id, rendering, a bench workload, canonical get_state / set_state
    records (`snapshot()` / `restore()` checkpoint the whole batch)."""

    _abi = "cge_emergency"
    INFO_FIELDS = INFO_FIELDS
    _invalid_action_text = "Invalid action in {n} env-step(s): must be an integer 0-49"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_timesteps=1440, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.max_timesteps = int(max_timesteps)
        self.single_action_space = Discrete(NUM_ACTIONS)
        self.single_observation_space = Box(0.0, 10.0, (OBS_DIM,), np.float32)
        self._obs_shape = (self.num_envs, OBS_DIM)
        self._create(_native.EmergencyConfig(self._mode_code, self.max_timesteps), info_fields, record_episode_statistics, reference_info)

    def _create_error(self, status):
        if status == -1 and not 1 <= self.max_timesteps <= MAX_TIMESTEPS:
            return ValueError(f"max_timesteps must be in 1..{MAX_TIMESTEPS}, got {self.max_timesteps}")
        return None

    def reference_info(self):
        """The reference's `info` dict (:913-920): its six keys in its order, one float64 tensor [N] per key."""
        return {key: self.info(key) for key in REFERENCE_INFO_KEYS}
