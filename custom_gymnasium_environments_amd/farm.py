"""AgriculturalFarmVectorEnv — batched drop-in for AgriculturalFarmEnv (agricultural_farm_env/farm_env.py:116-935, crops/crop_data.py)."""
import numpy as np
import torch

from . import _native
from ._spaces import Box, Discrete
from .vector_env import DeviceVectorEnv

REFERENCE_INFO_KEYS = ("day", "season", "year", "cash_flow", "total_revenue", "total_expenses", "profit_margin", "carbon_sequestered",
                       "water_conservation_score", "biodiversity_index", "soil_health_trend")     # :913-924, in its order
FIELD_INFO_KEYS = ("field_crop", "field_stage", "field_health", "field_yield_potential")         # field_status :925-934, [N, 4] each
INFO_FIELDS = {**{k: i for i, k in enumerate(REFERENCE_INFO_KEYS)}, **{k: 11 + 4 * i for i, k in enumerate(FIELD_INFO_KEYS)},
               "needs_reset": 27, "water_quality": 28}
SEASONS = ("spring", "summer", "fall", "winter")                                                  # `season`
CROPS = ("Wheat", "Corn", "Tomatoes", "Apples", "Soybeans")                                       # `field_crop`; -1 is "None"
OBS_DIM, COMPACT_OBS_DIM, NUM_ACTIONS, NUM_FIELDS, MAX_YEARS = 620, 134, 45, 4, 255
RECORD_BYTES, GENERATOR_BYTES = 832, 2 * 2560                                            # device bytes per env; + 8 per batch (the error counter)


class AgriculturalFarmVectorEnv(DeviceVectorEnv):
    """N independent AgriculturalFarmEnv instances (four fields, eight machines, a market of five crops, weather by season; a step is
    a day, a season 90 days) stepped by one HIP kernel launch.  Actions as the reference: `Discrete(45)` (:179).  Observations as
    the reference declares and returns them: `Box(-inf, inf, (620,), float32)` (:183-185), of which 134 values are live (60 fields +
    10 weather + 40 equipment + 10 market + 5 water + 5 finances + 4 sustainability) and 486 are the reference's zero padding.
    `compact_obs=True` makes the space `Box(-inf, inf, (134,), float32)` and the rows the 134 leading values only: a `[k, N, 620]`
    trajectory is mostly zeros (32 steps of 1,048,576 envs are 83 GB).

    Bit-exact with the reference: observations, the integer-valued reward, `terminated` and the float64 info values.  One caveat:
    the five Gaussians of a step's prices go through `log`, and where the device's float64 `log` differs from glibc's in the last
    place a float64 price does too (it has to cross a float32 rounding boundary or a threshold to show in an output; the number of
    draws never depends on a price; profiles/farm_timing.txt has the measured count).

    The reference's quirks are kept, each is observable: `CropType.WHEAT` is 0 and false, so a wheat field shows -1 / "None", takes
    no weather damage, sequesters no carbon and is skipped by actions 42 and 43, while growth, soil depletion and the plant action
    (`is not None`) treat it as planted, and a wheat `last_crop` earns no rotation bonus; the three initial crops start DORMANT and
    never grow, so only field 3 is ever planted (action 3) or harvested; actions 4, 9, 14, 19, 24 and 34 name a fifth field and do
    nothing; `is_operating` is never cleared within an episode (50 a day per machine from then on) and an operating machine compacts
    nothing; weather damage leaves a negative health in that step's observation; the soil termination cannot fire; reset() does not
    touch `water_quality`.

    `terminated` when `year > max_years` (the reference's attribute, 1; 1..255) — in the step that makes the day a multiple of 360 —
    or when `cash_flow < -50000` (-5000).  The reference never truncates.  In Disabled mode the reference may be stepped on past
    termination; so may this.  In SameStep mode `infos["final_obs"]` is valid where `terminated`; its other rows are unspecified.
    The terminal rows of a fused rollout go to a side output once `collect_final_obs()` has registered one (`final_obs()`,
    `final_obs_dropped()`; segments of 64 envs), in either layout.

    Streams: the reference draws from the process-global `np.random` and, for the crop it plants, from CPython's global `random`,
    and seeds neither, so env i owns both streams of `s_i = seed + env_index0 + i`.  `reset(seed=s)` is `random.seed(s_i);
    np.random.seed(s_i); env = AgriculturalFarmEnv(); env.reset(seed=s_i)`: the constructor draws the fields, the equipment and
    the market, reset() draws them again.  A reset() without a seed, `reset_mask` and every autoreset continue both streams, the
    legacy Gaussian's cached second value included, and keep `water_quality`.  A new batch is seeded with 0.

    Actions: int32 [N].  An action outside 0..44 falls through every branch of `_process_action`, as in the reference; the rest of
    the step runs, and `invalid_action_count()` counts it.

    rollout(k): k fused step()s in one launch.  actions: None -> counter-hash actions cge_hash_action(action_seed, env_index0 + i,
    t0 + t, 45, 0), or int32 [k, N].  Returns (obs, reward_sum, done_count) with obs [k, N, 620 | 134] if trajectory else the last
    step's; with per_step=True (obs, reward[k, N], terminated[k, N], reward_sum, done_count).  A SAME_STEP trajectory holds the reset
    observation at a terminated step, as step()'s `obs` does.

    Not built: a registry id (the reference registers none), rendering, a bench workload,
    canonical get_state / set_state records (`snapshot()` / `restore()` checkpoint the whole batch)."""

    _abi = "cge_farm"
    _seed_bits = 32   # np.random.seed(s_i)
    INFO_FIELDS = INFO_FIELDS
    _invalid_action_text = "Invalid action in {n} env-step(s): must be an integer 0-44"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_years=1, compact_obs=False, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.max_years = int(max_years)
        self.compact_obs = bool(compact_obs)
        width = COMPACT_OBS_DIM if self.compact_obs else OBS_DIM
        self.single_action_space = Discrete(NUM_ACTIONS)
        self.single_observation_space = Box(-np.inf, np.inf, (width,), np.float32)
        self._obs_shape = (self.num_envs, width)
        self._create(_native.FarmConfig(self._mode_code, self.max_years, int(self.compact_obs), 0), info_fields, record_episode_statistics, reference_info)

    def _create_error(self, status):
        if status == -1 and not 1 <= self.max_years <= MAX_YEARS:
            return ValueError(f"max_years must be in 1..{MAX_YEARS}, got {self.max_years}")
        return None

    def info(self, field, index=0):
        """One field of INFO_FIELDS for every env, float64 [N]; the four `field_*` values of `field_status` are [N, 4], a column per field."""
        if field not in FIELD_INFO_KEYS:
            return super().info(field, index)
        if index:
            raise TypeError(f"{type(self).__name__}.info() takes no index")
        out = torch.empty((NUM_FIELDS, self.num_envs), dtype=self._info_dtype, device=self.device)
        for k in range(NUM_FIELDS):
            self._check(self._c_info(self._h, INFO_FIELDS[field] + k, out[k].data_ptr(), self._stream()), "info")
        return out.t().contiguous()

    def reference_info(self):
        """The reference's `info` dict (:911-935): its eleven scalar keys in its order, one float64 tensor [N] per key (`season` as
        0..3, `SEASONS` has the names), then `field_status` as four [N, 4] tensors: `field_crop` (the index into `CROPS`, -1 where the
        reference prints "None", which it does for wheat too), `field_stage`, `field_health` and `field_yield_potential`."""
        return {key: self.info(key) for key in REFERENCE_INFO_KEYS + FIELD_INFO_KEYS}
