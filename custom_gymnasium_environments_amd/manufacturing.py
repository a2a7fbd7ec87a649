"""ManufacturingVectorEnv — batched drop-in for SmartManufacturingEnv (smart_manufacturing_env/manufacturing_env.py:69-606)."""
import numpy as np

from . import _native
from ._spaces import Box, Discrete, MultiDiscrete  # noqa: F401
from .vector_env import BOTH, DeviceVectorEnv

INFO_FIELDS = {"raw_material": 0, "energy_consumption": 1, "total_reward": 2, "in_system": 3, "completed": 4, "scrapped": 5,
               "product_ids": 6, "history_len": 7, "oee_availability": 8, "oee_performance": 9, "oee_quality": 10,
               "timestep": 11, "episodes": 12, "needs_reset": 13, "overflow": 14,
               "completed_A": 15, "completed_B": 16, "completed_C": 17, "completed_D": 18, "completed_E": 19, "completed_F": 20}
OBS_DIM = 73


class ManufacturingVectorEnv(DeviceVectorEnv):
    """N independent SmartManufacturingEnv instances (5 stations, 6 product types, quality checkpoints, machine breakdowns,
    supply disruptions) stepped by one HIP kernel launch.  Actions `Discrete(25)` (:303-359), obs float32 (73,).  Both
    `terminated` (:555-578) and `truncated` (timestep >= 1500) are reported; auto-reset triggers on either.  `reset(seed=s)`
    gives env i gymnasium's `np_random` for seed s + env_index0 + i (PCG64 from SeedSequence, :115); a later `reset()`
    continues the stream.  Bit-exact with the reference, including the NumPy pairwise-summed per-type quality means."""

    _abi = "cge_manufacturing"
    INFO_FIELDS = INFO_FIELDS
    _flags = BOTH
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_steps=1500, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.single_action_space = Discrete(25)
        self.single_observation_space = Box(0.0, 500.0, (OBS_DIM,), np.float32)
        self._obs_shape = (self.num_envs, OBS_DIM)
        self._create(_native.ManufacturingConfig(int(max_steps), self._mode_code), info_fields, record_episode_statistics, reference_info)

    def reference_info(self):
        """The reference's `info` under ITS keys (manufacturing_env.py:293-299, reset: :184-190): timestep, total_reward,
        products_completed (the per-type dict, :157,485), oee {availability, performance, quality} (:533-549), energy_consumption.
        `reference_info=True` merges it into every `infos`."""
        import torch
        return {"timestep": self.info("timestep").to(torch.int64), "total_reward": self.info("total_reward"),
                "products_completed": {k: self.info(f"completed_{k}").to(torch.int64) for k in "ABCDEF"},
                "oee": {"availability": self.info("oee_availability"), "performance": self.info("oee_performance"), "quality": self.info("oee_quality")},
                "energy_consumption": self.info("energy_consumption")}
