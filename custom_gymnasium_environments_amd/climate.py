"""ClimateVectorEnv — batched drop-in for SmartClimateEnv (smartclimate_rl-main/smartclimate/env.py:10-116)."""
import numpy as np
import torch

from . import _native
from ._spaces import Box
from .vector_env import DeviceVectorEnv

INFO_FIELDS = {"room_temp": 0, "outside_temp": 1, "ac_setting": 2, "energy_usage": 3, "total_reward": 4, "num_people": 5,
               "step": 6, "comfort_time": 7, "episodes": 8, "needs_reset": 9}
OBS_DIM = 9


class ClimateVectorEnv(DeviceVectorEnv):
    """N independent SmartClimateEnv instances stepped by one HIP kernel launch.

    Observation `Box((9,), float32)`: room_temp, num_people, time_of_day, outside_temp, ac_setting, 4 light
    states (:74-83).  Action: the reference's Dict space (:39-43) batched — `{"ac_temp": float32 (N,1),
    "lights": int8 (N,4)}` (a tuple `(ac_temp, lights)` is accepted too).  `reset(seed=s)` gives env i the
    private generator `np.random.default_rng(s + env_index0 + i)` (:63-65); float64 dynamics, float32 obs.
    """

    _abi = "cge_climate"
    INFO_FIELDS = INFO_FIELDS
    _action_ptrs = 2                     # ac_temp float32 [N], lights int8 [N, 4]
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_occupancy=8, episode_minutes=1440,
                 reuse_buffers=False, info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        lo = np.array([0.0, 0, 0.0, 10.0, 16.0, 0, 0, 0, 0]); hi = np.array([50.0, max_occupancy, 23.99, 50.0, 32.0, 1, 1, 1, 1])
        self.single_observation_space = Box(lo, hi, (OBS_DIM,), np.float32)
        self.single_action_space = {"ac_temp": Box(16.0, 32.0, (1,), np.float32), "lights": Box(0, 1, (4,), np.int8)}
        self._obs_shape = (self.num_envs, OBS_DIM)
        self._create(_native.ClimateConfig(int(max_occupancy), int(episode_minutes), self._mode_code, 0), info_fields,
                     record_episode_statistics, reference_info)

    def _split(self, actions, k=None):
        ac, li = (actions["ac_temp"], actions["lights"]) if isinstance(actions, dict) else actions
        lead = (self.num_envs,) if k is None else (k, self.num_envs)
        ac = torch.as_tensor(ac) if not isinstance(ac, torch.Tensor) else ac
        ac = ac.reshape(lead).to(device=self.device, dtype=torch.float32).contiguous()
        li = self._as_device(li, torch.int8, lead + (4,), "lights")
        return ac, li

    _device_actions = _split

    def reference_info(self, obs=None):
        """The reference's step() `info` under ITS keys (env.py:105-110): the three terms of calculate_reward (utils.py:30-50) —
        comfort (10 / 5 / 0 / -15 |T - 22| by the room temperature's band), ac_penalty = -0.5 |ac_setting - outside_temp|,
        light_penalty = -max(0, lights_on - min(4, ceil(num_people / 2))) — and comfort_time, energy_usage, step; float64, from the
        env's CURRENT state (room / outside temperature, AC setting and occupancy from the state record, the light switches from the
        observation: `obs`, default the last one step() / reset() returned).  `reference_info=True` merges it into every `infos`."""
        obs = self._last_obs if obs is None else obs
        room, out, ac, people = self.info("room_temp"), self.info("outside_temp"), self.info("ac_setting"), self.info("num_people")
        comfort = torch.where((room >= 20) & (room <= 24), torch.full_like(room, 10.0),
                              torch.where((room >= 18) & (room <= 26), torch.full_like(room, 5.0),
                                          torch.where((room >= 16) & (room <= 28), torch.zeros_like(room), -15.0 * (room - 22.0).abs())))
        lights_on = obs[:, 5:9].to(torch.float64).sum(1)
        required = torch.clamp(torch.ceil(people / 2.0), max=4.0)
        return {"comfort": comfort, "ac_penalty": -0.5 * (ac - out).abs(), "light_penalty": -torch.clamp(lights_on - required, min=0.0),
                "comfort_time": self.info("comfort_time").to(torch.int64), "energy_usage": self.info("energy_usage"),
                "step": self.info("step").to(torch.int64)}
