"""SnakeVectorEnv — batched drop-in for SnakeEnvClassic (snake_env_classic/snake_env.py:9-143)."""
import numpy as np
import torch

from . import _native
from ._spaces import Box, Discrete
from .vector_env import DeviceVectorEnv

INFO_FIELDS = {"score": 0, "snake_length": 1, "steps": 2, "direction": 3, "food_r": 4, "food_c": 5,
               "board_full": 6, "episodes": 7, "head_r": 8, "head_c": 9, "needs_reset": 10}


class SnakeVectorEnv(DeviceVectorEnv):
    """N independent SnakeEnvClassic instances stepped by one HIP kernel launch.

    Same spaces as the reference (snake_env.py:26-32): `Discrete(4)` actions (0 up, 1 right,
    2 down, 3 left), obs `Box(0, 2, (G, G), int8)` (0 empty, 1 snake, 2 food); rewards
    -10 / 0 / +10; `terminated` on wall or self collision or after `max_steps`=1000 steps;
    `truncated` is always False (snake_env.py:119).

    RNG protocol: the reference draws food positions from the process-global `random` and never
    seeds it; here env i owns the stream `random.seed(seed + env_index0 + i)` (bit-exact CPython
    MT19937), which is what one gets from the reference by running that env alone after
    `random.seed(...)`.  Auto-reset continues the stream, as `env.reset()` does.

    info_fields: names from INFO_FIELDS to return in `infos` each step (the reference returns
    `score` and `snake_length`, snake_env.py:63,117); each costs one small kernel, default none.

    rollout(k): k fused step()s in one launch (state stays in registers).  actions: None -> counter-hash
    random actions (cge_hash_action) or an int32 [k, N] tensor.  Returns (obs, reward_sum, done_count)
    with obs of shape [k, N, G, G] if trajectory else the last step's [N, G, G]; with per_step=True
    returns (obs, reward[k, N], terminated[k, N], reward_sum, done_count) — the outputs of k step() calls.
    reward_sum is float32 here and float64 for every other env type.
    """

    _abi = "cge_snake"
    INFO_FIELDS = INFO_FIELDS
    _obs_dtype = torch.int8
    _reward_sum_dtype = torch.float32
    _info_dtype = torch.int32
    _invalid_action_text = "Invalid action in {n} env-step(s)"   # an action outside 0..3 (reference: ValueError, snake_env.py:69-70)
    metadata = {"render_modes": ["rgb_array"]}

    def __init__(self, num_envs, grid_size=20, device="cuda:0", autoreset_mode="NextStep", env_index0=0,
                 max_steps=1000, reuse_buffers=False, info_fields=(), record_episode_statistics=False, render_mode=None,
                 reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        if render_mode not in (None, "rgb_array"):
            raise ValueError("render_mode must be None or 'rgb_array' (the pygame window of 'human' is out of scope)")
        self.render_mode = render_mode
        self.grid_size = int(grid_size)
        self.max_steps = int(max_steps)
        self.single_action_space = Discrete(4)
        self.single_observation_space = Box(0, 2, (self.grid_size, self.grid_size), np.int8)
        self._obs_shape = (self.num_envs, self.grid_size, self.grid_size)
        self._create(_native.SnakeConfig(self.grid_size, self.max_steps, self._mode_code, 0), info_fields, record_episode_statistics,
                     reference_info)

    def _create_error(self, status):
        if status == -3:
            return ValueError(f"grid_size={self.grid_size} is not compiled into libcge_amd.so (supported: every size from 4 to 30)")

    # ------------------------------------------------------------------ extras
    def render_rgb(self):
        """render_mode="rgb_array" for the whole batch (snake_env.py:175-188): uint8 [N, G, G, 3] of the current states —
        empty black, snake (0, 255, 0), food (255, 0, 0)."""
        out = self._out("rgb", self._obs_shape + (3,), torch.uint8)
        self._check(self._lib.cge_snake_render_rgb(self._h, out.data_ptr(), self._stream()), "render_rgb")
        return out

    def render(self):
        """gymnasium.vector.VectorEnv.render(): a tuple with one frame per env when render_mode == "rgb_array"."""
        if self.render_mode != "rgb_array":
            return None
        return tuple(self.render_rgb())

    def reference_info(self):
        """The reference's `info` (snake_env.py:62,117): {"score", "snake_length"} of the env's CURRENT state — after a SAME_STEP
        auto-reset that is the fresh episode's (the finished episode's score is what `record_episode_statistics` reports:
        return = 10 * score - 10 on a crash).  `reference_info=True` merges it into every `infos`."""
        return {"score": self.info("score"), "snake_length": self.info("snake_length")}
