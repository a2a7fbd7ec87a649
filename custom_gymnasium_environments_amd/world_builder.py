"""WorldBuilderVectorEnv — batched drop-in for WorldBuilderEnv (world_builder_env/src/environment/world_builder_env.py:11-248)."""
import numpy as np
import torch

from . import _native
from ._spaces import Box, Dict, Discrete
from ._slab import SlabVectorEnv
from .vector_env import TERMINATED

INFO_FIELDS = {"steps": 0, "win_steps": 1, "reached_win_population": 2, "food": 3, "wood": 4, "stone": 5, "population": 6,
               "population_capacity": 7, "building_count": 8, "needs_reset": 9}
BUILDINGS = ("farm", "lumberyard", "quarry", "house")                                  # ids 1..4 (:47-53)
MIN_GRID, MAX_GRID, WIN_STEPS = 2, 10, 50
_TORCH = {"int8": torch.int8, "float32": torch.float32, "int32": torch.int32}


def planes(grid_size):
    """The planes of one Dict observation slab in the order of include/cge_amd.h: (key, per-env shape, dtype name)."""
    g = int(grid_size)
    return (("grid", (g, g), "int8"), ("resources", (4,), "float32"), ("population_capacity", (1,), "float32"), ("win_steps", (1,), "int32"))


def slab_layout(num_envs, grid_size):
    """({key: byte offset}, slab bytes): key-major planes, each starting at a multiple of 16 bytes, the slab a multiple of 16."""
    offs, o = {}, 0
    for key, shape, dtype in planes(grid_size):
        offs[key] = o
        o = -(-(o + num_envs * int(np.prod(shape)) * np.dtype(dtype).itemsize) // 16) * 16
    return offs, o


def plane_table(num_envs, grid_size):
    """(the planes as _slab takes them: key, per-env shape, torch dtype, byte offset in the uint8 slab; slab bytes)."""
    offs, total = slab_layout(num_envs, grid_size)
    return tuple((key, shape, _TORCH[dtype], offs[key]) for key, shape, dtype in planes(grid_size)), total


def make_spaces(grid_size=10, flatten_obs=False):
    """(observation_space, action_space) of ONE WorldBuilderEnv (:57, :69-86)."""
    g = int(grid_size)
    if flatten_obs:
        return Box(0.0, 1000.0, (g * g + 6,), np.float32), Discrete(5)
    observation = Dict({
        "grid": Box(0, 4, (g, g), np.int8),
        "resources": Box(0.0, 1000.0, (4,), np.float32),
        "population_capacity": Box(0.0, 100.0, (1,), np.float32),
        "win_steps": Box(0, WIN_STEPS, (1,), np.int32),
    })
    return observation, Discrete(5)


class WorldBuilderVectorEnv(SlabVectorEnv):
    """N independent WorldBuilderEnv instances (a `grid_size` x `grid_size` grid, food / wood / stone, a population that must reach 20
    and hold for 50 steps) stepped by one HIP kernel launch.  Spaces as the reference: `Discrete(5)` actions (pass, farm, lumberyard,
    quarry, house) and either the `Dict` observation of :79-86 — int8 `grid`, float32 `resources` (food, wood, stone, population) and
    `population_capacity`, int32 `win_steps` — or, with `flatten_obs=True`, the float32 `Box(G*G + 6)` the reference's trainer uses
    (:69-77).  Bit-exact with the reference; `terminated` only, there is no time limit; `Box.high` is not enforced (the reference
    exceeds it too).

    Dict observations are dicts of typed device tensors in gymnasium's batched-Dict layout ([N, G, G], [N, 4], [N, 1], [N, 1]); all
    are views of ONE uint8 slab the kernel writes key by key (`obs_slab(obs)` gives it back).  SAME_STEP `infos["final_obs"]` is valid
    where `infos["_final_obs"]` is set.

    The reference never seeds the generator it draws from (reset(seed) reaches np_random only; _try_build calls the global
    np.random.randint, game_logic.py:130), so env i owns the stream `np.random.seed(seed + env_index0 + i)`, as ParkingVectorEnv,
    SnakeVectorEnv and BusVectorEnv do.  reset() draws nothing.

    rollout(k): k fused step()s in one launch (the record stays in registers).  actions: None -> counter-hash actions
    (cge_hash_action(action_seed, env_index0 + i, t0 + t, 5, 0)) or int32 [k, N].  A SAME_STEP trajectory holds the reset observation at
    a terminated step, as step()'s `obs` does; the terminal observations of a fused rollout go to a side output once
    `collect_final_obs()` has registered one: `final_obs()` returns (rows, step, env) with rows a dict of per-key tensors [m, G, G],
    [m, 4], [m, 1], [m, 1] — float32 rows [m, G*G + 6] with `flatten_obs=True` — and `final_obs_dropped()` what did not fit (segments
    of 64 envs).  get_state() / set_state(): canonical per-env records holding NumPy's own (key, pos) generator state
    (include/cge_amd.h)."""

    _abi = "cge_world_builder"
    _seed_bits = 32   # np.random.seed(s_i)
    INFO_FIELDS = INFO_FIELDS
    _action_shape = ()
    _flags = TERMINATED
    _info_dtype, _info_indexed = torch.int32, True
    # an env-step refused for an action outside 0..4 (reference: ValueError, :133-134)
    _invalid_action_text = "Invalid action in {n} env-step(s). Action space is Discrete(5)"
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, grid_size=10, flatten_obs=False,
                 reuse_buffers=False, info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self.grid_size, self.flatten_obs = int(grid_size), bool(flatten_obs)
        self.single_observation_space, self.single_action_space = make_spaces(self.grid_size, self.flatten_obs)
        self._offsets = slab_layout(self.num_envs, self.grid_size)[0]          # {key: byte offset}; nothing in the package or in tests/ reads it any more
        if self.flatten_obs:                                                    # plain float32 rows: no slab, no dict of views
            self._obs_dtype, self._obs_shape, self._wrap_obs = torch.float32, (self.num_envs, self.grid_size * self.grid_size + 6), None
        else:
            self._init_slab(*plane_table(self.num_envs, self.grid_size), torch.uint8)
        self._create(_native.WorldBuilderConfig(self.grid_size, int(self.flatten_obs), self._mode_code, 0), info_fields,
                     record_episode_statistics, reference_info)

    def _create_error(self, status):
        if status == -1 and not MIN_GRID <= self.grid_size <= MAX_GRID:
            return ValueError(f"grid_size must be in {MIN_GRID}..{MAX_GRID}, got {self.grid_size}")
        return None

    def _rows_layout(self, num_rows):
        return plane_table(num_rows, self.grid_size)

    # ------------------------------------------------------------------ extras
    def reference_info(self):
        """The reference's `info` dict under ITS keys (_get_info, :218-232), one tensor [N] per value: int32, `reached_win_population`
        bool; `resources` and `building_counts` are dicts of tensors.  `reference_info=True` in the constructor merges it into every
        step's / reset's infos (twelve small kernels per call: not for the hot loop)."""
        return {"steps": self.info("steps"), "win_steps": self.info("win_steps"),
                "reached_win_population": self.info("reached_win_population").bool(),
                "resources": {k: self.info(k) for k in ("food", "wood", "stone")},
                "population": self.info("population"), "population_capacity": self.info("population_capacity"),
                "building_counts": {k: self.info("building_count", j) for j, k in enumerate(BUILDINGS)}}
