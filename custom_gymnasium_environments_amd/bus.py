"""BusVectorEnv — batched drop-in for BusSystemEnv (bus_system_env/environment.py:44-383)."""
import ctypes as C

import numpy as np
import torch

from . import _native
from ._spaces import Box, Dict, Discrete, MultiBinary, MultiDiscrete, batch_space
from .vector_env import DeviceVectorEnv

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


class BusVectorEnv(DeviceVectorEnv):
    """N independent BusSystemEnv instances (4 buses on a ring of 4 stops, 50..150 passengers per episode, 500 steps) stepped by one
    HIP kernel launch.  Spaces as the reference: `MultiDiscrete([11] * 4)` actions (the dwell time each bus takes when it next
    arrives at a stop, :82) and the `Dict` observation of :94-123 with its eleven keys and bounds.  Bit-exact with the reference.

    Observations are dicts of int32 device tensors, one per key, in gymnasium's batched-Dict layout ([N, 4], [N, 4, 4] or [N]); all
    are views of ONE slab the kernel writes key by key (`obs_slab(obs)` gives it back).  The reference's `bus_states` is int8 and
    its four scalars are Python ints; here everything is int32.  `terminated` is never set (:156); `truncated`
    after `max_timesteps` steps.

    The reference never seeds `random` (reset(seed) reaches np_random only, :127) while generate_passengers (utils.py:22-46) draws
    from it, so env i owns the stream `random.seed(seed + env_index0 + i)`, as ParkingVectorEnv and SnakeVectorEnv do.  A new batch
    holds empty stops until its first reset()."""

    _abi = "cge_bus"
    _obs_dtype = torch.int32
    metadata = {"render_modes": []}

    def __init__(self, num_envs, device="cuda:0", autoreset_mode="NextStep", env_index0=0, max_timesteps=500, reuse_buffers=False,
                 info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        self._reference_info = bool(reference_info)
        self.max_timesteps = int(max_timesteps)
        self.single_observation_space, self.single_action_space = make_spaces(self.max_timesteps)
        self.action_space = batch_space(self.single_action_space, self.num_envs)
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)
        for f in info_fields:
            if f not in INFO_FIELDS:
                raise ValueError(f"unknown info field {f!r}; choose from {sorted(INFO_FIELDS)}")
        self.info_fields = tuple(info_fields)
        cfg = _native.BusConfig(self.max_timesteps, self._mode_code)
        h = C.c_void_p()
        _native.check(self._lib.cge_bus_create(C.byref(cfg), self.num_envs, self._dev_index, self.env_index0, C.byref(h)), what="cge_bus_create")
        self._h = h
        self._slab = self.num_envs * OBS_INTS
        self._views = {}
        self.record_episode_statistics(record_episode_statistics)

    # ------------------------------------------------------------------ the slab and its per-key views
    def _dict(self, slab):
        """slab int32 [56 * N] or [k, 56 * N] -> {key: view [N, ...] or [k, N, ...]}.  The dict of a persistent buffer is built once."""
        key = (slab.data_ptr(), tuple(slab.shape)) if self._reuse else None
        d = self._views.get(key) if key is not None else None
        if d is None:
            n, d, o = self.num_envs, {}, 0
            for name, shape in PLANES:
                w = n * int(np.prod(shape))
                d[name] = slab[..., o:o + w].view(slab.shape[:-1] + (n,) + shape)
                o += w
            if key is not None:
                self._views = {k: v for k, v in self._views.items() if k[0] != key[0]}       # a regrown buffer drops its old views
                self._views[key] = d
        return dict(d)

    def obs_slab(self, obs):
        """The flat int32 slab ([56 * N], or [k, 56 * N] for a trajectory) behind an observation dict of this env."""
        first = obs["bus_stops"]
        lead = first.shape[:-2]
        return torch.as_strided(first, lead + (self._slab,), tuple(first.stride()[:len(lead)]) + (1,), first.storage_offset())

    # ------------------------------------------------------------------ gymnasium API
    def reset(self, *, seed=None, options=None):
        self._seed_native(seed)
        mask = None
        if options and options.get("reset_mask") is not None:
            mask = self._as_device(options["reset_mask"], torch.uint8, (self.num_envs,), "reset_mask")
        obs = self._out("obs", (self._slab,), torch.int32)
        self._check(self._lib.cge_bus_reset(self._h, mask.data_ptr() if mask is not None else None, obs.data_ptr(), self._stream()), "reset")
        return self._dict(obs), self._infos()

    def step(self, actions):
        a = self._as_device(actions, torch.int32, (self.num_envs, NUM_BUSES), "actions")
        obs = self._out("obs", (self._slab,), torch.int32)
        rew = self._out("reward", (self.num_envs,), torch.float32)
        term = self._out("terminated", (self.num_envs,), torch.bool)
        trunc = self._out("truncated", (self.num_envs,), torch.bool)
        same = self._mode_code == _native.AUTORESET_SAME_STEP
        fin = self._out("final_obs", (self._slab,), torch.int32) if same else None
        self._check(self._lib.cge_bus_step(self._h, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                           fin.data_ptr() if same else None, self._stream()), "step")
        infos = self._infos()
        if same:
            infos["final_obs"] = self._dict(fin)             # rows are valid where _final_obs is True (gymnasium's SAME_STEP convention)
            infos["_final_obs"] = trunc
        return self._dict(obs), rew, term, trunc, self._episode_infos(infos, trunc)

    def rollout(self, k_steps, actions=None, action_seed=0, t0=0, trajectory=False, want_obs=True, per_step=False):
        """k fused step()s in one launch (the record stays in registers).  actions: None -> counter-hash dwell times
        (cge_hash_action(action_seed, env_index0 + i, t0 + t, 11, bus)) or int32 [k, N, 4].  Returns (obs, reward_sum, done_count)
        with obs a dict of views [k, N, ...] if trajectory else the last step's [N, ...]; with per_step=True
        (obs, reward[k, N], truncated[k, N], reward_sum, done_count) — the outputs of k step() calls (a SAME_STEP trajectory holds
        the reset observation at a truncated step, as step()'s `obs` does)."""
        k = int(k_steps)
        a = None if actions is None else self._as_device(actions, torch.int32, (k, self.num_envs, NUM_BUSES), "actions")
        obs, stride = None, 0
        if want_obs:
            if trajectory:
                obs = self._out("traj", (k, self._slab), torch.int32)
                stride = self._slab
            else:
                obs = self._out("obs", (self._slab,), torch.int32)
        rs = self._out("reward_sum", (self.num_envs,), torch.float64)
        dc = self._out("done_count", (self.num_envs,), torch.int32)
        rt = tt = None
        if per_step:
            rt = self._out("reward_traj", (k, self.num_envs), torch.float32)
            tt = self._out("truncated_traj", (k, self.num_envs), torch.bool)
        self._check(self._lib.cge_bus_rollout(self._h, k, a.data_ptr() if a is not None else None, int(action_seed), int(t0),
                                              obs.data_ptr() if obs is not None else None, stride,
                                              rt.data_ptr() if per_step else None, tt.data_ptr() if per_step else None,
                                              rs.data_ptr(), dc.data_ptr(), self._stream()), "rollout")
        od = self._dict(obs) if obs is not None else None
        return (od, rt, tt, rs, dc) if per_step else (od, rs, dc)

    # ------------------------------------------------------------------ extras
    def info(self, field, index=0):
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._check(self._lib.cge_bus_info(self._h, INFO_FIELDS[field], int(index), out.data_ptr(), self._stream()), "info")
        return out

    def _infos(self):
        d = {f: self.info(f) for f in self.info_fields}
        if self._reference_info:
            d.update(self.reference_info())
        return d

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

    def invalid_action_count(self):
        """Synchronises; number of env-steps refused for a dwell time outside 0..10 since the last call (reference: ValueError)."""
        return int(self._lib.cge_bus_error_count(self._h, self._stream()))

    def check_actions(self):
        n = self.invalid_action_count()
        if n:
            raise ValueError(f"Invalid action in {n} env-step(s): must be {NUM_BUSES} integers 0-{MAX_DWELL_TIME}")   # :160-161
