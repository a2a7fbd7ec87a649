"""gymnasium.vector.VectorEnv façade over the C ABI (include/cge_amd.h): shared plumbing.

The reference implements single `gym.Env`s (L2 in SURVEY.md) and is batched only by gymnasium's
SyncVectorEnv Python loop inside RLlib (smart_parking_env/examples/training.py:43-47).  The classes
built on this module occupy that SyncVectorEnv slot: same attribute surface, same
reset()/step() return tuples, but the batch lives in HBM and one step() is one kernel launch.
Observations/rewards/flags are torch tensors on the env's device (no host sync per step).
"""
import ctypes as C
import enum

import numpy as np
import torch

from . import _native
from ._spaces import VectorEnvBase, batch_space

try:  # pragma: no cover
    from gymnasium.vector import AutoresetMode
except Exception:
    class AutoresetMode(enum.Enum):
        """Mirror of gymnasium.vector.AutoresetMode (gymnasium >= 1.1)."""
        NEXT_STEP = "NextStep"
        SAME_STEP = "SameStep"
        DISABLED = "Disabled"

_MODE_CODE = {"NEXT_STEP": _native.AUTORESET_NEXT_STEP, "SAME_STEP": _native.AUTORESET_SAME_STEP,
              "DISABLED": _native.AUTORESET_DISABLED}


def parse_autoreset_mode(mode):
    if isinstance(mode, str):
        key = mode.replace("-", "_").upper()
        key = {"NEXTSTEP": "NEXT_STEP", "SAMESTEP": "SAME_STEP"}.get(key, key)
        if key not in _MODE_CODE:
            raise ValueError(f"unknown autoreset_mode {mode!r}")
        return AutoresetMode[key]
    if hasattr(mode, "name") and mode.name in _MODE_CODE:
        return AutoresetMode[mode.name]
    raise ValueError(f"unknown autoreset_mode {mode!r}")


def _batch(space, n):
    """batch_space, key by key for a plain dict of spaces (climate's Dict action)."""
    return {k: batch_space(v, n) for k, v in space.items()} if isinstance(space, dict) else batch_space(space, n)


def checked_seed(seed, num_envs, env_index0, bits):
    """What reset(seed=...) hands to the C ABI: a Python int (the base: env i gets seed + env_index0 + i) or a uint64 array of
    `num_envs` per-env seeds.  `bits` is the width of the type's generator seed: 32 where a NumPy legacy stream is seeded
    (np.random.seed raises "Seed must be between 0 and 2**32 - 1" above it), 64 elsewhere (CPython's random.seed and NumPy's
    SeedSequence take a third 32-bit limb from 2**64 on, which the kernels do not implement).  Every env's seed must lie in
    [0, 2**bits - 1]: ValueError otherwise, for a base through its LAST env, with the reference's words for 32 bits.  A sequence
    must hold integers: an array of float or bool dtype, or a list holding a float or a bool, is a TypeError, never a cast."""
    limit = (1 << bits) - 1
    text = f"Seed must be between 0 and 2**{bits} - 1"
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, (bool, np.bool_)):
        seed = int(seed)
        last = seed + int(env_index0) + int(num_envs) - 1
        if seed < 0 or last > limit:
            raise ValueError(f"{text}: seed {seed} gives env {int(num_envs) - 1} of this batch (env_index0 {int(env_index0)}) the seed {last}")
        return seed
    if isinstance(seed, torch.Tensor):
        seed = seed.cpu().numpy()
    if isinstance(seed, np.ndarray) and seed.dtype != object:
        if seed.dtype.kind not in "iu":
            raise TypeError(f"seed sequence must hold integers, not {seed.dtype}")
        arr = seed
    else:
        arr = np.empty(len(seed), dtype=object)
        for i, s in enumerate(seed):
            if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)):
                raise TypeError(f"seed sequence must hold integers, not {type(s).__name__} (item {i})")
            arr[i] = int(s)
    if arr.shape != (int(num_envs),):
        raise ValueError(f"seed sequence must hold {int(num_envs)} ints, got shape {arr.shape}")
    lo, hi = int(arr.min()), int(arr.max())
    if lo < 0 or hi > limit:
        raise ValueError(f"{text}: the seed sequence holds {lo if lo < 0 else hi}")
    return np.ascontiguousarray(arr.astype(np.uint64))


TERMINATED, TRUNCATED, BOTH, TERMINATED_AT_LIMIT = "terminated", "truncated", "both", "terminated_at_limit"
_RECORD_CALLS = ("state_bytes", "get_state", "set_state", "pack", "unpack")


class DeviceVectorEnv(VectorEnvBase):
    """Base of every batched env: owns the native handle, the device and the output buffers, and holds the ONLY reset() / step() /
    rollout() / info() / get_state() / set_state().  An env type declares what differs through the class attributes below and
    `_obs_shape` (the shape of one observation buffer, set in __init__), and writes none of them; DESIGN.md §1 "One façade" has the
    table of variants.  `_flags` names the flag the type raises and with it the tensor that means "done": TERMINATED (`truncated` is
    NULL for the kernel and one shared all-False tensor for the caller; done = terminated), TRUNCATED (bus: both written,
    done = truncated), BOTH (done = the `done_mask` buffer the step kernel fills; a rollout's per-step flags are uint8
    terminated | truncated << 1 instead of bool) or TERMINATED_AT_LIMIT (space station: both written, `truncated` only ever together
    with `terminated`, so done = terminated and a rollout's per-step flags are the bool `terminated`)."""

    _abi = None  # e.g. "cge_snake"
    _seed_bits = 64   # the width of a per-env seed (checked_seed): 32 for the types that seed a NumPy legacy stream
    INFO_FIELDS = {}
    INFO64_FIELDS = {}
    _obs_dtype = torch.float32
    _action_shape, _action_dtype, _action_ptrs = (), torch.int32, 1
    _flags = TERMINATED
    _reward_sum_dtype = torch.float64
    _info_dtype, _info_indexed = torch.float64, False
    _invalid_action_text = None   # check_actions(): the ValueError text of a type with an error counter, with {n} = the count

    def _init_common(self, num_envs, device, autoreset_mode, env_index0, reuse_buffers):
        if int(num_envs) <= 0:
            raise ValueError("num_envs must be positive")
        self.num_envs = int(num_envs)
        self.env_index0 = int(env_index0)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _native.NativeLibraryError(
                f"{type(self).__name__} runs only on an MI355X (device 'cuda:N' under PyTorch-ROCm); got {device!r}. "
                "There is no CPU path.")
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("no HIP device is visible to PyTorch; there is no CPU path")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self._dev_index)
        self.autoreset_mode = parse_autoreset_mode(autoreset_mode)
        self._mode_code = _MODE_CODE[self.autoreset_mode.name]
        self.metadata = dict(getattr(type(self), "metadata", {}), autoreset_mode=self.autoreset_mode)
        self._reuse = bool(reuse_buffers)
        self._lib = _native.lib()
        self._h = None
        self._bufs = {}
        self._ep_ret = self._ep_len = None
        self._done_ptr = 0
        self._last_obs = None
        self.closed = False

    def _create(self, cfg, info_fields, record_episode_statistics, reference_info):
        """The tail of every constructor, after the type has set its spaces and `_obs_shape`: create the native handle, bind the
        entry points the hot path calls, batch the spaces; `info_fields` is validated first."""
        known = {**self.INFO_FIELDS, **self.INFO64_FIELDS}
        for f in info_fields:                                      # before create: a misspelt field allocates nothing
            if f not in known:
                raise ValueError(f"unknown info field {f!r}; choose from {sorted(known)}")
        h = C.c_void_p()
        status = self._fn("create")(C.byref(cfg), self.num_envs, self._dev_index, self.env_index0, C.byref(h))
        if status:
            error = self._create_error(status)
            if error is not None:
                raise error
        _native.check(status, what=f"{self._abi}_create")
        self._h = h
        # bound once: step() / reset() / rollout() / info() do no string formatting and no getattr by name
        self._c_reset, self._c_step, self._c_rollout, self._c_info, self._c_done_mask, self._c_last_error, self._c_seed = (
            getattr(self._lib, f"{self._abi}_{name}", None) for name in ("reset", "step", "rollout", "info", "done_mask", "last_error", "seed"))
        self._obs_stride = int(np.prod(self._obs_shape))
        self._actions_shape = (self.num_envs,) + tuple(self._action_shape)
        self._reference_info = bool(reference_info)
        self.action_space = _batch(self.single_action_space, self.num_envs)
        self.observation_space = _batch(self.single_observation_space, self.num_envs)
        self.info_fields = tuple(info_fields)
        self.record_episode_statistics(record_episode_statistics)

    def _create_error(self, status):
        """The exception a failing create raises instead of the generic NativeLibraryError, or None."""
        return None

    # ------------------------------------------------------------------ native helpers
    def _fn(self, name):
        if name in ("rollout_final_obs", "final_obs_segment") and not hasattr(self._lib, f"{self._abi}_{name}"):
            return getattr(self._lib, f"cge_rows_{self._abi[4:]}_{name}")      # the lane-per-env types but airline: cge_rows_<env>_* (cge_amd.h)
        if name in _RECORD_CALLS and not hasattr(self._lib, f"{self._abi}_{name}"):
            return getattr(self._lib, f"cge_records_{self._abi[4:]}_{name}")   # the record-lane types: cge_records_<env>_* (cge_amd.h)
        return getattr(self._lib, f"{self._abi}_{name}")

    def _check(self, status, what):
        if status:                                             # hot path: no lookups or string formatting on success
            _native.check(status, self._h, self._c_last_error, f"{self._abi}_{what}")

    def _stream(self):
        # the raw handle of torch's current stream on this device (the private getter skips building a Stream object: ~2 us per call
        # on the step() path, where a kernel is 30-40 us)
        get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        return get(self._dev_index) if get is not None else torch.cuda.current_stream(self.device).cuda_stream

    def _out(self, key, shape, dtype):
        """Output tensor: a fresh allocation per call (gymnasium's `copy=True` contract) or, with
        reuse_buffers=True, one persistent buffer per output that the next call overwrites."""
        if self._reuse:
            t = self._bufs.get(key)
            if t is not None and tuple(t.shape) == tuple(shape) and t.dtype == dtype:
                return t
            numel = int(np.prod(shape))
            if t is None or t.dtype != dtype or t.numel() < numel:           # first use, or a larger request (e.g. a longer rollout)
                t = self._bufs[key] = torch.empty(shape, dtype=dtype, device=self.device)
                return t
            return t.view(-1)[:numel].view(shape)                            # a shorter rollout reuses the front of the buffer
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _as_device(self, x, dtype, shape, what):
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.device, dtype=dtype, non_blocking=True)
        else:
            t = torch.as_tensor(np.asarray(x), device=self.device).to(dtype)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    def _seed_native(self, seed):
        """seed: None (streams continue), int (env i gets seed + env_index0 + i) or a per-env sequence.  `checked_seed` refuses
        what the reference's generator refuses before anything native is called: a refused seed changes nothing."""
        if seed is None:
            return
        seed = checked_seed(seed, self.num_envs, self.env_index0, self._seed_bits)
        if isinstance(seed, int):
            self._check(self._c_seed(self._h, None, seed, self._stream()), "seed")
            return
        t = torch.from_numpy(seed.view(np.int64)).to(self.device)
        self._check(self._c_seed(self._h, t.data_ptr(), 0, self._stream()), "seed")
        self._keepalive = t

    def device_bytes(self):
        return int(self._fn("device_bytes")(self._h))

    def action_sampler(self, seed=None, dtype=None):
        """A DeviceSpaceSampler over this batch's `action_space` (sampling.py): `env.step(env.action_sampler(0).sample())` is
        `env.step(env.action_space.sample())` for an action_space seeded with 0, as one sampling launch plus the step launch.  Its
        output is what step() takes with no conversion (int32 for the discrete kinds).  A shard of `make_sharded` samples its
        slice of the whole batch's stream."""
        from .sampling import DeviceSpaceSampler
        space = self.action_space
        if dtype is None and hasattr(space, "nvec"):
            dtype = torch.int32
        return DeviceSpaceSampler(space, self.device, seed=seed, env_index0=self.env_index0,
                                  global_num_envs=getattr(self, "global_num_envs", None), dtype=dtype)

    def invalid_action_count(self):
        """Synchronises; number of env-steps since the last call whose action the kernel reported instead of acting on (what counts
        is the type's: see its `_invalid_action_text`).  Reading clears the counter.  Only the types that export
        `<abi>_error_count` have one (snake, bus, world builder, restaurant, airline, emergency, space station, farm); for the others this is an AttributeError."""
        return int(self._fn("error_count")(self._h, self._stream()))

    def check_actions(self):
        """Raises the reference's ValueError if `invalid_action_count()` is not zero."""
        n = self.invalid_action_count()
        assert self._invalid_action_text is not None, f"{type(self).__name__} has an error counter but no _invalid_action_text"
        if n:
            raise ValueError(self._invalid_action_text.format(n=n))

    def last_kernel(self):
        """Name(s) of the kernel(s) the last step() / rollout() launched, as rocprofv3 prints them ("" before the first call)."""
        raw = self._fn("last_kernel")(self._h)
        return raw.decode() if raw else ""

    # ------------------------------------------------------------------ gymnasium API
    # hooks; None = the plain case, which the hot path then handles without a call
    _device_actions = None    # (actions, k=None) -> the tuple of device tensors whose pointers the C call takes (climate: ac_temp, lights;
                              # restaurant: its Dict action packed into one tensor)
    _wrap_obs = None          # an observation buffer -> what the caller sees (bus: its dict of views)

    def reset(self, *, seed=None, options=None):
        """Reset every env (or those in options['reset_mask']).  Returns (obs, infos)."""
        self._seed_native(seed)
        mask = None
        if options and options.get("reset_mask") is not None:
            mask = self._as_device(options["reset_mask"], torch.uint8, (self.num_envs,), "reset_mask")
        obs = self._last_obs = self._out("obs", self._obs_shape, self._obs_dtype)
        self._check(self._c_reset(self._h, mask.data_ptr() if mask is not None else None, obs.data_ptr(), self._stream()), "reset")
        return (obs if self._wrap_obs is None else self._wrap_obs(obs)), self._infos()

    def step(self, actions):
        split = self._device_actions
        a = self._as_device(actions, self._action_dtype, self._actions_shape, "actions") if split is None else split(actions)
        obs = self._last_obs = self._out("obs", self._obs_shape, self._obs_dtype)
        rew = self._out("reward", (self.num_envs,), torch.float32)
        term = self._out("terminated", (self.num_envs,), torch.bool)
        same = self._mode_code == _native.AUTORESET_SAME_STEP
        fin = self._out("final_obs", self._obs_shape, self._obs_dtype) if same else None
        if self._flags == TERMINATED:
            # the reference never truncates: one shared all-False tensor, never rewritten (also without reuse_buffers)
            trunc = self._bufs.get("_truncated")
            if trunc is None:
                trunc = self._bufs["_truncated"] = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            trunc_ptr, done = None, term
        else:
            trunc = done = self._out("truncated", (self.num_envs,), torch.bool)
            trunc_ptr = trunc.data_ptr()
            if self._flags == TERMINATED_AT_LIMIT:
                done = term
            elif self._flags == BOTH:
                done = None
                if same or self._ep_ret is not None:               # terminated | truncated, written by the step kernel itself
                    done = self._out("done", (self.num_envs,), torch.bool)
                    if done.data_ptr() != self._done_ptr:
                        self._done_ptr = done.data_ptr()
                        self._check(self._c_done_mask(self._h, self._done_ptr), "done_mask")
                elif self._done_ptr:
                    self._done_ptr = 0
                    self._check(self._c_done_mask(self._h, None), "done_mask")
        fin_ptr = fin.data_ptr() if same else None
        if split is None:                                          # spelled out, not splatted: ~0.5 us per call on a 10 us step
            status = self._c_step(self._h, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc_ptr, fin_ptr, self._stream())
        elif self._action_ptrs == 1:                               # restaurant: the hook packs a mapping into the one tensor the C call takes
            status = self._c_step(self._h, a[0].data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc_ptr, fin_ptr, self._stream())
        else:
            status = self._c_step(self._h, a[0].data_ptr(), a[1].data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc_ptr,
                                  fin_ptr, self._stream())
        self._check(status, "step")
        infos = self._infos()
        wrap = self._wrap_obs
        if same:
            # rows of final_obs are valid where _final_obs is True (gymnasium's SAME_STEP convention)
            infos["final_obs"] = fin if wrap is None else wrap(fin)
            infos["_final_obs"] = done
        return (obs if wrap is None else wrap(obs)), rew, term, trunc, self._episode_infos(infos, done)

    def rollout(self, k_steps, actions=None, action_seed=0, t0=0, trajectory=False, want_obs=True, per_step=False):
        """k fused step()s queued by one C-ABI call (state stays in registers between steps).  actions: None -> counter-hash
        random actions (cge_hash_action) or what step() takes with a leading [k].  Returns (obs, reward_sum, done_count) with obs
        [k, N, ...] if trajectory else the last step's [N, ...] (None with want_obs=False); with per_step=True
        (obs, reward[k, N], flags[k, N], reward_sum, done_count) — the outputs of k step() calls, where flags is the bool flag the
        type raises (terminated; bus: truncated) or, for the types that raise both, uint8 terminated | truncated << 1.
        reward_sum is float64 (snake: float32).  A SAME_STEP trajectory holds the reset observation at a step that ends an episode,
        as step()'s `obs` does."""
        k = int(k_steps)
        a = ()                                                     # the tensors are held until the launch is queued
        if actions is not None and self._device_actions is None:
            a = (self._as_device(actions, self._action_dtype, (k,) + self._actions_shape, "actions"),)
        elif actions is not None:
            a = self._device_actions(actions, k)
        a_ptrs = [t.data_ptr() for t in a] or [None] * self._action_ptrs
        obs, stride = None, 0
        if want_obs:
            if trajectory:
                obs = self._out("traj", (k,) + self._obs_shape, self._obs_dtype)
                stride = self._obs_stride
            else:
                obs = self._out("obs", self._obs_shape, self._obs_dtype)
        rs = self._out("reward_sum", (self.num_envs,), self._reward_sum_dtype)
        dc = self._out("done_count", (self.num_envs,), torch.int32)
        rt = ft = None
        if per_step:
            rt = self._out("reward_traj", (k, self.num_envs), torch.float32)
            ft = self._out("flags_traj", (k, self.num_envs), torch.uint8 if self._flags == BOTH else torch.bool)
        self._check(self._c_rollout(self._h, k, *a_ptrs, int(action_seed), int(t0), obs.data_ptr() if obs is not None else None, stride,
                                    rt.data_ptr() if per_step else None, ft.data_ptr() if per_step else None,
                                    rs.data_ptr(), dc.data_ptr(), self._stream()), "rollout")
        if obs is not None and self._wrap_obs is not None:
            obs = self._wrap_obs(obs)
        return (obs, rt, ft, rs, dc) if per_step else (obs, rs, dc)

    def info(self, field, index=0):
        """One field of INFO_FIELDS for every env; `index` selects the item of a per-item field where the type has those."""
        if index and not self._info_indexed:
            raise TypeError(f"{type(self).__name__}.info() takes no index")
        out = torch.empty(self.num_envs, dtype=self._info_dtype, device=self.device)
        at = (int(index),) if self._info_indexed else ()
        self._check(self._c_info(self._h, self.INFO_FIELDS[field], *at, out.data_ptr(), self._stream()), "info")
        return out

    def _infos(self):
        d = {f: self.info(f) for f in self.info_fields}
        if self._reference_info:
            d.update(self.reference_info())
        return d

    def reference_info(self):
        """The reference's own `info` dict (its keys, its derived expressions) as tensors; subclasses define it."""
        raise NotImplementedError

    def _device_records(self):
        """Does the type pack its records on the device (airline, emergency, space station, farm: cge_records_<env>_*)?"""
        return hasattr(self._lib, f"cge_records_{self._abi[4:]}_pack")

    def _record_range(self, first, count):
        first = int(first)
        if first < 0 or first + count > self.num_envs:
            raise ValueError(f"envs [{first}, {first + count}) are not within [0, {self.num_envs})")
        return first

    def _record_call(self, name, fn, *args):
        """A records call whose refusal of its input (CGE_ERR_INVALID_ARG: a record the check refuses) is a ValueError with the
        library's text, which names the env."""
        status = fn(self._h, *args, self._stream())
        if status == -1 and self._device_records():
            raw = self._c_last_error(self._h)
            raise ValueError(raw.decode() if raw else f"{self._abi}_{name}: invalid argument")
        self._check(status, name)

    def get_state(self, out=None, first=0):
        """Canonical per-env state records, uint8 [N, state_bytes] on the host (snake, crypto, traffic, world builder, and airline,
        emergency, space station, farm; the others: `snapshot()`).  The last four pack their records on the device: with `out` a
        contiguous CUDA uint8 tensor [M, state_bytes] the records of envs [first, first + M) are packed into it, with
        `out="device"` into a new tensor of envs [first, N), and that tensor is returned — nothing passes through the host.
        `set_state` checks every record before it writes one: a refused buffer leaves the batch as it was."""
        rec = int(self._fn("state_bytes")(self._h))
        if out is None and not first:
            buf = np.zeros((self.num_envs, rec), np.uint8)
            self._check(self._fn("get_state")(self._h, buf.ctypes.data, self._stream()), "get_state")
            return buf
        if not self._device_records():
            raise NotImplementedError(f"{self._abi}: records on the device and sub-ranges are for the types that pack them there")
        if isinstance(out, torch.Tensor):
            t = out
        elif out is None or out == "device":                       # None with `first`: envs [first, N) on the host
            first = self._record_range(first, 0)
            t = torch.empty((self.num_envs - first, rec), dtype=torch.uint8, device=self.device)
        else:
            raise ValueError('out must be a CUDA uint8 tensor, "device" or None')
        self._check_records(t, rec)
        first = self._record_range(first, t.shape[0])
        self._record_call("pack", self._fn("pack"), first, t.shape[0], t.data_ptr())
        return t if out is not None else t.cpu().numpy()

    def _check_records(self, t, rec):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] == rec):
            raise ValueError(f"records must be a uint8 tensor [M, {rec}]")
        if t.device != self.device:
            raise ValueError(f"records must be on {self.device}, got {t.device}")
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("records must be contiguous and 16-byte aligned")

    def set_state(self, buf, first=0):
        """Takes what `get_state` returns: a host array of all N records, or (the four types that pack on the device) a CUDA uint8
        tensor [M, state_bytes] for envs [first, first + M); a host array with `first` goes through such a tensor."""
        rec = int(self._fn("state_bytes")(self._h))
        if isinstance(buf, torch.Tensor) and buf.device.type == "cuda" or first:
            if not self._device_records():
                raise NotImplementedError(f"{self._abi}: records on the device and sub-ranges are for the types that pack them there")
            if not (isinstance(buf, torch.Tensor) and buf.device.type == "cuda"):
                host = np.ascontiguousarray(buf, dtype=np.uint8)
                if host.ndim != 2 or host.shape[1] != rec:
                    raise ValueError(f"state buffer must be uint8 [M, {rec}]")
                buf = torch.from_numpy(host).to(self.device)
            self._check_records(buf, rec)
            first = self._record_range(first, buf.shape[0])
            self._record_call("unpack", self._fn("unpack"), first, buf.shape[0], buf.data_ptr())
            return
        if isinstance(buf, torch.Tensor):
            buf = buf.numpy()
        if not (isinstance(buf, np.ndarray) and buf.dtype == np.uint8) and self._device_records():
            raise ValueError(f"state buffer must be uint8 {(self.num_envs, rec)}")
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        if buf.shape != (self.num_envs, rec):
            raise ValueError(f"state buffer must be uint8 {(self.num_envs, rec)}")
        self._record_call("set_state", self._fn("set_state"), buf.ctypes.data)

    # ------------------------------------------------------------------ episode statistics
    def record_episode_statistics(self, enable=True):
        """What gymnasium.wrappers.vector.RecordEpisodeStatistics adds around a vector env, computed by the step kernel itself:
        with it enabled every step()'s infos carries `episode = {"r": float64[N], "l": int32[N]}` and the mask `_episode`
        (= terminated | truncated); r / l of env i are the return (float64 sum of the episode's rewards in step order) and
        the length in env steps of the episode that just ended — the numbers the reference's RLlib scripts report as
        episode_return_mean / episode_len_mean (smart_parking_env/examples/training.py:55).  Entries where `_episode` is False
        keep the env's previous episode.  Enable it before the episode starts (constructor flag or before reset())."""
        if enable:
            self._ep_ret = torch.zeros(self.num_envs, dtype=torch.float64, device=self.device)
            self._ep_len = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self._check(self._fn("episode_stats")(self._h, self._ep_ret.data_ptr(), self._ep_len.data_ptr()), "episode_stats")
        elif getattr(self, "_ep_ret", None) is not None:
            torch.cuda.current_stream(self.device).synchronize()          # no kernel may still be writing the buffers
            self._check(self._fn("episode_stats")(self._h, None, None), "episode_stats")
            self._ep_ret = self._ep_len = None
        else:
            self._ep_ret = self._ep_len = None

    def episode_statistics(self):
        """(return float64[N], length int32[N]) of each env's last finished episode (also after a rollout()), or None."""
        return None if self._ep_ret is None else (self._ep_ret, self._ep_len)

    def _episode_infos(self, infos, done):
        if self._ep_ret is not None:
            infos["episode"] = {"r": self._ep_ret, "l": self._ep_len}
            infos["_episode"] = done
        return infos

    # ------------------------------------------------------------------ terminal observations of fused SAME_STEP rollouts
    def collect_final_obs(self, rows_per_env=4):
        """A SAME_STEP `rollout()` writes the RESET observation of an env that finishes at step t to slot t of its trajectory —
        what `step()` returns as `obs`; the terminal observation, which `step()` hands over as `infos["final_obs"]` (and the
        reference's own step() returns), goes to a side output once this is enabled.  The rows are compacted per segment of S
        consecutive envs (the envs one wavefront steps: `self.final_obs_segment`); a segment holds S * rows_per_env rows per rollout
        call — size it for the episodes a rollout can end (`final_obs_dropped()` says whether it was enough).  Read the rows back with
        `final_obs()`; `rows_per_env=0` disables the output again."""
        seg = self.final_obs_segment = int(self._fn("final_obs_segment")(self._h))
        if rows_per_env <= 0:
            torch.cuda.current_stream(self.device).synchronize()
            self._check(self._fn("rollout_final_obs")(self._h, None, None, 0, None), "rollout_final_obs")
            self._fin = None
            return
        nseg, cap = -(-self.num_envs // seg), int(seg * rows_per_env)
        rows = torch.empty((nseg * cap,) + tuple(self._obs_shape[1:]), dtype=self._obs_dtype, device=self.device)
        index = torch.empty(nseg * cap, dtype=torch.int64, device=self.device)
        count = torch.zeros(nseg, dtype=torch.int32, device=self.device)
        self._check(self._fn("rollout_final_obs")(self._h, rows.data_ptr(), index.data_ptr(), cap, count.data_ptr()), "rollout_final_obs")
        self._fin = (rows, index, count, cap)

    def _fin_buffers(self):
        fin = getattr(self, "_fin", None)
        if fin is None:
            raise RuntimeError(f"{type(self).__name__}: no terminal-row output is registered; call collect_final_obs(rows_per_env > 0) "
                               "before rollout() and final_obs()")
        return fin

    def final_obs(self):
        """(rows [m, *obs_shape], step [m], env [m]) delivered by the last rollout(), sorted by (step, env): row j is the terminal
        observation of env[j] at step step[j] of that call.  Gathers the segments' rows on the device (boolean indexing: synchronises)."""
        rows, index, count, cap = self._fin_buffers()
        nseg = count.shape[0]
        keep = (torch.arange(cap, device=self.device)[None, :] < count.clamp(max=cap)[:, None]).reshape(-1)
        idx = index[keep]
        order = torch.argsort(idx)
        idx = idx[order]
        return rows[keep][order], idx // self.num_envs, idx % self.num_envs

    def final_obs_dropped(self):
        """Terminal rows the last rollout() produced but could not store (its segments were full); synchronises."""
        rows, _, count, cap = self._fin_buffers()
        return int((count - cap).clamp(min=0).sum().item())

    def snapshot(self):
        """Whole-batch checkpoint as an opaque uint8 array (env types without a canonical per-env `get_state` record).
        Restores only into an env created with the same num_envs and config; synchronises the stream."""
        if not hasattr(self._lib, f"{self._abi}_snapshot_bytes"):
            raise NotImplementedError(f"{self._abi}: use get_state()/set_state()")
        import numpy as np
        buf = np.zeros(int(self._fn("snapshot_bytes")(self._h)), np.uint8)
        self._check(self._fn("snapshot_get")(self._h, buf.ctypes.data, self._stream()), "snapshot_get")
        return buf

    def restore(self, buf):
        import numpy as np
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        if buf.shape != (int(self._fn("snapshot_bytes")(self._h)),):
            raise ValueError("not a snapshot of an env of this type and size")
        self._check(self._fn("snapshot_set")(self._h, buf.ctypes.data, self._stream()), "snapshot_set")

    def close_extras(self, **kwargs):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None
