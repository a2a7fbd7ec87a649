"""`action_space.sample()` of a batched space on the device, bit for bit what NumPy draws.

Every reference script drives its env with `env.action_space.sample()` (snake_env_classic/example.py:23, traffic_management_env/demo.py:49,
...); the gymnasium vector form is `envs.step(envs.action_space.sample())`.  On the host that is a NumPy draw plus an upload per step.
`DeviceSpaceSampler` owns the same NumPy PCG64 stream a space seeded with `np.random.default_rng(seed)` owns and writes, from one
HIP launch (csrc/sample.hip), exactly what that space's successive `sample()` calls return (gymnasium 1.x):

  MultiDiscrete (batched Discrete)   one random() per element, C order: int(trunc(u * nvec[col]))
  bounded float Box                  one random() per element: float32(low + (high - low) * u)   (Generator.uniform)
  bounded integer Box                one random() per element: floor(low + ((high + 1) - low) * u)   (gymnasium's integer path)
  MultiBinary                        Generator.integers(0, 2, dtype=int8): bytes of 32-bit words, the buffered half carried over
  Dict / a plain mapping of these    one stream per subspace, keys in sorted order; seed(int s) seeds subspace j with
                                     default_rng(s).integers(2**31 - 1, size=len(keys))[j]

The stream is advanced on the device inside the same launch: no host synchronisation, and `sample(out=...)` can be captured in a
HIP graph.  `state` is NumPy's `bit_generator.state` (get and set synchronise), so a host generator and the sampler can hand the
stream back and forth.  Spaces whose sample() takes a variable number of draws (unbounded Box components, Lemire rejection) are
refused with NotImplementedError.
"""
import ctypes as C
from collections.abc import Mapping

import numpy as np
import torch

from . import _native

_ABI_DTYPE = {torch.int8: _native.DTYPE_INT8, torch.int32: _native.DTYPE_INT32, torch.int64: _native.DTYPE_INT64,
              torch.float32: _native.DTYPE_FLOAT32}
_TORCH_DTYPE = {np.dtype(np.int8): torch.int8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
                np.dtype(np.float32): torch.float32}
_M64 = (1 << 64) - 1


class _Leaf:
    """One non-mapping batched space: kind, k columns, per-column params, rows, output dtype (host-side checks only)."""

    def __init__(self, space, dtype):
        shape = tuple(int(v) for v in (getattr(space, "shape", None) or ()))
        if len(shape) not in (1, 2) or shape[0] < 1 or (len(shape) == 2 and shape[1] < 1):
            raise ValueError(f"{space}: a batched space of shape (num_envs,) or (num_envs, k) is expected")
        self.shape, self.rows = shape, shape[0]
        self.k = shape[1] if len(shape) == 2 else 1
        if self.k > _native.SAMPLER_MAX_K:
            raise ValueError(f"{space}: at most {_native.SAMPLER_MAX_K} columns")
        dtype = None if dtype is None else torch.empty(0, dtype=dtype).dtype
        if hasattr(space, "nvec"):                                            # MultiDiscrete
            if np.any(np.asarray(getattr(space, "start", 0)) != 0):
                raise NotImplementedError(f"{space}: MultiDiscrete with a non-zero start")
            nvec = np.asarray(space.nvec, dtype=np.int64).reshape(self.rows, self.k)
            if np.any(nvec < 1):
                raise ValueError(f"{space}: nvec must be >= 1")
            if np.any(nvec != nvec[:1]):
                raise ValueError(f"{space}: nvec must be one row broadcast over the envs")
            self.kind, self.params = _native.SAMPLE_INDEX, nvec[0].astype(np.float64)
            self.dtype = dtype or torch.int64
            if self.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{space}: samples as int32 or int64, not {self.dtype}")
            if self.dtype == torch.int32 and nvec.max() > 2**31:
                raise ValueError(f"{space}: nvec too large for int32")
        elif hasattr(space, "low") and hasattr(space, "high"):                # Box
            low = np.broadcast_to(np.asarray(space.low, dtype=np.float64), shape).reshape(self.rows, self.k)
            high = np.broadcast_to(np.asarray(space.high, dtype=np.float64), shape).reshape(self.rows, self.k)
            if not (np.all(np.isfinite(low)) and np.all(np.isfinite(high))):
                raise NotImplementedError(f"{space}: unbounded Box components draw a variable number of values")
            if np.any(low != low[:1]) or np.any(high != high[:1]):
                raise ValueError(f"{space}: bounds must be one row broadcast over the envs")
            if np.any(low > high):
                raise ValueError(f"{space}: low > high")
            sdt = np.dtype(space.dtype)
            self.kind, self.params = _native.SAMPLE_UNIFORM, np.concatenate([low[0], high[0]])
            if sdt.kind == "f":
                if sdt != np.float32:
                    raise NotImplementedError(f"{space}: float Boxes sample as float32 only")
                self.dtype = dtype or torch.float32
                if self.dtype != torch.float32:
                    raise ValueError(f"{space}: a float Box samples as float32")
            elif sdt.kind in "iu":
                if np.any(low != np.floor(low)) or np.any(high != np.floor(high)):
                    raise ValueError(f"{space}: integer Box bounds must be whole numbers")
                self.dtype = dtype or _TORCH_DTYPE.get(sdt)
                if self.dtype not in (torch.int8, torch.int32):
                    raise ValueError(f"{space}: an integer Box samples as int8 or int32")
                lim = 128 if self.dtype == torch.int8 else 2**31
                if low.min() < -lim or high.max() > lim - 1:
                    raise ValueError(f"{space}: bounds do not fit {self.dtype}")
            else:
                raise NotImplementedError(f"{space}: Box of dtype {sdt}")
        elif type(space).__name__ == "MultiBinary":
            self.kind, self.params = _native.SAMPLE_BITS, None
            self.dtype = dtype or torch.int8
            if self.dtype != torch.int8:
                raise ValueError(f"{space}: MultiBinary samples as int8")
        else:
            raise NotImplementedError(f"no device sampler for {space!r}")


def _pcg_state(st):
    """NumPy bit_generator.state dict -> cge_pcg64_state."""
    if not isinstance(st, Mapping) or st.get("bit_generator") != "PCG64":
        raise ValueError("expected a PCG64 bit_generator.state dict")
    s, i = int(st["state"]["state"]), int(st["state"]["inc"])
    return _native.Pcg64State(s & _M64, s >> 64, i & _M64, i >> 64, int(st["has_uint32"]), int(st["uinteger"]))


def _np_state(c):
    return {"bit_generator": "PCG64", "state": {"state": c.state_hi << 64 | c.state_lo, "inc": c.inc_hi << 64 | c.inc_lo},
            "has_uint32": int(c.has_uint32), "uinteger": int(c.uinteger)}


class DeviceSpaceSampler:
    """Device twin of `space.sample()` for a batched space (see the module docstring).

    space            the batched space (an env's `action_space`): MultiDiscrete, bounded Box, MultiBinary, or a Dict / mapping of them
    seed             as `space.seed(seed)`: int, None (OS entropy) or, for a mapping, {key: int}
    env_index0, global_num_envs
                     this batch holds rows [env_index0, env_index0 + num_envs) of a world batch of global_num_envs rows: it samples
                     its slice of the world batch's stream, so shards of one batch together sample what the unsplit batch does
    dtype            output torch dtype (a {key: dtype} dict for a mapping); default the space's dtype
    """

    def __init__(self, space, device="cuda:0", seed=None, env_index0=0, global_num_envs=None, dtype=None):
        self.space = space
        if isinstance(space, Mapping):
            keys = list(space.keys()) if type(space).__name__ == "Dict" else sorted(space.keys())
            if not keys:
                raise ValueError("an empty mapping space")
            if dtype is not None and not isinstance(dtype, Mapping):
                raise ValueError("dtype of a mapping space is a {key: dtype} dict")
            self._leaves = {k: _Leaf(space[k], None if dtype is None else dtype.get(k)) for k in keys}
            if len({lf.rows for lf in self._leaves.values()}) != 1:
                raise ValueError("the subspaces of a mapping space must have the same number of envs")
            self._mapping = True
        else:
            if isinstance(dtype, Mapping):
                raise ValueError("dtype of a non-mapping space is one torch dtype")
            self._leaves = {None: _Leaf(space, dtype)}
            self._mapping = False
        self.num_envs = next(iter(self._leaves.values())).rows
        self.env_index0 = int(env_index0)
        self.global_num_envs = self.env_index0 + self.num_envs if global_num_envs is None else int(global_num_envs)
        if self.env_index0 < 0 or self.global_num_envs < self.env_index0 + self.num_envs:
            raise ValueError(f"rows [{self.env_index0}, {self.env_index0 + self.num_envs}) do not fit a world batch of {self.global_num_envs}")
        self._h = {}
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _native.NativeLibraryError(f"DeviceSpaceSampler runs only on an MI355X (device 'cuda:N'); got {device!r}. There is no CPU path.")
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("no HIP device is visible to PyTorch; there is no CPU path")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self._dev_index)
        self._lib = _native.lib()
        for key, lf in self._leaves.items():
            h = C.c_void_p()
            params = None if lf.params is None else np.ascontiguousarray(lf.params, dtype=np.float64)
            ptr = None if params is None else params.ctypes.data_as(C.POINTER(C.c_double))
            _native.check(self._lib.cge_sampler_create(lf.kind, lf.k, ptr, lf.rows, self.env_index0, self.global_num_envs, self._dev_index,
                                                       C.byref(h)), what="cge_sampler_create")
            self._h[key] = h
        self.seed(seed)

    # ------------------------------------------------------------------ stream
    def _stream(self):
        get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        return get(self._dev_index) if get is not None else torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, key, status, what):
        if status:
            _native.check(status, self._h[key], self._lib.cge_sampler_last_error, f"cge_sampler_{what}")

    def _set(self, key, st):
        c = _pcg_state(st)
        self._check(key, self._lib.cge_sampler_set_state(self._h[key], C.byref(c), self._stream()), "set_state")

    def _get(self, key):
        c = _native.Pcg64State()
        self._check(key, self._lib.cge_sampler_get_state(self._h[key], C.byref(c), self._stream()), "get_state")
        return _np_state(c)

    def seed(self, seed=None):
        """Reseed as `space.seed(seed)` does (host-side seed derivation; the device only sees PCG64 states).  Synchronises."""
        if not self._mapping:
            if isinstance(seed, Mapping):
                raise ValueError("a {key: seed} dict seeds a mapping space only")
            self._set(None, np.random.default_rng(seed).bit_generator.state)
            return
        keys = list(self._leaves)
        if isinstance(seed, Mapping):
            if set(seed) - set(keys):
                raise ValueError(f"seed keys {sorted(set(seed) - set(keys))} are not subspaces")
            for k, s in seed.items():
                self._set(k, np.random.default_rng(s).bit_generator.state)
        elif seed is None:
            for k in keys:
                self._set(k, np.random.default_rng(None).bit_generator.state)
        else:
            subs = np.random.default_rng(int(seed)).integers(np.iinfo(np.int32).max, size=len(keys))
            for k, s in zip(keys, subs):
                self._set(k, np.random.default_rng(int(s)).bit_generator.state)

    @property
    def state(self):
        """NumPy's `bit_generator.state` of the stream (a {key: state} dict for a mapping space).  Synchronises."""
        if not self._mapping:
            return self._get(None)
        return {k: self._get(k) for k in self._leaves}

    @state.setter
    def state(self, st):
        if not self._mapping:
            self._set(None, st)
            return
        if not isinstance(st, Mapping) or set(st) - set(self._leaves):
            raise ValueError(f"state of a mapping space is a {{key: state}} dict over {list(self._leaves)}")
        for k, v in st.items():
            self._set(k, v)

    # ------------------------------------------------------------------ sampling
    def _sample_leaf(self, key, out, steps):
        lf = self._leaves[key]
        shape = lf.shape if steps is None else (steps,) + lf.shape
        if out is None:
            out = torch.empty(shape, dtype=lf.dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != lf.dtype or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {lf.dtype} tensor of shape {shape} on {self.device}")
        self._check(key, self._lib.cge_sampler_sample(self._h[key], 1 if steps is None else steps, out.data_ptr(), _ABI_DTYPE[lf.dtype],
                                                      self._stream()), "sample")
        return out

    def sample(self, out=None, steps=None):
        """One `space.sample()` (steps=None: shape of the space) or `steps` successive ones stacked ([steps, *shape], what
        `rollout(actions=...)` takes).  Fresh tensors, or written into `out` (a {key: tensor} dict for a mapping space)."""
        if steps is not None:
            steps = int(steps)
            if not 1 <= steps <= _native.SAMPLER_MAX_STEPS:
                raise ValueError(f"steps must be in [1, {_native.SAMPLER_MAX_STEPS}]")
        if not self._mapping:
            return self._sample_leaf(None, out, steps)
        if out is not None and (not isinstance(out, Mapping) or set(out) != set(self._leaves)):
            raise ValueError(f"out of a mapping space is a {{key: tensor}} dict over {list(self._leaves)}")
        return {k: self._sample_leaf(k, None if out is None else out[k], steps) for k in self._leaves}

    def device_bytes(self):
        return sum(int(self._lib.cge_sampler_device_bytes(h)) for h in self._h.values())

    def last_kernel(self):
        """Kernel(s) the last sample() launched, as rocprofv3 prints them."""
        names = [self._lib.cge_sampler_last_kernel(h) for h in self._h.values()]
        return ",".join(n.decode() for n in names if n)

    def close(self):
        for h in getattr(self, "_h", {}).values():
            if h:
                self._lib.cge_sampler_destroy(h)
        self._h = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
