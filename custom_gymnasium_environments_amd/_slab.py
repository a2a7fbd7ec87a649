"""Key-major observation slabs: the ONE buffer a lane-per-env kernel (bus, world builder, restaurant) writes plane by plane, and the dict
of per-key views of it that the caller sees — gymnasium's batched-Dict layout, with no copy.

A plane is (key, per-env shape, torch dtype, offset in slab elements).  Bus and restaurant slabs are int32 with the planes packed
(`packed_planes`); world builder's is a uint8 slab of typed planes that each start at a multiple of 16 bytes (its `slab_layout`)."""
import numpy as np
import torch

from .vector_env import DeviceVectorEnv


def packed_planes(planes, num_envs, dtype=torch.int32):
    """(key, per-env shape) planes of one dtype, back to back -> (the plane table, slab elements)."""
    table, o = [], 0
    for key, shape in planes:
        table.append((key, tuple(shape), dtype, o))
        o += num_envs * int(np.prod(shape))
    return tuple(table), o


def plane_views(slab, num_envs, planes):
    """slab [slab_elems] or [k, slab_elems] -> {key: view [N, ...] or [k, N, ...]} in the planes' dtypes.  Works on any device."""
    lead, size, d = slab.shape[:-1], slab.element_size(), {}
    for key, shape, dtype, off in planes:
        w = num_envs * int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size() // size
        v = slab[..., off:off + w]
        d[key] = (v if dtype == slab.dtype else v.view(dtype)).view(lead + (num_envs,) + tuple(shape))
    return d


def slab_of(obs, planes, slab_elems, dtype):
    """The slab ([slab_elems], or [k, slab_elems] for a trajectory) behind a dict of `plane_views`: the first plane starts it."""
    key, shape, _, off = planes[0]
    assert off == 0
    first = obs[key].view(dtype)
    lead = first.shape[:first.dim() - 1 - len(shape)]
    return torch.as_strided(first, lead + (slab_elems,), tuple(first.stride()[:len(lead)]) + (1,), first.storage_offset())


class SlabVectorEnv(DeviceVectorEnv):
    """A DeviceVectorEnv whose observation buffer is one flat slab per step, handed out as a dict of views.  The type calls
    `_init_slab` in its constructor, before `_create`."""

    def _init_slab(self, planes, slab_elems, dtype):
        self._planes, self._slab, self._obs_dtype = tuple(planes), int(slab_elems), dtype
        self._obs_shape = (self._slab,)                                  # one flat slab per step, not [N, ...]
        self._views = {}

    def _dict(self, slab):
        """slab [slab_elems] or [k, slab_elems] -> {key: view [N, ...] or [k, N, ...]}.  The dict of a persistent buffer is built once."""
        key = (slab.data_ptr(), tuple(slab.shape)) if self._reuse else None
        d = self._views.get(key) if key is not None else None
        if d is None:
            d = plane_views(slab, self.num_envs, self._planes)
            if key is not None:
                self._views = {k: v for k, v in self._views.items() if k[0] != key[0]}       # a regrown buffer drops its old views
                self._views[key] = d
        return dict(d)

    _wrap_obs = _dict

    def obs_slab(self, obs):
        """The flat slab ([slab_elems], or [k, slab_elems] for a trajectory) behind an observation dict of this env."""
        return slab_of(obs, self._planes, self._slab, self._obs_dtype)
