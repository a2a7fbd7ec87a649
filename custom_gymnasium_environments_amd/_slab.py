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

    # ------------------------------------------------------------------ terminal observations of fused SAME_STEP rollouts
    # The compacted rows are a slab too: the type's ordinary observation slab for R = segments * capacity "envs", row j of segment s
    # being env s * capacity + j of it (include/cge_amd.h).  A type without a slab (world builder's flatten_obs) has the base class's rows.
    def _rows_layout(self, num_rows):
        """(the plane table, slab elements) of this type's observation slab for `num_rows` envs."""
        raise NotImplementedError

    def collect_final_obs(self, rows_per_env=4):
        if rows_per_env <= 0 or getattr(self, "_planes", None) is None:
            self._fin_planes = None
            return super().collect_final_obs(rows_per_env)
        seg = self.final_obs_segment = int(self._fn("final_obs_segment")(self._h))
        nseg, cap = -(-self.num_envs // seg), int(seg * rows_per_env)
        planes, elems = self._rows_layout(nseg * cap)
        rows = torch.empty(elems, dtype=self._obs_dtype, device=self.device)
        index = torch.empty(nseg * cap, dtype=torch.int64, device=self.device)
        count = torch.zeros(nseg, dtype=torch.int32, device=self.device)
        self._check(self._fn("rollout_final_obs")(self._h, rows.data_ptr(), index.data_ptr(), cap, count.data_ptr()), "rollout_final_obs")
        self._fin, self._fin_planes = (rows, index, count, cap), planes

    collect_final_obs.__doc__ = DeviceVectorEnv.collect_final_obs.__doc__

    def final_obs(self):
        """(rows, step [m], env [m]) delivered by the last rollout(), sorted by (step, env): `rows` is a dict {key: tensor [m, ...]} in
        the keys' dtypes and gymnasium's batched-Dict shapes, and rows[key][j] belongs to the terminal observation of env[j] at step
        step[j] of that call.  Gathers the segments' rows on the device (boolean indexing: synchronises)."""
        rows, index, count, cap = self._fin_buffers()
        if getattr(self, "_fin_planes", None) is None:
            return super().final_obs()
        keep = (torch.arange(cap, device=rows.device)[None, :] < count.clamp(max=cap)[:, None]).reshape(-1)
        idx = index[keep]
        order = torch.argsort(idx)
        idx = idx[order]
        return gather_rows(rows, keep, order, self._fin_planes), idx // self.num_envs, idx % self.num_envs


def gather_rows(slab, keep, order, planes):
    """The rows `keep` (bool [R]) of every plane of a rows slab for R = keep.numel() envs, permuted by `order`: {key: tensor [m, ...]}."""
    return {key: v[keep][order] for key, v in plane_views(slab, keep.numel(), planes).items()}
