"""The slab-to-dict view function of the lane-per-env types (custom_gymnasium_environments_amd/_slab.py) on CPU tensors: for the plane
tables of bus, restaurant and world builder, every view is the NumPy reshape of its plane, the views together cover every slab element
exactly once (world builder: except the padding that aligns its planes to 16 bytes), and `slab_of` gives the slab back."""
import numpy as np
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

from custom_gymnasium_environments_amd import _slab, bus, restaurant, world_builder

_NP = {torch.int8: np.int8, torch.int32: np.int32, torch.float32: np.float32, torch.uint8: np.uint8}


def _tables(n):
    yield "bus", _slab.packed_planes(bus.PLANES, n), torch.int32
    yield "restaurant", _slab.packed_planes(restaurant.PLANES, n), torch.int32
    for g in (3, 10):                                         # 9 cells: the grid plane ends off a 16-byte boundary for every n here
        yield f"world_builder{g}", world_builder.plane_table(n, g), torch.uint8


def test_plane_views_are_the_planes_of_the_slab():
    assert bus.OBS_INTS == 56 and restaurant.OBS_INTS == 341
    for n in (1, 3, 65):
        for name, (planes, elems), dtype in _tables(n):
            size = np.dtype(_NP[dtype]).itemsize
            for lead in ((), (2,)):
                what = (name, n, lead)
                count = int(np.prod(lead + (elems,)))
                # distinct values (int32), or bytes that differ between neighbours and between planes (uint8)
                host = np.arange(count, dtype=np.int64) if dtype == torch.int32 else (np.arange(count, dtype=np.int64) * 131 + 7) % 251
                host = host.astype(_NP[dtype]).reshape(lead + (elems,))
                slab = torch.from_numpy(host.copy())
                views = _slab.plane_views(slab, n, planes)
                assert list(views) == [p[0] for p in planes], what
                covered = np.zeros(lead + (elems,), np.int32)
                for key, shape, vdtype, off in planes:
                    w = n * int(np.prod(shape)) * np.dtype(_NP[vdtype]).itemsize // size
                    want = np.ascontiguousarray(host[..., off:off + w]).view(_NP[vdtype]).reshape(lead + (n,) + tuple(shape))
                    got = views[key]
                    assert got.dtype == vdtype and tuple(got.shape) == want.shape, (what, key)
                    assert got.contiguous().numpy().tobytes() == want.tobytes(), (what, key)
                    assert got.data_ptr() == slab.data_ptr() + off * size, (what, key)           # a view, not a copy
                    covered[..., off:off + w] += 1
                if dtype == torch.int32:
                    assert (covered == 1).all(), what
                else:                                          # only the bytes that round a plane up to 16 are left out
                    pad = covered == 0
                    assert ((covered == 1) | pad).all(), what
                    ends = [(off + n * int(np.prod(shape)) * np.dtype(_NP[vdtype]).itemsize) for _, shape, vdtype, off in planes]
                    want_pad = np.zeros(elems, bool)
                    for e in ends:
                        want_pad[e:-(-e // 16) * 16] = True
                    assert elems % 16 == 0 and np.array_equal(pad, np.broadcast_to(want_pad, pad.shape)), what
                back = _slab.slab_of(views, planes, elems, dtype)
                assert back.data_ptr() == slab.data_ptr() and back.shape == slab.shape and back.stride() == slab.stride(), what
                assert back.dtype == dtype and torch.equal(back, slab), what
