"""The rollout_rows_kernel instances of the bus, world-builder and restaurant types (terminal rows of fused SAME_STEP rollouts into a
rows SLAB), read from the BUILT library's code-object notes the way tests/test_lane_final_rows_cpu.py reads its three types' (no GPU,
no recompilation), the C ABI that goes with them, and the Python side of the slab of compacted rows on the CPU.

A rows instance is the SAME_STEP rollout of its type plus a store pass that runs only at a step in which an episode ends.  Per instance:
  * no scratch (private segment 0), no dynamic stack, no vector register parked anywhere;
  * at least the waves per SIMD of its sibling rollout_kernel<1, (FLAT,) ACTIONS>, counted from the unified register total in blocks of
    8 out of 512;
  * LDS per workgroup that allows as many workgroups per CU as the sibling's (bus has none).
Figures of the build this was written against (registers, rows <given, hashed> against the sibling's):
  bus          149, 149 against 142, 144: three waves    no LDS; 256-lane workgroups, the segment found per wave
  restaurant   217, 209 against 213, 206: two waves      LDS 8,960
  wb Dict      183, 184 against 175, 176: two waves      LDS 6,400
  wb flat      167, 168 against 161, 161: three waves    LDS 7,936   (held to three waves by amdgpu_waves_per_eu; 170 without)"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from test_kernel_occupancy import LIB
from test_lane_final_rows_cpu import LDS_PER_CU, kernels, needs_tools, waves_per_simd  # noqa: F401  (kernels: a fixture)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cge_amd.h")
ENVS = ("bus", "restaurant", "world_builder")
# instance -> (fragment of the rows instance's mangled name, of its sibling's)
INSTANCES = {}
for given in ("Lb1E", "Lb0E"):
    INSTANCES[f"bus-{given}"] = ("3cge3bus19rollout_rows_kernelI" + given, "3cge3bus14rollout_kernelILi1E" + given)
    INSTANCES[f"restaurant-{given}"] = ("3cge10restaurant19rollout_rows_kernelI" + given, "3cge10restaurant14rollout_kernelILi1E" + given)
    for flat in ("Lb1E", "Lb0E"):
        INSTANCES[f"wb-{flat}-{given}"] = ("3cge2wb19rollout_rows_kernelI" + flat + given, "3cge2wb14rollout_kernelILi1E" + flat + given)


@needs_tools
@pytest.mark.parametrize("instance", list(INSTANCES))
def test_rows_instances_stay_where_their_siblings_are(kernels, instance):
    rows_frag, sibling_frag = INSTANCES[instance]
    (name, k), = [(n, v) for n, v in kernels.items() if rows_frag in n]
    (sname, s), = [(n, v) for n, v in kernels.items() if sibling_frag in n]
    print(f"{name}: {k}\n  sibling {sname}: {s}")
    for frag in ("11step_kernel", "14rollout_kernel", "12reset_kernel"):
        assert frag not in name, "the kernel counts of the existing tests"
    assert k["scratch"] == 0 and not k["dynamic"] and k["parked"] == 0 and k["agpr"] == 0, (name, k)
    assert s["scratch"] == 0 and waves_per_simd(k["vgpr"]) >= waves_per_simd(s["vgpr"]), (name, k, s)
    assert k["lds"] == s["lds"] and (k["lds"] == 0) == instance.startswith("bus"), (name, k, s)
    assert k["lds"] == 0 or LDS_PER_CU // k["lds"] >= LDS_PER_CU // s["lds"]


@needs_tools
def test_there_are_eight_rows_instances(kernels):
    assert sorted(n for n in kernels if "19rollout_rows_kernel" in n and any(f"3cge{ns}" in n for ns in ("3bus", "10restaurant", "2wb"))) == \
        sorted(n for frag, _ in INSTANCES.values() for n in kernels if frag in n) and len(INSTANCES) == 8


@pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")
def test_the_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(LIB)
    header = open(HEADER).read()
    from custom_gymnasium_environments_amd import _native
    for env in ENVS:
        for fn in ("rollout_final_obs", "final_obs_segment"):
            name = f"cge_rows_{env}_{fn}"
            assert hasattr(lib, name), name
            assert re.search(r"\b%s\(cge_%s \*h, " % (name, env), header) or re.search(r"\b%s\(const cge_%s \*h\)" % (name, env), header), name
            assert name in _native.SIGNATURES, name
        seg = getattr(lib, f"cge_rows_{env}_final_obs_segment")
        seg.restype, seg.argtypes = ctypes.c_int64, [ctypes.c_void_p]
        assert seg(None) == 0                                           # a null handle has no segments; a live one answers 64 (GPU tests)
        assert "final_obs_rows" in _native._ENV_TYPES[env][1].split()
        assert not [n for n in _native.SIGNATURES if n.startswith(f"cge_{env}_") and "final_obs" in n]       # the type's own surface is as it was


def _layouts():
    from custom_gymnasium_environments_amd import bus, restaurant, world_builder
    return {"bus": (bus.BusVectorEnv, types.SimpleNamespace(), torch.int32, {k: torch.int32 for k, _ in bus.PLANES}, dict(bus.PLANES)),
            "restaurant": (restaurant.RestaurantVectorEnv, types.SimpleNamespace(), torch.int32, {k: torch.int32 for k, _ in restaurant.PLANES},
                           dict(restaurant.PLANES)),
            "world_builder": (world_builder.WorldBuilderVectorEnv, types.SimpleNamespace(grid_size=3), torch.uint8,
                              {"grid": torch.int8, "resources": torch.float32, "population_capacity": torch.float32, "win_steps": torch.int32},
                              {"grid": (3, 3), "resources": (4,), "population_capacity": (1,), "win_steps": (1,)})}


@pytest.mark.parametrize("env", ENVS)
def test_the_rows_slab_reads_back_per_key(env):
    """A slab for R rows built with the type's layout function, known rows written through plane_views, and the gather final_obs() uses:
    per key the kept rows in the asked order, in the key's dtype and gymnasium's batched-Dict shape."""
    from custom_gymnasium_environments_amd import _slab
    cls, self, slab_dtype, dtypes, shapes = _layouts()[env]
    cap, nseg = 5, 3
    R = nseg * cap
    planes, elems = cls._rows_layout(self, R)
    assert [p[0] for p in planes] == list(shapes)
    slab = torch.full((elems,), 0x7F, dtype=slab_dtype)
    item = slab.element_size()
    ends = []
    for key, shape, dtype, off in planes:                                 # planes do not overlap, in order; world builder's start at multiples of 16 bytes
        nbytes = R * int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert off * item >= (ends[-1] if ends else 0) and (env != "world_builder" or (off * item) % 16 == 0), key
        ends.append(off * item + nbytes)
    assert ends[-1] <= elems * item
    if env == "world_builder":
        assert planes[1][3] == 144 and elems % 16 == 0, "G = 3: the grid plane of 15 rows is 135 bytes, padded to 144"
    views = _slab.plane_views(slab, R, planes)
    rng = np.random.RandomState(1)
    want = {}
    for key, v in views.items():
        assert v.dtype == dtypes[key] and tuple(v.shape) == (R,) + tuple(shapes[key]), key
        x = rng.randint(0, 100, size=tuple(v.shape))
        want[key] = torch.from_numpy(x).to(v.dtype)
        v.copy_(want[key])
    count = torch.tensor([2, 7, 0], dtype=torch.int32)                    # the second segment overflowed: its five rows
    keep = (torch.arange(cap)[None, :] < count.clamp(max=cap)[:, None]).reshape(-1)
    assert int(keep.sum()) == 7
    order = torch.tensor([6, 0, 3, 1, 5, 2, 4])
    got = _slab.gather_rows(slab, keep, order, planes)
    rows = torch.nonzero(keep).flatten()[order]
    assert list(got) == list(shapes)
    for key in got:
        assert got[key].dtype == dtypes[key] and tuple(got[key].shape) == (7,) + tuple(shapes[key]) and torch.equal(got[key], want[key][rows]), key
