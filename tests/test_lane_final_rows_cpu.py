"""The rollout_rows_kernel instances of the emergency, space-station and farm types (terminal rows of fused SAME_STEP rollouts),
read from the BUILT library's code-object notes as tests/test_kernel_occupancy.py does (no GPU, no recompilation), and the C ABI that
goes with them.

A rows instance is the SAME_STEP rollout of its type plus a store pass that runs only at a step in which an episode ends, so it has to
stay where its sibling rollout_kernel<1, ACTIONS> is: the record in registers, nothing in memory.  Per instance:
  * no scratch (private segment 0) and no dynamic stack: no register of the record is ever written to memory;
  * registers "spilled" within the register file.  The notes count a vector register parked in an accumulation register as a spill
    (.vgpr_spill_count) although it never leaves the register file; the emergency rollouts have none, the space-station
    and farm rollouts were built and measured with up to 26 and 218 of them (profiles/space_station_timing.txt, profiles/farm_timing.txt).
    The bound for a rows instance is the largest figure among the rollout_kernel instances of its type in the same build — zero for
    emergency;
  * at least the sibling's waves per SIMD.  .vgpr_count is the unified total (it includes .agpr_count), allocated in blocks of 8 out
    of 512 per SIMD lane; the helper of tests/test_kernel_occupancy.py adds the accumulation registers a second time and would call
    264 registers and 254 the same single wave, which they are not (the airline type's rows instance, left out for this reason:
    profiles/lane_final_rows_timing.txt);
  * LDS per workgroup that allows as many workgroups per CU (160 KiB of LDS) as the sibling's does.
Figures of the build this was written against (registers = arch + accumulation, parked registers, LDS bytes), rows <given, hashed>
against rollout_kernel<1, given / hashed>:
  emergency 256+46 twice     0, 0      30,720    sibling 256+37 twice, 0, 30,720
  station   256+92, 256+86   16, 6     9,360     sibling 256+83, 256+78; 16, 0; 9,360
  farm      256+189, 256+196 218, 120  9,360     sibling 256+182, 256+192; 218, 120; 9,360
Every one of them runs at one wave per SIMD, as its sibling does."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_occupancy import LIB, LLVM

LDS_PER_CU = 160 * 1024
# type -> (fragment of the rows instances' mangled names, fragment of the rollout_kernel instances')
TYPES = {
    "emergency": ("3cge9emergency19rollout_rows_kernel", "3cge9emergency14rollout_kernel"),
    "space_station": ("3cge7station19rollout_rows_kernel", "3cge7station14rollout_kernel"),
    "farm": ("3cge4farm19rollout_rows_kernel", "3cge4farm14rollout_kernel"),
}


def waves_per_simd(vgpr_total):
    return min(8, 512 // (-(-max(vgpr_total, 8) // 8) * 8))


needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and the ROCm LLVM tools")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: the fields of its code-object note}"""
    tmp = str(tmp_path_factory.mktemp("notes"))
    lib = os.path.join(tmp, "lib.so")
    shutil.copy(LIB, lib)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], cwd=tmp, check=True, capture_output=True)
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)], capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            out[name] = dict(agpr=int(re.match(r"\s*(\d+)", blk).group(1)), vgpr=field("vgpr_count"), lds=field("group_segment_fixed_size"),
                             scratch=field("private_segment_fixed_size"), parked=field("vgpr_spill_count"), dynamic="uses_dynamic_stack: true" in blk)
    return out


@needs_tools
@pytest.mark.parametrize("env", list(TYPES))
def test_rows_instances_stay_where_their_siblings_are(kernels, env):
    rows_frag, rollout_frag = TYPES[env]
    rows = {n: k for n, k in kernels.items() if rows_frag in n}
    rollouts = {n: k for n, k in kernels.items() if rollout_frag in n}
    assert len(rows) == 2 and len(rollouts) == 6, (sorted(rows), sorted(rollouts))
    parked_bound = max(k["parked"] for k in rollouts.values())
    assert parked_bound == 0 or env in ("space_station", "farm")
    for given in ("Lb1E", "Lb0E"):
        (name, k), = [(n, k) for n, k in rows.items() if rows_frag + "I" + given in n]
        (sname, s), = [(n, k) for n, k in rollouts.items() if rollout_frag + "ILi1E" + given in n]
        print(f"{name}: {k}\n  sibling {sname}: {s}")
        for frag in ("11step_kernel", "14rollout_kernel", "12reset_kernel"):
            assert frag not in name, "the kernel counts of the existing tests"
        assert k["scratch"] == 0 and not k["dynamic"], (name, k)
        assert k["parked"] <= parked_bound, (name, k, parked_bound)
        assert k["vgpr"] >= k["agpr"] and waves_per_simd(k["vgpr"]) >= waves_per_simd(s["vgpr"]), (name, k, s)
        assert k["lds"] > 0 and LDS_PER_CU // k["lds"] >= LDS_PER_CU // s["lds"], (name, k, s)


@pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")
def test_the_entry_points_are_exported_and_bound():
    lib = ctypes.CDLL(LIB)
    for env in TYPES:
        for fn in ("rollout_final_obs", "final_obs_segment"):
            assert hasattr(lib, f"cge_rows_{env}_{fn}"), (env, fn)
        seg = getattr(lib, f"cge_rows_{env}_final_obs_segment")
        seg.restype, seg.argtypes = ctypes.c_int64, [ctypes.c_void_p]
        assert seg(None) == 0                                           # a null handle has no segments; a live one answers 64 (GPU tests)
    from custom_gymnasium_environments_amd import _native
    for env in TYPES:
        assert "final_obs_rows" in _native._ENV_TYPES[env][1].split()
        assert f"cge_rows_{env}_rollout_final_obs" in _native.SIGNATURES and f"cge_rows_{env}_final_obs_segment" in _native.SIGNATURES
        assert not [n for n in _native.SIGNATURES if n.startswith(f"cge_{env}_") and "final_obs" in n]       # the type's own surface is as it was
