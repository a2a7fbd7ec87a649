"""Waves per SIMD of the airline kernels, read from the BUILT library's code-object notes as tests/test_kernel_occupancy.py does (no GPU,
no recompilation), and that none of them uses scratch.  Gates, weather and the scalars live in registers for a whole launch; what a
runtime index reaches is in LDS (21,760 bytes per wave, which allows seven one-wave workgroups per CU: under two per SIMD whatever the
registers) or in HBM columns.  The floors are what the measurements in profiles/airline_timing.txt were taken
at: the step kernels at two waves per SIMD (243-247 registers), the fused rollouts at one (256-296 with the accumulation registers:
thirty flight words and twenty-five maintenance bases are fetched together).  Scratch came and went while the kernel was written — 64-bit per-lane column
addresses kept across the step loop spilled up to 320 registers — so it is pinned at zero here."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_occupancy import LIB, LLVM, _kernels, check_floors

# mangled-name fragment -> minimum waves per SIMD; template arguments: autoreset mode (0 NextStep, 1 SameStep, 2 Disabled), caller's actions
FLOORS = {
    "7airline11step_kernelILi0E": 2,
    "7airline11step_kernelILi1E": 2,
    "7airline11step_kernelILi2E": 2,
    "7airline14rollout_kernelILi0ELb1E": 1,
    "7airline14rollout_kernelILi0ELb0E": 1,
    "7airline14rollout_kernelILi1ELb1E": 1,
    "7airline14rollout_kernelILi1ELb0E": 1,
    "7airline14rollout_kernelILi2ELb1E": 1,
    "7airline14rollout_kernelILi2ELb0E": 1,
}
needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and the ROCm LLVM tools")


@needs_tools
def test_airline_kernels_keep_their_waves_per_simd(tmp_path):
    check_floors(_kernels(str(tmp_path)), FLOORS)


@needs_tools
def test_no_airline_kernel_uses_scratch(tmp_path):
    tmp = str(tmp_path)
    lib = os.path.join(tmp, "lib.so")
    shutil.copy(LIB, lib)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], cwd=tmp, check=True, capture_output=True)
    seen = {}
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)], capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and "3cge7airline" in name.group(1):
                seen[name.group(1)] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                       int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)), "uses_dynamic_stack: true" in blk)
    assert len(seen) == 11, sorted(seen)                                  # nine step / rollout instances, reset_kernel, info_kernel
    assert all(v == (0, 0, False) for v in seen.values()), seen
