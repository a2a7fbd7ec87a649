"""Waves per SIMD of the restaurant kernels, read from the BUILT library's code-object notes as tests/test_kernel_occupancy.py does (no
GPU, no recompilation).  The record (eleven uint4 columns, unpacked: the waiting line, ten waiters, ten ready orders, the table
masks) lives in registers for a whole launch; the fused rollouts hold 16 ready generator words on top.  The floors are what the
measurements in profiles/restaurant_timing.txt were taken at: the step kernels at three waves per SIMD, the fused rollouts at two."""
import os

import pytest

from test_kernel_occupancy import LIB, LLVM, _kernels, check_floors

# mangled-name fragment -> minimum waves per SIMD; template arguments: autoreset mode (0 NextStep, 1 SameStep, 2 Disabled), caller's actions
FLOORS = {
    "10restaurant11step_kernelILi0E": 3,
    "10restaurant11step_kernelILi1E": 3,
    "10restaurant11step_kernelILi2E": 3,
    "10restaurant14rollout_kernelILi0ELb1E": 2,
    "10restaurant14rollout_kernelILi0ELb0E": 2,
    "10restaurant14rollout_kernelILi1ELb1E": 2,
    "10restaurant14rollout_kernelILi1ELb0E": 2,
    "10restaurant14rollout_kernelILi2ELb1E": 2,
    "10restaurant14rollout_kernelILi2ELb0E": 2,
}


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and the ROCm LLVM tools")
def test_restaurant_kernels_keep_their_waves_per_simd(tmp_path):
    check_floors(_kernels(str(tmp_path)), FLOORS)
