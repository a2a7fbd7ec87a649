"""Waves per SIMD of the bus kernels, read from the BUILT library's code-object notes as tests/test_kernel_occupancy.py does (no GPU, no
recompilation).  The record (three uint4 columns) and the reset's draw machinery (a 32-word twist chunk, a 16-word run) live in
registers; the floors are what the measurements in profiles/bus_timing.txt were taken at: the step kernels with an in-kernel reset
(NextStep, SameStep) at four waves per SIMD, the fused rollouts at three, the Disabled instances (no reset code) higher."""
import os

import pytest

from test_kernel_occupancy import LIB, LLVM, _kernels, check_floors

# mangled-name fragment -> minimum waves per SIMD; template arguments: autoreset mode (0 NextStep, 1 SameStep, 2 Disabled), caller's actions
FLOORS = {
    "3bus11step_kernelILi0E": 4,
    "3bus11step_kernelILi1E": 4,
    "3bus11step_kernelILi2E": 6,
    "3bus14rollout_kernelILi0ELb1E": 3,
    "3bus14rollout_kernelILi0ELb0E": 3,
    "3bus14rollout_kernelILi1ELb1E": 3,
    "3bus14rollout_kernelILi1ELb0E": 3,
    "3bus14rollout_kernelILi2ELb1E": 4,
    "3bus14rollout_kernelILi2ELb0E": 4,
}


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and the ROCm LLVM tools")
def test_bus_kernels_keep_their_waves_per_simd(tmp_path):
    check_floors(_kernels(str(tmp_path)), FLOORS)
