"""Waves per SIMD of the world-builder kernels by their REGISTER counts, read from the built library's code-object notes as
tests/test_kernel_occupancy.py does (no GPU, no recompilation).  The record (13 grid words, the occupancy mask, a dozen scalars) and the
draw machinery (a 32-word twist chunk, a DRAW_WINDOW-word run) live in registers.  The floors are the committed build's: the step kernels
at four waves per SIMD, the fused rollouts at three (flat rows) and two (Dict slab) — the build profiles/world_builder_timing.txt was
measured with.  Registers only: the one-wave workgroups also hold 6,400 B (Dict) or 7,936 B (flat) of LDS each, which caps a CU at 25 / 20
workgroups, so reset_kernel's 8 is a register figure, not its residency."""
import os

import pytest

from test_kernel_occupancy import LIB, LLVM, _kernels, check_floors

# mangled-name fragment -> minimum waves per SIMD; template arguments: autoreset mode (0 NextStep, 1 SameStep, 2 Disabled), flat rows
# (rollouts: then the caller's actions)
FLOORS = {f"2wb11step_kernelILi{m}ELb{f}E": 4 for m in range(3) for f in range(2)}
FLOORS.update({f"2wb14rollout_kernelILi{m}ELb{f}ELb{a}E": 3 if f else 2 for m in range(3) for f in range(2) for a in range(2)})
FLOORS.update({"2wb12reset_kernelILb0E": 8, "2wb12reset_kernelILb1E": 8})


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and the ROCm LLVM tools")
def test_world_builder_kernels_keep_their_waves_per_simd(tmp_path):
    check_floors(_kernels(str(tmp_path)), FLOORS)
