"""Replays every emergency fixture through the kernels' own dynamics code compiled for the CPU (csrc/emergency_env.hpp, driven by
emergency_host_check.cpp): the check of the record's packing, the draw order and the step logic that needs no GPU.  The host program
checks every runtime index itself, and `--sanitize` builds it with -fsanitize=address,undefined (tools/probes/lane_host_check.py).
`--mean` pipes float64 vectors of 25 from stdin through the host build of mean25() to stdout (tests/test_emergency_cpu.py compares
them with np.mean).
Usage: python tools/probes/emergency_host_check.py [--sanitize] [--mean]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lane_host_check  # noqa: E402

FIXTURES = ("emergency_hash", "emergency_dispatch", "emergency_idle", "emergency_timeout", "emergency_overrun", "emergency_day")
build, write_fixture, main = lane_host_check.bind("emergency", FIXTURES, header=("max_timesteps",), modes=(("--mean", 0),))

if __name__ == "__main__":
    main()
