"""Replays every airline fixture through the kernels' own dynamics code compiled for the CPU (csrc/airline_env.hpp, driven by
airline_host_check.cpp): the check of the record's packing, the draw order and the step logic that needs no GPU.  The host program
checks every runtime index itself, and `--sanitize` builds it with -fsanitize=address,undefined (tools/probes/lane_host_check.py).
Usage: python tools/probes/airline_host_check.py [--sanitize]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lane_host_check  # noqa: E402

FIXTURES = ("airline_hash", "airline_dispatch", "airline_cancel", "airline_overrun")
build, write_fixture, main = lane_host_check.bind("airline", FIXTURES)

if __name__ == "__main__":
    main()
