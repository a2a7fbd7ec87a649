"""Replays every farm fixture through the kernels' own dynamics code compiled for the CPU (csrc/farm_env.hpp, driven by
farm_host_check.cpp): the check of the record's packing, the draw order of both streams and the step logic that needs no GPU.
`--sanitize` builds the stand-alone program with -fsanitize=address,undefined and runs it directly (tools/probes/lane_host_check.py).
`--layout` prints the word offset of every field a fixture's `pokes` table can name (tests/_lane_env_pokes.py reads it), `--mean` pipes
float64 vectors of 4 from stdin through the host build of mean4() to stdout, `--stage-days` writes the forty stage durations,
`--randint S N` and `--randbelow S n k N` write draws of the two streams, `--record S0 N K` the float64 records after K steps of the
actions on stdin (tests/test_farm_cpu.py compares them with np.mean, Python and NumPy; tools/probes/farm_timing.py compares the last
with the device).
Usage: python tools/probes/farm_host_check.py [--sanitize] [--layout | --mean | --stage-days | --randint S N | --randbelow S n k N | --record S0 N K]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lane_host_check  # noqa: E402

FIXTURES = ("farm_hash", "farm_bankrupt", "farm_orchard", "farm_chores", "farm_overrun", "farm_two_years", "farm_soil", "farm_poked")
MODES = (("--layout", 0), ("--mean", 0), ("--stage-days", 0), ("--randint", 2), ("--randbelow", 4), ("--record", 3))
build, write_fixture, main = lane_host_check.bind("farm", FIXTURES, header=("max_years",), pokes=True, info0=True, modes=MODES)

if __name__ == "__main__":
    main()
