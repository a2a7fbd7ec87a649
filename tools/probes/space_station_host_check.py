"""Replays every space-station fixture through the kernels' own dynamics code compiled for the CPU (csrc/space_station_env.hpp, driven
by space_station_host_check.cpp): the check of the record's packing, the draw order and the step logic that needs no GPU.  `--sanitize`
builds the stand-alone program with -fsanitize=address,undefined and runs it directly (tools/probes/lane_host_check.py).  `--layout`
prints the word offset of every field a fixture's `pokes` table can name (tests/_lane_env_pokes.py reads it), `--record S0 N K` writes
the float64 records after K steps of the actions on stdin, `--mean N` pipes float64 vectors of N (6, 8 or 12) from stdin through the
host build of mean6() / mean8() / mean12() to stdout, `--tables` writes the three trigonometric tables and `--reset S0 N` the float64
module state after a seeded reset (tests/test_space_station_cpu.py compares them with np.mean, math and the model;
tools/probes/space_station_timing.py compares the last with the device).
Usage: python tools/probes/space_station_host_check.py [--sanitize] [--layout | --record S0 N K | --mean N | --tables | --reset S0 N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lane_host_check  # noqa: E402

FIXTURES = ("station_hash", "station_keep", "station_idle", "station_evacuate", "station_timeout", "station_overrun", "station_poked")
MODES = (("--layout", 0), ("--record", 3), ("--mean", 1), ("--tables", 0), ("--reset", 2))
build, write_fixture, main = lane_host_check.bind("space_station", FIXTURES, header=("max_steps",), pokes=True, info0=True, truncated=True, modes=MODES)

if __name__ == "__main__":
    main()
