"""Replays every space-station fixture through the kernels' own dynamics code compiled for the CPU (csrc/space_station_env.hpp, driven
by space_station_host_check.cpp): the check of the record's packing, the draw order and the step logic that needs no GPU.  `--sanitize`
builds the stand-alone program with -fsanitize=address,undefined and runs it directly.  `--layout` prints the word offset of every field a fixture's
`pokes` table can name (tests/_lane_env_pokes.py reads it), `--record S0 N K` writes the float64 records after K steps of the
actions on stdin, `--mean N` pipes float64 vectors of N (6, 8 or
12) from stdin through the host build of mean6() / mean8() / mean12() to stdout, `--tables` writes the three trigonometric tables and
`--reset S0 N` the float64 module state after a seeded reset (tests/test_space_station_cpu.py compares them with np.mean, math and
the model; tools/probes/space_station_timing.py compares the last with the device).
Usage: python tools/probes/space_station_host_check.py [--sanitize] [--layout | --record S0 N K | --mean N | --tables | --reset S0 N]"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from airline_host_check import ROOT, host_compiler  # noqa: E402

FIXTURES = ("station_hash", "station_keep", "station_idle", "station_evacuate", "station_timeout", "station_overrun", "station_poked")

OPT = ["-O1"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(outdir, flags=OPT, compiler=None):
    """the host program, built into outdir with the given compiler flags; returns its path"""
    exe = os.path.join(outdir, "check")
    subprocess.run([compiler or host_compiler(), *flags, "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "probes", "space_station_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_fixture(name, outdir):
    """the fixture as the binary file that the host program reads; returns its path"""
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        z = {k: z[k] for k in z.files}
    n, T = z["reward"].shape
    obs = np.ascontiguousarray(np.bitwise_xor.accumulate(z["obs_xor"], axis=2).transpose(0, 2, 1))      # uint32 [n, T, 120]
    reset_at = np.full((n, T), -1, np.int32)
    for j, (i, t) in enumerate(z["reset_index"]):
        reset_at[i, t] = j
    path = os.path.join(outdir, name + ".bin")
    with open(path, "wb") as f:
        pokes = z.get("pokes", np.zeros((0, 4)))
        names = json.loads(str(z["poke_fields"])) if "poke_fields" in z else []
        f.write(np.array([n, T, int(z["autoreset"]), len(z["reset_index"]), int(z["max_steps"]), len(pokes)], np.int32).tobytes())
        f.write(z["reset_obs"].astype(np.float32).tobytes())
        for i, t, k, value in pokes:                                  # the named field of env i is set before step t
            f.write(struct.pack("<ii24sd", int(i), int(t), names[int(k)].encode(), float(value)))
        for i in range(n):
            f.write(np.array([int(z["seed0"]) + i], np.int32).tobytes())
            f.write(z["actions"][i].astype(np.int32).tobytes())
            f.write(reset_at[i].tobytes())
            f.write(z["obs0"][i].astype(np.float32).tobytes())
            f.write(z["info0"][i].astype(np.float64).tobytes())
            f.write(obs[i].tobytes())
            f.write(z["reward"][i].astype(np.float64).tobytes())
            f.write(z["terminated"][i].astype(np.uint8).tobytes())
            f.write(z["truncated"][i].astype(np.uint8).tobytes())
            f.write(z["info"][i].astype(np.float64).tobytes())
    return path


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, OPT + (SANITIZE if "--sanitize" in sys.argv else []))
        for mode, nargs in (("--layout", 0), ("--record", 3), ("--mean", 1), ("--tables", 0), ("--reset", 2)):
            if mode in sys.argv:
                at = sys.argv.index(mode)
                sys.exit(subprocess.run([exe, *sys.argv[at:at + 1 + nargs]]).returncode)
        for name in FIXTURES:
            subprocess.run([exe, write_fixture(name, tmp)], check=True)


if __name__ == "__main__":
    main()
