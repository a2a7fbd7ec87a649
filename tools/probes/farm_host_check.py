"""Replays every farm fixture through the kernels' own dynamics code compiled for the CPU (csrc/farm_env.hpp, driven by
farm_host_check.cpp): the check of the record's packing, the draw order of both streams and the step logic that needs no GPU.
`--sanitize` builds the stand-alone program with -fsanitize=address,undefined and runs it directly.  `--layout` prints the word offset of every field a fixture's
`pokes` table can name (tests/_lane_env_pokes.py reads it), `--mean` pipes float64 vectors
of 4 from stdin through the host build of mean4() to stdout, `--stage-days` writes the forty stage durations, `--randint S N` and
`--randbelow S n k N` write draws of the two streams, `--record S0 N K` the float64 records after K steps of the actions on stdin
(tests/test_farm_cpu.py compares them with np.mean, Python and NumPy; tools/probes/farm_timing.py compares the last with the device).
Usage: python tools/probes/farm_host_check.py [--sanitize] [--layout | --mean | --stage-days | --randint S N | --randbelow S n k N | --record S0 N K]"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from airline_host_check import ROOT, host_compiler  # noqa: E402

FIXTURES = ("farm_hash", "farm_bankrupt", "farm_orchard", "farm_chores", "farm_overrun", "farm_two_years", "farm_soil", "farm_poked")
MODES = (("--layout", 0), ("--mean", 0), ("--stage-days", 0), ("--randint", 2), ("--randbelow", 4), ("--record", 3))

OPT = ["-O1"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(outdir, flags=OPT, compiler=None):
    """the host program, built into outdir with the given compiler flags; returns its path"""
    exe = os.path.join(outdir, "check")
    subprocess.run([compiler or host_compiler(), *flags, "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "probes", "farm_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_fixture(name, outdir):
    """the fixture as the binary file that the host program reads; returns its path"""
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        z = {k: z[k] for k in z.files}
    n, T = z["reward"].shape
    obs = np.ascontiguousarray(np.bitwise_xor.accumulate(z["obs_xor"], axis=2).transpose(0, 2, 1))      # uint32 [n, T, 134]
    reset_at = np.full((n, T), -1, np.int32)
    for j, (i, t) in enumerate(z["reset_index"]):
        reset_at[i, t] = j
    path = os.path.join(outdir, name + ".bin")
    with open(path, "wb") as f:
        pokes = z.get("pokes", np.zeros((0, 4)))
        names = json.loads(str(z["poke_fields"])) if "poke_fields" in z else []
        f.write(np.array([n, T, int(z["autoreset"]), len(z["reset_index"]), int(z["max_years"]), len(pokes)], np.int32).tobytes())
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
            f.write(z["info"][i].astype(np.float64).tobytes())
    return path


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, OPT + (SANITIZE if "--sanitize" in sys.argv else []))
        for mode, nargs in MODES:
            if mode in sys.argv:
                at = sys.argv.index(mode)
                sys.exit(subprocess.run([exe, *sys.argv[at:at + 1 + nargs]]).returncode)
        for name in FIXTURES:
            subprocess.run([exe, write_fixture(name, tmp)], check=True)


if __name__ == "__main__":
    main()
