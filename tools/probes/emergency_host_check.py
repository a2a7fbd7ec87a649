"""Replays every emergency fixture through the kernels' own dynamics code compiled for the CPU (csrc/emergency_env.hpp, driven by
emergency_host_check.cpp): the check of the record's packing, the draw order and the step logic that needs no GPU.  The host program
checks every runtime index itself, and `--sanitize` builds it with -fsanitize=address,undefined.  `--mean` pipes float64 vectors of 25
from stdin through the host build of mean25() to stdout (tests/test_emergency_cpu.py compares them with np.mean).
Usage: python tools/probes/emergency_host_check.py [--sanitize] [--mean]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from airline_host_check import ROOT, host_compiler  # noqa: E402

FIXTURES = ("emergency_hash", "emergency_dispatch", "emergency_idle", "emergency_timeout", "emergency_overrun", "emergency_day")

OPT = ["-O1"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(outdir, flags=OPT, compiler=None):
    """the host program, built into outdir with the given compiler flags; returns its path"""
    exe = os.path.join(outdir, "check")
    subprocess.run([compiler or host_compiler(), *flags, "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "probes", "emergency_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_fixture(name, outdir):
    """the fixture as the binary file that the host program reads; returns its path"""
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        z = {k: z[k] for k in z.files}
    n, T = z["reward"].shape
    obs = np.ascontiguousarray(np.bitwise_xor.accumulate(z["obs_xor"], axis=2).transpose(0, 2, 1))      # uint32 [n, T, 276]
    reset_at = np.full((n, T), -1, np.int32)
    for j, (i, t) in enumerate(z["reset_index"]):
        reset_at[i, t] = j
    path = os.path.join(outdir, name + ".bin")
    with open(path, "wb") as f:
        f.write(np.array([n, T, int(z["autoreset"]), len(z["reset_index"]), int(z["max_timesteps"])], np.int32).tobytes())
        f.write(z["reset_obs"].astype(np.float32).tobytes())
        for i in range(n):
            f.write(np.array([int(z["seed0"]) + i], np.int32).tobytes())
            f.write(z["actions"][i].astype(np.int32).tobytes())
            f.write(reset_at[i].tobytes())
            f.write(z["obs0"][i].astype(np.float32).tobytes())
            f.write(obs[i].tobytes())
            f.write(z["reward"][i].astype(np.float64).tobytes())
            f.write(z["terminated"][i].astype(np.uint8).tobytes())
            f.write(z["info"][i].astype(np.float64).tobytes())
    return path


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, OPT + (SANITIZE if "--sanitize" in sys.argv else []))
        if "--mean" in sys.argv:
            sys.exit(subprocess.run([exe, "--mean"]).returncode)
        for name in FIXTURES:
            subprocess.run([exe, write_fixture(name, tmp)], check=True)


if __name__ == "__main__":
    main()
