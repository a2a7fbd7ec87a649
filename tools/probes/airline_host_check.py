"""Replays every airline fixture through the kernels' own dynamics code compiled for the CPU (csrc/airline_env.hpp, driven by
airline_host_check.cpp): the check of the record's packing, the draw order and the step logic that needs no GPU.  The host program
checks every runtime index itself, and `--sanitize` builds it with -fsanitize=address,undefined.
Usage: python tools/probes/airline_host_check.py [--sanitize]"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURES = ("airline_hash", "airline_dispatch", "airline_cancel", "airline_overrun")


def host_compiler():
    """g++ / c++ / clang++ from the PATH, else the clang++ that hipcc itself drives (the build needs ROCm anyway)."""
    for cc in ("g++", "c++", "clang++"):
        if shutil.which(cc):
            return cc
    rocm = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin", "clang++")
    if os.path.exists(rocm):
        return rocm
    raise RuntimeError("no host C++ compiler found (g++, c++, clang++, ROCm's clang++)")


OPT = ["-O1"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(outdir, flags=OPT, compiler=None):
    """the host program, built into outdir with the given compiler flags; returns its path"""
    exe = os.path.join(outdir, "check")
    subprocess.run([compiler or host_compiler(), *flags, "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "probes", "airline_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_fixture(name, outdir):
    """the fixture as the binary file that the host program reads; returns its path"""
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        z = {k: z[k] for k in z.files}
    n, T = z["reward"].shape
    obs = np.ascontiguousarray(np.bitwise_xor.accumulate(z["obs_xor"], axis=2).transpose(0, 2, 1))      # uint32 [n, T, 160]
    reset_at = np.full((n, T), -1, np.int32)
    for j, (i, t) in enumerate(z["reset_index"]):
        reset_at[i, t] = j
    path = os.path.join(outdir, name + ".bin")
    with open(path, "wb") as f:
        f.write(np.array([n, T, int(z["autoreset"]), len(z["reset_index"])], np.int32).tobytes())
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
        for name in FIXTURES:
            subprocess.run([exe, write_fixture(name, tmp)], check=True)


if __name__ == "__main__":
    main()
