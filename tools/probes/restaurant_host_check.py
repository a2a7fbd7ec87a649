"""Replays every restaurant fixture through the kernels' own dynamics code compiled for the CPU (csrc/restaurant_env.hpp, driven by
restaurant_host_check.cpp): the check of the record and of the step logic that needs no GPU.  `-fsanitize` on the host build finds an
index out of range in the record's arrays before a kernel could.  Usage: python tools/probes/restaurant_host_check.py [--sanitize]"""
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KEYS = ("waiting_customers", "waiter_status", "table_occupancy", "table_cleanliness", "kitchen_queue", "ready_orders")
FIXTURES = ("restaurant_hash", "restaurant_busy", "restaurant_short", "restaurant_short40", "restaurant_long")


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
    subprocess.run([compiler or host_compiler(), *flags, "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "probes", "restaurant_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_fixture(name, outdir):
    """the fixture as the binary file that the host program reads; returns its path"""
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        z = {k: z[k] for k in z.files}
    n, T = z["reward"].shape
    path = os.path.join(outdir, name + ".bin")
    with open(path, "wb") as f:
        f.write(np.array([n, T, int(z["max_episode_steps"])], np.int32).tobytes())
        for i in range(n):
            rng = random.Random(int(z["seed0"]) + i)
            f.write(z["actions"][i].astype(np.int32).tobytes())
            f.write(np.array([rng.random() for _ in range(T)], np.float64).tobytes())
            f.write(z["reward"][i].tobytes())
            f.write(z["total_reward"][i].tobytes())
            f.write(z["info"][i].astype(np.int32).tobytes())
            f.write(np.concatenate([z["obs_" + k][i].reshape(T, -1) for k in KEYS], 1).astype(np.int32).tobytes())
    return path


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, OPT + (SANITIZE if "--sanitize" in sys.argv else []))
        for name in FIXTURES:
            subprocess.run([exe, write_fixture(name, tmp)], check=True)


if __name__ == "__main__":
    main()
