"""Replays every restaurant fixture through the kernels' own dynamics code compiled for the CPU (csrc/restaurant_env.hpp, driven by
restaurant_host_check.cpp): the check of the record and of the step logic that needs no GPU.  `-fsanitize` on the host build finds an
index out of range in the record's arrays before a kernel could.  The build and the driver are those of the record-lane types
(tools/probes/lane_host_check.py); the binary file is the type's own.  Usage: python tools/probes/restaurant_host_check.py [--sanitize]"""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lane_host_check  # noqa: E402
from lane_host_check import ROOT  # noqa: E402

KEYS = ("waiting_customers", "waiter_status", "table_occupancy", "table_cleanliness", "kitchen_queue", "ready_orders")
FIXTURES = ("restaurant_hash", "restaurant_busy", "restaurant_short", "restaurant_short40", "restaurant_long")


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


build, write_fixture, main = lane_host_check.bind("restaurant", FIXTURES, writer=write_fixture)

if __name__ == "__main__":
    main()
