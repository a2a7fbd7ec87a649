"""A/B of two builds of the CPU oracle (oracle/libcge_oracle.so) on the legs bench.py reports as cpu_baseline (no GPU).

    taskset -c 2 python tools/probes/oracle_driver_ab.py PARENT/libcge_oracle.so oracle/libcge_oracle.so

Both libraries are loaded into this one process.  For each of the eight env types, constructed as bench.py's cpu_baseline does
(SAME_STEP, default arguments): rollout(200, 7) on 256 freshly seeded and reset envs, one thread.  Four rounds of parent / new /
parent / new; a sample is the best of five such rollouts.  Per type the table gives both medians over the rounds in env-steps/s
and the parent's own max - min; the new library passes if its median is no slower than the parent's median minus that spread.
Exit status 1 if a type fails."""
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

import oracle  # noqa: E402

N, K, ROUNDS, BEST_OF = 256, 200, 4, 5
CTOR = {"snake": lambda: oracle.SnakeOracle(N, 10, oracle.SAME_STEP), "crypto": lambda: oracle.CryptoOracle(N, "discrete", oracle.SAME_STEP),
        "traffic": lambda: oracle.TrafficOracle(N, oracle.SAME_STEP), "parking": lambda: oracle.ParkingOracle(N, oracle.SAME_STEP),
        "climate": lambda: oracle.ClimateOracle(N, oracle.SAME_STEP), "fleet": lambda: oracle.FleetOracle(N, oracle.SAME_STEP),
        "manufacturing": lambda: oracle.ManufacturingOracle(N, oracle.SAME_STEP), "hospital": lambda: oracle.HospitalOracle(N, oracle.SAME_STEP)}


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    oracle._declare(L)
    return L


def sample(L, name):
    """best of BEST_OF: env-steps/s of rollout(K, 7) on N fresh envs, with library L behind the wrapper"""
    oracle._lib = L
    best = 0.0
    for _ in range(BEST_OF):
        o = CTOR[name]()
        o.seed(np.arange(N, dtype=np.uint64))
        o.reset()
        t = time.perf_counter()
        o.rollout(K, 7, 0, 0)
        best = max(best, N * K / (time.perf_counter() - t))
        del o
    return best


def main(parent_path, new_path):
    parent, new = load(parent_path), load(new_path)
    print(f"cpus {sorted(os.sched_getaffinity(0))}; {N} envs x {K} steps, {ROUNDS} rounds parent/new, sample = best of {BEST_OF}; env-steps/s")
    print(f"{'type':14s} {'parent median':>14s} {'parent spread':>14s} {'new median':>14s} {'new/parent':>10s} {'bound':>14s}  verdict")
    failed = []
    for name in CTOR:
        p, q = [], []
        for _ in range(ROUNDS):
            p.append(sample(parent, name))
            q.append(sample(new, name))
        pm, qm, spread = statistics.median(p), statistics.median(q), max(p) - min(p)
        ok = qm >= pm - spread
        failed += [] if ok else [name]
        print(f"{name:14s} {pm:14.4e} {spread:14.3e} {qm:14.4e} {qm / pm:10.4f} {pm - spread:14.4e}  {'ok' if ok else 'SLOWER'}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
