"""get_state() / set_state() of the four env types with canonical records, two builds of the library against each other: wall time and
peak host memory.  What it answers: does the chunked record driver (csrc/cge_host.hpp: get_records / set_records) cost time against
the whole-batch staging it replaced, and is its host staging really independent of the batch size.

    python tools/probes/state_io_ab.py PARENT_LIB NEW_LIB [--envs 131072] [--reps 5] [--out profiles/state_io_ab.txt]

Every measurement is a fresh child process with CGE_AMD_LIBRARY pointing at one build (the library is loaded once per process), under
its own time limit; the first child that fails ends the run.
  time:    `reps` children per library, the two libraries interleaved; per type a child does one untimed get/set pair, then times one
           get_state() and one set_state() (the stream is idle: the calls synchronise).  Median and min-max per library.
  memory:  per type and library, one child that does a get/set pair at n envs and one at 4n; the growth of the peak RSS
           (resource.getrusage) over the pair, minus the caller's own record buffer = what the library staged on the host.
"""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TYPES = {"snake": ("SnakeVectorEnv", dict(grid_size=10)), "crypto": ("CryptoVectorEnv", {}), "traffic": ("TrafficVectorEnv", {}),
         "world_builder": ("WorldBuilderVectorEnv", {})}
CHILD_LIMIT = 240


def child(kinds, n, mode):
    sys.path.insert(0, ROOT)
    import torch
    import custom_gymnasium_environments_amd as cge
    out = {}
    for kind in kinds.split(","):
        cls, kw = TYPES[kind]
        env = getattr(cge, cls)(n, **kw)
        env.reset(seed=1)
        env.rollout(20, action_seed=2, want_obs=False)
        torch.cuda.synchronize()
        if mode == "time":
            env.set_state(env.get_state())                   # untimed: first-touch of the staging pages, lazy runtime setup
            t0 = time.perf_counter()
            rec = env.get_state()
            t1 = time.perf_counter()
            env.set_state(rec)
            t2 = time.perf_counter()
            out[kind] = dict(get_ms=(t1 - t0) * 1e3, set_ms=(t2 - t1) * 1e3)
        else:                                                # (one type per child: the peak is the process's)
            before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
            rec = env.get_state()
            env.set_state(rec)
            peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
            out[kind] = dict(staged_mb=(peak - before) / 1024.0 - rec.nbytes / 2**20, record_mb=rec.nbytes / 2**20)
        del rec
        env.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(lib, kind, n, mode):
    env = dict(os.environ, CGE_AMD_LIBRARY=os.path.abspath(lib))
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", kind, str(n), mode],
                       env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(f"child {kind} n={n} {mode} with {lib} ended with status {p.returncode}: nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--envs", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--types", default=",".join(TYPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_io_ab.txt"))
    a = ap.parse_args()
    libs = {"parent": a.parent, "new": a.new}
    lines = [f"tools/probes/state_io_ab.py: get_state / set_state at {a.envs} envs, {a.reps} fresh processes per library, interleaved; ms",
             "verdict: the new median against the parent's min-max"]
    t = {name: [] for name in libs}
    for _ in range(a.reps):
        for name, lib in libs.items():
            t[name].append(run_child(lib, a.types, a.envs, "time"))
    for kind in a.types.split(","):
        for call in ("get_ms", "set_ms"):
            v = {name: sorted(r[kind][call] for r in t[name]) for name in libs}
            med = {name: statistics.median(v[name]) for name in libs}
            verdict = "below" if med["new"] < v["parent"][0] else "inside" if med["new"] <= v["parent"][-1] else "ABOVE"
            lines.append(f"{kind:14s} {call[:3]}_state  parent median {med['parent']:8.1f} [{v['parent'][0]:8.1f} .. {v['parent'][-1]:8.1f}]   "
                         f"new median {med['new']:8.1f} [{v['new'][0]:8.1f} .. {v['new'][-1]:8.1f}]   ratio {med['new'] / med['parent']:.2f}  {verdict}")
            print(lines[-1], flush=True)
    lines.append("")
    lines.append("host memory the library staged for one get/set pair (peak RSS growth minus the caller's record buffer), MB, at n and 4n envs")
    for kind in a.types.split(","):
        for name, lib in libs.items():
            m1, m4 = run_child(lib, kind, a.envs, "mem")[kind], run_child(lib, kind, 4 * a.envs, "mem")[kind]
            lines.append(f"{kind:14s} {name:6s}  n: {m1['staged_mb']:9.1f} (records {m1['record_mb']:7.1f})   4n: {m4['staged_mb']:9.1f} (records {m4['record_mb']:7.1f})")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
