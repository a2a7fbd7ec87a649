"""What the terminal rows of fused rollouts cost the emergency, space-station and farm types (rollout_rows_kernel), at 1,048,576 envs,
SAME_STEP, rollout(32) on hashed actions from a reset (the airline type, which has no rows instance, is timed without rows: 71 steps, a
whole episode):

  (a) rows not registered: step() (k calls with device-resident actions) and rollout(k), us per step, for a BASELINE library (a build of
      the commit before the rows instances) and for this build, each in two processes that alternate — the two baseline processes give the
      run-to-run spread the comparison is read against;
  (b) rows registered (collect_final_obs(rows_per_env=1)): rollout(k) through rollout_rows_kernel, its ratio to (a) and the rows it
      delivered — the workload's own end rate;
  (c) the same rows from k SAME_STEP step() calls, the only way to get them without the rows instance: the factor between (c) and (b).

Times are device events around work that ends in a synchronise; the first run of every measurement warms up and is dropped; ranges are
over --runs runs.  One library per process (CGE_AMD_LIBRARY), so every column of the table is a child process of its own.

  python tools/probes/lane_final_rows_timing.py --baseline /path/to/older/libcge_amd.so [--runs 3] [--n 1048576] [--types ...]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TYPES = {   # name -> (class, number of actions, steps of a rollout)
    "airline": ("AirlineVectorEnv", 45, 71),
    "emergency": ("EmergencyVectorEnv", 50, 32),
    "space_station": ("SpaceStationVectorEnv", 40, 32),
    "farm": ("AgriculturalFarmVectorEnv", 45, 32),
}


def child(n, runs, types):
    import torch
    import custom_gymnasium_environments_amd as cge
    from lane_timing import timed
    assert torch.cuda.is_available(), "needs an MI355X"
    for name in types:
        cls, nact, k = TYPES[name]
        env = getattr(cge, cls)(n, autoreset_mode="SameStep", reuse_buffers=True)
        g = torch.Generator(device="cuda").manual_seed(0)
        acts = (torch.rand((k, n), generator=g, device="cuda") * nact).to(torch.int32)
        have_rows = hasattr(cge.native_lib(), f"cge_rows_{name}_rollout_final_obs")
        out = {"type": name, "k": k, "step": [], "roll": [], "rows": [], "delivered": None, "dropped": None, "kernels": []}
        for run in range(runs + 1):
            env.reset(seed=run)
            step = timed(lambda: [env.step(acts[t]) for t in range(k)]) / k
            out["kernels"] = [env.last_kernel()]
            env.reset(seed=run)
            roll = timed(lambda: env.rollout(k, action_seed=7, want_obs=False)) / k
            out["kernels"].append(env.last_kernel())
            rows = None
            if have_rows:
                env.collect_final_obs(rows_per_env=1)
                env.reset(seed=run)
                rows = timed(lambda: env.rollout(k, action_seed=7, want_obs=False)) / k
                out["kernels"].append(env.last_kernel())
                out["delivered"], out["dropped"] = int(env.final_obs()[0].shape[0]), env.final_obs_dropped()
                env.collect_final_obs(0)
            if run:
                out["step"].append(step); out["roll"].append(roll)
                if rows is not None:
                    out["rows"].append(rows)
        print("RESULT " + json.dumps(out), flush=True)
        env.close()
        del env, acts
        torch.cuda.empty_cache()


def rng(v):
    return f"{min(v):8.2f} - {max(v):8.2f}" if v else "       -          "


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", default=None, help="library of the commit before the rows instances")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--n", type=int, default=1048576)
    ap.add_argument("--types", nargs="+", default=list(TYPES))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.n, args.runs, args.types)
        sys.exit(0)
    this = os.path.join(ROOT, "custom_gymnasium_environments_amd", "libcge_amd.so")
    order = [("baseline 1", args.baseline), ("this build 1", this), ("baseline 2", args.baseline), ("this build 2", this)] if args.baseline else [("this build 1", this)]
    res = {}
    for label, lib in order:
        env = dict(os.environ)
        if lib != this:
            env["CGE_AMD_LIBRARY"] = lib
        else:
            env.pop("CGE_AMD_LIBRARY", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--n", str(args.n), "--types", *args.types],
                           env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"{label}: exit status {p.returncode}")                 # nothing more is started on the device
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                res.setdefault(r["type"], {})[label] = r
    print(f"n_envs {args.n}, SAME_STEP, hashed actions from reset(seed=run); us per step, ranges over {args.runs} runs after a warm-up run; one process per column")
    for name, by in res.items():
        k = next(iter(by.values()))["k"]
        print(f"\n{name}: rollout({k})")
        for label, r in by.items():
            print(f"  {label:13s} step() {rng(r['step'])}   rollout {rng(r['roll'])}   rollout with rows {rng(r['rows'])}   kernels {', '.join(r['kernels'])}")
        new = [r for label, r in by.items() if label.startswith("this")]
        old = [r for label, r in by.items() if label.startswith("baseline")]
        if old:
            mean = lambda v: sum(v) / len(v)                                 # noqa: E731
            o_roll, o_step = [mean(r["roll"]) for r in old], [mean(r["step"]) for r in old]
            n_roll, n_step = [mean(r["roll"]) for r in new], [mean(r["step"]) for r in new]
            print(f"  (a) rollout: baseline processes {o_roll[0]:.2f} / {o_roll[-1]:.2f} (spread {abs(o_roll[0] - o_roll[-1]) / min(o_roll) * 100:.2f} %), this build "
                  f"{n_roll[0]:.2f} / {n_roll[-1]:.2f}: {(mean(n_roll) / mean(o_roll) - 1) * 100:+.2f} % on the means")
            print(f"      step():  baseline processes {o_step[0]:.2f} / {o_step[-1]:.2f} (spread {abs(o_step[0] - o_step[-1]) / min(o_step) * 100:.2f} %), this build "
                  f"{n_step[0]:.2f} / {n_step[-1]:.2f}: {(mean(n_step) / mean(o_step) - 1) * 100:+.2f} % on the means")
        for r in new[:1]:
            if r["rows"]:
                a, b, c = sum(r["roll"]) / len(r["roll"]), sum(r["rows"]) / len(r["rows"]), sum(r["step"]) / len(r["step"])
                print(f"  (b) with rows / without: {b / a:.3f}; {r['delivered']} rows delivered ({r['delivered'] / (args.n * k) * 100:.3f} % of the env-steps end an episode), "
                      f"{r['dropped']} dropped at one row per env")
                print(f"  (c) {k} step() calls / rollout with rows: {c / b:.2f} x")
