"""What the terminal rows of fused rollouts cost the three types with a Dict observation — bus, restaurant, world builder in both layouts
(rollout_rows_kernel into a rows slab) — SAME_STEP, rollout(32) with want_obs=False, at 131,072 and 1,048,576 envs:

  the same call from the same reset with rows registered (collect_final_obs) and without — without, the kernel is rollout_kernel<1, ...>,
  which this output leaves as it was — in two scenarios:
    no end     no episode ends inside the call: bus / restaurant at their default limits on hashed actions; world builder on the given
               actions farm x 4, lumberyard x 2, farm x 26, under which no env starves within 32 steps (asserted from done_count);
    ends       bus / restaurant with max_timesteps / max_episode_steps = 32: every env ends once, in the last step, all 64 lanes of a
               wave together; world builder under hashed actions, where ends are scattered over steps and lanes (several per env).
  The two are timed alternately, --runs pairs after a warm-up pair; times are device events around the call, us per step.  "spread" is
  (max - min) / min over the runs of one variant: what a ratio between the variants is read against.

  Beside them, from the built library's code-object notes (no GPU): registers, LDS, scratch and waves per SIMD of every rows instance
  and of its sibling rollout_kernel<1, ...>.

  python tools/probes/slab_final_rows_timing.py [--runs 5] [--n 131072 1048576] [--types bus restaurant wb_dict wb_flat]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

K = 32
WB_QUIET = [1, 1, 1, 1, 2, 2] + [1] * 26
# name -> (class, constructor arguments, the argument that limits an episode or None, rows_per_env of the `ends` scenario)
TYPES = {
    "bus": ("BusVectorEnv", {}, "max_timesteps", 1),
    "restaurant": ("RestaurantVectorEnv", {}, "max_episode_steps", 1),
    "wb_dict": ("WorldBuilderVectorEnv", {"flatten_obs": False}, None, 4),
    "wb_flat": ("WorldBuilderVectorEnv", {"flatten_obs": True}, None, 4),
}
# namespace fragment of the mangled names, template arguments before ACTIONS
NOTES = {"bus": ("3cge3bus", ""), "restaurant": ("3cge10restaurant", ""), "wb_dict": ("3cge2wb", "Lb0E"), "wb_flat": ("3cge2wb", "Lb1E")}


def child(sizes, runs, types):
    import torch
    import custom_gymnasium_environments_amd as cge
    from lane_timing import timed
    assert torch.cuda.is_available(), "needs an MI355X"
    for name in types:
        cls, kw, limit, per_env = TYPES[name]
        for n in sizes:
            for scenario in ("no end", "ends"):
                ckw = dict(kw)
                if limit and scenario == "ends":
                    ckw[limit] = K
                env = getattr(cge, cls)(n, autoreset_mode="SameStep", reuse_buffers=True, **ckw)
                acts = None
                if limit is None and scenario == "no end":
                    acts = torch.tensor(WB_QUIET, dtype=torch.int32, device="cuda")[:, None].expand(K, n).contiguous()
                out = {"type": name, "n": n, "scenario": scenario, "plain": [], "rows": [], "kernels": []}

                last = {}

                def call():
                    last["done_count"] = env.rollout(K, actions=acts, action_seed=7, want_obs=False)[2]

                for run in range(runs + 1):
                    pair = {}
                    for variant in ("plain", "rows"):
                        env.collect_final_obs(per_env if variant == "rows" else 0)
                        env.reset(seed=run)
                        pair[variant] = timed(call) / K
                        if run == 0:
                            out["kernels"].append(env.last_kernel())
                        if variant == "rows":
                            out["delivered"], out["dropped"] = int(env.final_obs()[1].shape[0]), env.final_obs_dropped()
                            out["ended"] = int(last["done_count"].sum())
                    if run:
                        out["plain"].append(pair["plain"]); out["rows"].append(pair["rows"])
                assert (out["ended"] == 0) == (scenario == "no end"), (name, n, scenario, out["ended"])
                print("RESULT " + json.dumps(out), flush=True)
                env.close()
                del env, acts
                torch.cuda.empty_cache()


def code_object_notes(lib):
    """{mangled name: fields} of the library's kernels (llvm-objdump --offloading, llvm-readelf --notes)"""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        out = {}
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp, f)], capture_output=True, text=True).stdout
            for blk in notes.split("  - .agpr_count:")[1:]:
                field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))   # noqa: E731
                out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = dict(vgpr=field("vgpr_count"), sgpr=field("sgpr_count"), lds=field("group_segment_fixed_size"),
                                                                        scratch=field("private_segment_fixed_size"), parked=field("vgpr_spill_count"))
        return out
    finally:
        shutil.rmtree(tmp)


def print_notes(lib, types):
    ks = code_object_notes(lib)
    waves = lambda v: min(8, 512 // (-(-max(v, 8) // 8) * 8))   # noqa: E731
    print("code-object notes: registers (unified total), scalar registers, LDS bytes, scratch bytes, parked registers, waves per SIMD")
    for name in types:
        ns, layout = NOTES[name]
        for given, label in (("Lb1E", "given"), ("Lb0E", "hashed")):
            for kind, frag in (("rollout_rows_kernel", f"{ns}19rollout_rows_kernelI{layout}{given}"), ("rollout_kernel<1>   ", f"{ns}14rollout_kernelILi1E{layout}{given}")):
                (k,) = [v for n, v in ks.items() if frag in n]
                print(f"  {name:10s} {label:6s} {kind}  {k['vgpr']:4d} {k['sgpr']:4d} {k['lds']:6d} {k['scratch']:3d} {k['parked']:3d}   {waves(k['vgpr'])} waves")


def fmt(v):
    return f"{min(v):9.2f} - {max(v):9.2f} (spread {(max(v) - min(v)) / min(v) * 100:5.2f} %)"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--types", nargs="+", default=list(TYPES))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--notes-only", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.n, args.runs, args.types)
        sys.exit(0)
    lib = os.path.join(ROOT, "custom_gymnasium_environments_amd", "libcge_amd.so")
    print_notes(lib, args.types)
    if args.notes_only:
        sys.exit(0)
    print(f"\nSAME_STEP, rollout({K}, want_obs=False) from reset(seed=run); us per step, ranges over {args.runs} alternating runs after a warm-up pair")
    for name in args.types:                                                  # one process per type: a failure starts nothing more on the device
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--n", *map(str, args.n), "--types", name],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"{name}: exit status {p.returncode}")
        for line in p.stdout.splitlines():
            if not line.startswith("RESULT "):
                continue
            r = json.loads(line[7:])
            mean = lambda v: sum(v) / len(v)                                 # noqa: E731
            print(f"\n{r['type']}, {r['n']} envs, {r['scenario']}: {r['ended']} episodes ended, {r['delivered']} rows delivered, {r['dropped']} dropped")
            print(f"  without rows  {fmt(r['plain'])}   {r['kernels'][0]}")
            print(f"  with rows     {fmt(r['rows'])}   {r['kernels'][1]}")
            print(f"  with / without on the means: {mean(r['rows']) / mean(r['plain']):.4f}")
