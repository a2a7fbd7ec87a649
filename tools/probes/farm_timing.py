"""AgriculturalFarmVectorEnv timing from a reset, at 131,072 and 1,048,576 envs, SAME_STEP (loop, header and options: lane_timing.py):

  reset()      on its own (54 uniforms and 16 bounded integers, about 125 generator words per env)
  step()       k calls with device-resident actions (uniform over 0..44), device events around them -> us per step
  rollout(k)   one fused launch with the full trajectory and per-step outputs (the same actions, given) -> us per step; at the larger
               size also with compact_obs (rows of 134 floats instead of 620)

five runs each after a warm-up run, reported as ranges, with the bytes each path moves per env-step, spelled out from the layout
(DESIGN.md section 3.18), the time a device-to-device copy of the same bytes takes on this box (measured in this process on 2-GiB torch
buffers: bytes read + written per second) and the ratio of the kernel time to it.  CGE_AMD_LIBRARY selects the library.

`--host-record F`: no GPU; writes to F the float64 records (89 values per env) that the host build of csrc/farm_env.hpp holds after
reset(seed) and 64 hashed steps (a_seed 1) for seeds 0..N-1, N from --log-caveat.
`--log-caveat N --host-file F`: no timing; runs the same on the device and counts the float64 record values that differ from F, read
from snapshot() bytes: the size of the `log` caveat.

  python tools/probes/farm_timing.py [--runs 5] [--sizes ...] [--k 32] [--log-caveat N (--host-record F | --host-file F)]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "gen"))
import numpy as np  # noqa: E402

import common  # noqa: E402  (the counter hash of the synthetic actions)
import lane_timing  # noqa: E402
from lane_timing import rng  # noqa: E402

OBS, COMPACT = 620 * 4, 134 * 4
RECORD = 832                                     # loaded by every launch and stored by it: the whole record
WORDS = 44                                       # generator words of a typical step: the weather 5 doubles, three pest tests, 2.5 polar
                                                 # pairs of 2.55 doubles each, five market uniforms: about 22 doubles
DRAWN = WORDS * 4
TWIST = WORDS * 12                               # ... and what twisting them ahead moves: word k and word k + 397 read, word k written
STEPS, A_SEED = 64, 1                            # the run of the log caveat


def step_bytes(obs):
    return obs + 4 + 1 + 4 + 2 * RECORD + DRAWN + TWIST


def roll_bytes(k, obs):
    return obs + 4 + 1 + 4 + DRAWN + TWIST + (2 * RECORD + 12) / k


def run(n, runs, copy_gbs, k, compact):
    import custom_gymnasium_environments_amd as cge
    obs = COMPACT if compact else OBS
    make = lambda: cge.AgriculturalFarmVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True, compact_obs=compact)   # noqa: E731
    rows = lane_timing.measure(make, n, k, 45, runs, label=f"  compact_obs {compact}")
    copy_us = lambda b: b * n / (copy_gbs * 1e9) * 1e6           # noqa: E731
    sb, rb = step_bytes(obs), roll_bytes(k, obs)
    print(f"  reset()                {rng(rows['reset'])} us   writes {obs + RECORD} B/env; as a copy: {copy_us(obs + RECORD):.1f} us")
    print(f"  step()   {k} calls      {rng(rows['step'])} us/step   moves {sb} B/env-step (obs {obs} + reward 4 + flag 1 + action 4 + record in {RECORD} "
          f"+ out {RECORD} + generator words drawn {DRAWN} + twisted {TWIST}); the same bytes as a copy: {copy_us(sb):.1f} us; ratio "
          f"{min(rows['step']) / copy_us(sb):.2f} - {max(rows['step']) / copy_us(sb):.2f};  {n / min(rows['step']) * 1e6:.3g} env-steps/s")
    print(f"  rollout({k}, trajectory) {rng(rows['roll'])} us/step   moves {rb:.1f} B/env-step (obs {obs} + reward 4 + flag 1 + action 4 + generator {DRAWN + TWIST} + "
          f"(record in + out + 12) / {k}); as a copy: {copy_us(rb):.1f} us; ratio {min(rows['roll']) / copy_us(rb):.2f} - {max(rows['roll']) / copy_us(rb):.2f};  "
          f"{n / min(rows['roll']) * 1e6:.3g} env-steps/s;  trajectory buffer {k * n * obs / 2**30:.1f} GiB")


def caveat_actions(n):
    return np.ascontiguousarray(np.stack([common.hash_actions_np(A_SEED, np.arange(n, dtype=np.uint64), t, 45, 0) for t in range(STEPS)]), np.int32)


def host_record(n, path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probes", "farm_host_check.py"), "--record", "0", str(n), str(STEPS)],
                         input=caveat_actions(n).tobytes(), capture_output=True, check=True)
    assert len(out.stdout) == n * 89 * 8
    with open(path, "wb") as f:
        f.write(out.stdout)
    print(f"wrote {path}: {n} records of 89 float64")


def log_caveat(n, host_file):
    import custom_gymnasium_environments_amd as cge
    host = np.fromfile(host_file, np.uint64).reshape(n, 89)
    env = cge.AgriculturalFarmVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=0)
    env.rollout(STEPS, action_seed=A_SEED)                                   # the same hashed actions as caveat_actions()
    dev = lane_timing.float64_columns(env.snapshot(), n, RECORD, 89)        # the 89 float64 of each env
    diff = dev != host
    ulp = np.abs(dev.astype(np.int64) - host.astype(np.int64))[diff]
    prices = diff[:, 65:75]
    print(f"log caveat: {int(diff.sum())} of {diff.size} float64 record values differ between the device and the host build after reset(seed) and {STEPS} hashed "
          f"steps, seeds 0..{n - 1}, in {int(diff.any(1).sum())} envs; {int(prices.sum())} of them are prices (columns 65..74), the others cash_flow, total_revenue, "
          f"profit_margin or the cached Gaussian; largest distance {int(ulp.max()) if len(ulp) else 0} ulp")
    for i in np.flatnonzero(diff.any(1))[:8]:
        for c in np.flatnonzero(diff[i])[:2]:
            print(f"  seed {i} column {c}: device {dev[i, c]:#018x} host {host[i, c]:#018x}")
    print("columns that differ:", sorted(set(np.nonzero(diff)[1].tolist())))
    env.close()


if __name__ == "__main__":
    ap = lane_timing.parser(32)
    ap.add_argument("--log-caveat", type=int, default=0)
    ap.add_argument("--host-file", default=None)
    ap.add_argument("--host-record", default=None)
    args = ap.parse_args()
    if args.host_record:
        host_record(args.log_caveat or 4096, args.host_record)
        sys.exit(0)
    if args.log_caveat:
        import torch
        assert torch.cuda.is_available(), "needs an MI355X"
        log_caveat(args.log_caveat, args.host_file)
        sys.exit(0)
    copy_gbs = lane_timing.header(library=True)
    for n in args.sizes:
        run(n, args.runs, copy_gbs, args.k, False)
    run(max(args.sizes), args.runs, copy_gbs, args.k, True)
