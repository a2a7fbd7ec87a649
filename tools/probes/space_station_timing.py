"""SpaceStationVectorEnv timing from a reset, at 131,072 and 1,048,576 envs, SAME_STEP (loop, header and options: lane_timing.py):

  reset()      on its own (32 Gaussians and 24 uniforms, about 130 generator words per env)
  step()       k calls with device-resident actions (uniform over 0..39), device events around them -> us per step
  rollout(k)   one fused launch with the full trajectory and per-step outputs (the same actions, given) -> us per step

five runs each after a warm-up run, reported as ranges, with the bytes each path moves per env-step, spelled out from the layout
(DESIGN.md section 3.17), the time a device-to-device copy of the same bytes takes on this box (measured in this process on 2-GiB torch
buffers: bytes read + written per second) and the ratio of the kernel time to it.  CGE_AMD_LIBRARY selects the library, so the
-DCGE_STATION_LANE_ROWS variant is timed by a second process of the same call.  That variant was last buildable at commit 84dc52e.

`--log-caveat N`: no timing; resets N envs with seeds 0..N-1 and counts those whose float64 module state (the 32 values a reset draws
through log) differs anywhere from `--host-file`, the same values from the host build of the same header
(tools/probes/space_station_host_check.py --reset 0 N > file), read from snapshot() bytes.

  python tools/probes/space_station_timing.py [--runs 5] [--sizes ...] [--k 32] [--log-caveat N --host-file F]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import custom_gymnasium_environments_amd as cge  # noqa: E402
import lane_timing  # noqa: E402
from lane_timing import rng  # noqa: E402

OBS = 120 * 4
RECORD = 752                                     # loaded by every launch and stored by it: the whole record
WORDS = 26 + 16                                  # generator words of a step once the power cascade has begun (most steps of a run): the
                                                 # emergency test 2, twelve failure tests 24, eight thermal drifts 16
DRAWN = WORDS * 4
TWIST = WORDS * 12                               # ... and what twisting them ahead moves: word k and word k + 397 read, word k written
STEP_BYTES = OBS + 4 + 2 + 4 + 2 * RECORD + DRAWN + TWIST


def roll_bytes(k):
    return OBS + 4 + 1 + 4 + DRAWN + TWIST + (2 * RECORD + 12) / k


def run(n, runs, copy_gbs, k):
    make = lambda: cge.SpaceStationVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)   # noqa: E731
    rows = lane_timing.measure(make, n, k, 40, runs)
    copy_us = lambda b: b * n / (copy_gbs * 1e9) * 1e6           # noqa: E731
    rb = roll_bytes(k)
    print(f"  reset()                {rng(rows['reset'])} us")
    print(f"  step()   {k} calls      {rng(rows['step'])} us/step   moves {STEP_BYTES} B/env-step (obs {OBS} + reward 4 + flags 2 + action 4 + record in {RECORD} "
          f"+ out {RECORD} + generator words drawn {DRAWN} + twisted {TWIST}); the same bytes as a copy: {copy_us(STEP_BYTES):.1f} us; ratio "
          f"{min(rows['step']) / copy_us(STEP_BYTES):.2f} - {max(rows['step']) / copy_us(STEP_BYTES):.2f};  {n / min(rows['step']) * 1e6:.3g} env-steps/s")
    print(f"  rollout({k}, trajectory) {rng(rows['roll'])} us/step   moves {rb:.1f} B/env-step (obs {OBS} + reward 4 + flag 1 + action 4 + generator {DRAWN + TWIST} + "
          f"(record in + out + 12) / {k}); as a copy: {copy_us(rb):.1f} us; ratio {min(rows['roll']) / copy_us(rb):.2f} - {max(rows['roll']) / copy_us(rb):.2f};  "
          f"{n / min(rows['roll']) * 1e6:.3g} env-steps/s;  trajectory buffer {k * n * OBS / 2**30:.1f} GiB")


def log_caveat(n, host_file):
    host = np.fromfile(host_file, np.uint64).reshape(n, 32)
    env = cge.SpaceStationVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=0)
    dev = lane_timing.float64_columns(env.snapshot(), n, RECORD, 32)        # the 32 module float64 of each env
    diff = dev != host
    envs = np.flatnonzero(diff.any(1))
    print(f"log caveat: {len(envs)} of {n} envs (seeds 0..{n - 1}) hold a float64 module value after reset(seed) that differs from the host build's "
          f"({int(diff.sum())} of {diff.size} values)")
    for i in envs[:8]:
        for c in np.flatnonzero(diff[i])[:2]:
            print(f"  seed {i} column {c}: device {dev[i, c]:#018x} host {host[i, c]:#018x}")
    env.close()


if __name__ == "__main__":
    ap = lane_timing.parser(32)
    ap.add_argument("--log-caveat", type=int, default=0)
    ap.add_argument("--host-file", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if args.log_caveat:
        log_caveat(args.log_caveat, args.host_file)
        sys.exit(0)
    copy_gbs = lane_timing.header(library=True)
    for n in args.sizes:
        run(n, args.runs, copy_gbs, args.k)
