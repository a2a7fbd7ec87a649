"""EmergencyVectorEnv timing from a reset, at 131,072 and 1,048,576 envs, SAME_STEP (loop, header and options: lane_timing.py):

  reset()      on its own (2 to about 20 generator words per env)
  step()       k calls with device-resident actions (uniform over 0..49), device events around them -> us per step
  rollout(k)   one fused launch with the full trajectory and per-step outputs (the same actions, given) -> us per step

five runs each, reported as ranges, with the bytes each path moves per env-step, spelled out from the layout,
the time a device-to-device copy of the same bytes takes on this box (measured in this process on 2-GiB torch buffers: bytes read +
written per second) and the ratio of the kernel time to it.

  python tools/probes/emergency_timing.py [--runs 5] [--sizes ...] [--k 32]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import custom_gymnasium_environments_amd as cge  # noqa: E402
import lane_timing  # noqa: E402
from lane_timing import rng  # noqa: E402

OBS = 276 * 4
RECORD = 808                                     # loaded by every launch and stored by it: the whole record
DRAWN = 58 * 4                                   # the generator words every step draws at the least: arrival 2, weather 6, traffic 50
TWIST = 58 * 12                                  # ... and what twisting them ahead moves: word k and word k + 397 read, word k written
STEP_BYTES = OBS + 4 + 1 + 4 + 2 * RECORD + DRAWN + TWIST


def roll_bytes(k):
    return OBS + 4 + 1 + 4 + DRAWN + TWIST + (2 * RECORD + 12) / k


def run(n, runs, copy_gbs, k):
    make = lambda: cge.EmergencyVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)   # noqa: E731
    rows = lane_timing.measure(make, n, k, 50, runs)                  # seeding (the constructor's 952 randint) is not part of the timed reset
    copy_us = lambda b: b * n / (copy_gbs * 1e9) * 1e6           # noqa: E731
    rb = roll_bytes(k)
    print(f"  reset()                {rng(rows['reset'])} us")
    print(f"  step()   {k} calls      {rng(rows['step'])} us/step   moves {STEP_BYTES} B/env-step (obs {OBS} + reward 4 + flag 1 + action 4 + record in {RECORD} "
          f"+ out {RECORD} + generator words drawn {DRAWN} + twisted {TWIST}); the same bytes as a copy: {copy_us(STEP_BYTES):.1f} us; ratio "
          f"{min(rows['step']) / copy_us(STEP_BYTES):.2f} - {max(rows['step']) / copy_us(STEP_BYTES):.2f};  {n / min(rows['step']) * 1e6:.3g} env-steps/s")
    print(f"  rollout({k}, trajectory) {rng(rows['roll'])} us/step   moves {rb:.1f} B/env-step (obs {OBS} + reward 4 + flag 1 + action 4 + generator {DRAWN + TWIST} + "
          f"(record in + out + 12) / {k}); as a copy: {copy_us(rb):.1f} us; ratio {min(rows['roll']) / copy_us(rb):.2f} - {max(rows['roll']) / copy_us(rb):.2f};  "
          f"{n / min(rows['roll']) * 1e6:.3g} env-steps/s;  trajectory buffer {k * n * OBS / 2**30:.1f} GiB")


if __name__ == "__main__":
    args = lane_timing.parser(32).parse_args()
    copy_gbs = lane_timing.header()
    for n in args.sizes:
        run(n, args.runs, copy_gbs, args.k)
