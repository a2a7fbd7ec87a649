"""AirlineVectorEnv timing over whole episodes from a reset, at 131,072 and 1,048,576 envs, SAME_STEP, modelled on restaurant_timing.py:

  reset()      on its own (about 270 generator words per env, 150 flight words rewritten)
  step()       71 calls with device-resident actions (uniform over 0..44), device events around the episode -> us per step
  rollout(71)  one fused launch with the full trajectory and per-step outputs (the same actions, given) -> us per step

five runs each, reported as ranges, with the bytes each path moves per env-step, spelled out from the layout,
the time a device-to-device copy of the same bytes takes on this box (measured in this process on 2-GiB torch buffers: bytes read +
written per second) and the ratio of the kernel time to it.

  python tools/probes/airline_timing.py [--runs 5] [--sizes ...] [--k 71]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import custom_gymnasium_environments_amd as cge  # noqa: E402
from bus_timing import copy_bandwidth, timed  # noqa: E402

EPISODE = 71
OBS = 160 * 4
LOADED = (25 + 30 + 30 + 15 + 30 + 14) * 4       # what a launch loads of the record: aircraft words, gates, prices, severities, weather, scalars
STORED = (25 + 30 + 15 + 30 + 14) * 4            # ... and stores (prices only after a reset)
PER_STEP = 150 * 4 + 25 * 8 + 25 * 8 + 10 * 8    # read by every step: the flight words, maintenance bases, fuel levels and the ten scheduled times
STEP_BYTES = OBS + 4 + 1 + 4 + LOADED + STORED + PER_STEP


def roll_bytes(k):
    return OBS + 4 + 1 + 4 + PER_STEP + (LOADED + STORED + 12) / k


def rng(v):
    return f"{min(v):9.2f} - {max(v):9.2f}"


def run(n, runs, copy_gbs, k):
    env = cge.AirlineVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = (torch.rand((k, n), generator=g, device="cuda") * 45).to(torch.int32)
    rows = {"reset": [], "step": [], "roll": []}
    for ep in range(runs + 1):                                   # the first run warms up (buffers, code objects)
        env.reset(seed=ep)                                       # seeding (the network draw) is not part of the timed reset
        r = timed(lambda: env.reset())
        steps = timed(lambda: [env.step(acts[t % k]) for t in range(EPISODE)])
        step_kernel = env.last_kernel()
        env.reset()
        roll = timed(lambda: env.rollout(k, actions=acts, trajectory=True, per_step=True))
        if ep:
            rows["reset"].append(r); rows["step"].append(steps / EPISODE); rows["roll"].append(roll / k)
    copy_us = lambda b: b * n / (copy_gbs * 1e9) * 1e6           # noqa: E731
    rb = roll_bytes(k)
    print(f"n_envs {n}  (kernels: {step_kernel}, {env.last_kernel()}; device bytes {env.device_bytes() / 2**20:.0f} MiB; ranges over {runs} runs)")
    print(f"  reset()                {rng(rows['reset'])} us")
    print(f"  step()   71 calls      {rng(rows['step'])} us/step   moves {STEP_BYTES} B/env-step (obs {OBS} + reward 4 + flag 1 + action 4 + record in {LOADED} "
          f"+ out {STORED} + per-step reads {PER_STEP}); the same bytes as a copy: {copy_us(STEP_BYTES):.1f} us; ratio {min(rows['step']) / copy_us(STEP_BYTES):.2f} - "
          f"{max(rows['step']) / copy_us(STEP_BYTES):.2f}")
    print(f"  rollout({k}, trajectory) {rng(rows['roll'])} us/step   moves {rb:.1f} B/env-step (obs {OBS} + reward 4 + flag 1 + action 4 + per-step reads {PER_STEP} + "
          f"(record in + out + 12) / {k}); as a copy: {copy_us(rb):.1f} us; ratio {min(rows['roll']) / copy_us(rb):.2f} - {max(rows['roll']) / copy_us(rb):.2f};  "
          f"trajectory buffer {k * n * OBS / 2**30:.1f} GiB")
    env.close()
    del env, acts
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--k", type=int, default=EPISODE)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    copy_gbs = copy_bandwidth(torch.device("cuda:0"))
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device-to-device copy (2-GiB buffers, read + written): {copy_gbs:.0f} GB/s")
    print("times: device events around work that ends in a synchronise; device-resident int32 actions, reuse_buffers=True, SameStep")
    for n in args.sizes:
        run(n, args.runs, copy_gbs, args.k)
