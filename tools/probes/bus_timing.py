"""BusVectorEnv timing over whole episodes from a reset (as `bench.py --episode` does for the other env types), at 131,072 and
1,048,576 envs, SAME_STEP:

  step()      500 calls with device-resident actions, device events around the episode -> us per step; the 500th call, which
              carries the in-kernel reset of every env (all envs hit the time limit in the same step), timed on its own, and
              reset() on its own
  rollout()   4 fused launches of 125 steps with the full trajectory (hash actions) -> us per step; the 4th launch holds the reset

with the obliged bytes per env-step of each path and the fraction of this box's device-to-device copy bandwidth they amount to
(measured in this process, on 2-GiB torch buffers: bytes read + written per second, like bench.py's roofline.peak_copy_measured).

  python tools/probes/bus_timing.py [--episodes 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import custom_gymnasium_environments_amd as cge  # noqa: E402
from lane_timing import copy_bandwidth, timed  # noqa: E402

LIMIT, K = 500, 125
# obliged bytes per env-step: what the call must read and write at least once
STATE = 3 * 16                                   # the record: three uint4 columns
OBS = 56 * 4                                     # one slab piece
STEP_BYTES = STATE + 16 + STATE + OBS + 4 + 1 + 1              # record in, actions in, record out, obs, reward, terminated, truncated
ROLL_BYTES = OBS + 4 + 1 + (2 * STATE + 8 + 4) / K            # obs + reward + truncated per step; record, reward_sum, done_count per launch


def run(n, episodes, copy_gbs):
    env = cge.BusVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    acts = env.action_sampler(seed=0).sample(steps=8)            # [8, n, 4] device-resident dwell times, cycled
    rows = {"reset": [], "step_episode": [], "step_plain": [], "step_reset": [], "roll_episode": [], "roll_plain": [], "roll_reset": []}
    for ep in range(episodes + 1):                               # the first episode warms up (buffers, code objects)
        env.reset(seed=ep)                                       # seeding is not part of the timed reset
        r = timed(lambda: env.reset())
        plain = timed(lambda: [env.step(acts[t & 7]) for t in range(LIMIT - 1)])
        last = timed(lambda: env.step(acts[(LIMIT - 1) & 7]))
        ro = timed(lambda: env.reset())
        launches = [timed(lambda j=j: env.rollout(K, action_seed=ep, t0=j * K, trajectory=True, per_step=True)) for j in range(LIMIT // K)]
        if ep:
            rows["reset"] += [r, ro]
            rows["step_episode"].append((plain + last) / LIMIT); rows["step_plain"].append(plain / (LIMIT - 1)); rows["step_reset"].append(last)
            rows["roll_episode"].append(sum(launches) / LIMIT); rows["roll_plain"].append(sum(launches[:-1]) / (LIMIT - K))
            rows["roll_reset"].append(launches[-1] - sum(launches[:-1]) / (len(launches) - 1))
    med = {k: float(np.median(v)) for k, v in rows.items()}
    gb = lambda bytes_per, us: bytes_per * n / (us * 1e-6) / 1e9  # noqa: E731
    print(f"n_envs {n}  (kernels: {env.last_kernel()}; device bytes {env.device_bytes() / 2**20:.0f} MiB; medians of {episodes} episodes)")
    print(f"  reset()                         {med['reset']:10.1f} us")
    print(f"  step()   whole episode          {med['step_episode']:10.2f} us/step   obliged {STEP_BYTES} B/env-step = {gb(STEP_BYTES, med['step_episode']):7.1f} GB/s = "
          f"{gb(STEP_BYTES, med['step_episode']) / copy_gbs:.3f} of copy")
    print(f"  step()   steps 1..499           {med['step_plain']:10.2f} us/step   {gb(STEP_BYTES, med['step_plain']):7.1f} GB/s = {gb(STEP_BYTES, med['step_plain']) / copy_gbs:.3f} of copy")
    print(f"  step()   step 500 (with reset)  {med['step_reset']:10.1f} us")
    print(f"  rollout(125, trajectory) whole episode {med['roll_episode']:8.2f} us/step   obliged {ROLL_BYTES:.1f} B/env-step = {gb(ROLL_BYTES, med['roll_episode']):7.1f} GB/s = "
          f"{gb(ROLL_BYTES, med['roll_episode']) / copy_gbs:.3f} of copy")
    print(f"  rollout  launches 1..3          {med['roll_plain']:10.2f} us/step   {gb(ROLL_BYTES, med['roll_plain']):7.1f} GB/s = {gb(ROLL_BYTES, med['roll_plain']) / copy_gbs:.3f} of copy")
    print(f"  rollout  the reset inside launch 4 (launch 4 - mean of launches 1..3)  {med['roll_reset']:10.1f} us")
    env.close()
    del env, acts
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    copy_gbs = copy_bandwidth(dev)
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device-to-device copy (2-GiB buffers, read + written): {copy_gbs:.0f} GB/s")
    print("times: device events around work that ends in a synchronise; step() with device-resident int32 actions, reuse_buffers=True, SameStep")
    for n in args.sizes:
        run(n, args.episodes, copy_gbs)
