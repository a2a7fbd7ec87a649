"""WorldBuilderVectorEnv timing at 131,072 and 1,048,576 envs, SAME_STEP, device-resident random actions, both observation layouts:

  reset()     on its own
  step()      `--steps` calls (default 2,000) after a warm-up, device events around the run -> us per step
  rollout()   fused launches of K = 50 steps with the full trajectory (given actions) -> us per step

with the obliged bytes per env-step of each path, computed from the shapes (observation + reward + flag + action, plus the record read
and written for step(); a SAME_STEP step() also owes the terminal observations, which are NOT counted), and the fraction of this box's
device-to-device copy bandwidth they amount to (measured in this process, on 2-GiB torch buffers: bytes read + written per second).

  python tools/probes/world_builder_timing.py [--steps 2000]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import custom_gymnasium_environments_amd as cge  # noqa: E402
from lane_timing import copy_bandwidth, timed  # noqa: E402

K, WARMUP = 50, 200
STATE = 5 * 16 + 4                               # the record: five uint4 columns + the running return


def run(n, flat, steps, copy_gbs):
    env = cge.WorldBuilderVectorEnv(n, autoreset_mode="SameStep", flatten_obs=flat, reuse_buffers=True)
    obs_bytes = int(np.prod(env._obs_shape)) * (4 if flat else 1) / n        # per env: the flat row, or the env's share of the slab
    step_bytes = obs_bytes + 4 + 1 + 4 + 2 * STATE                           # obs, reward, terminated, action, record in and out
    roll_bytes = obs_bytes + 4 + 1 + 4 + (2 * STATE + 8 + 4) / K             # per step; record, reward_sum, done_count per launch
    acts = env.action_sampler(seed=0).sample(steps=K)                        # [K, n] device-resident actions, cycled
    env.reset(seed=1)
    resets = [timed(lambda: env.reset()) for _ in range(5)]
    for t in range(WARMUP):
        env.step(acts[t % K])
    step_us = float(np.median([timed(lambda: [env.step(acts[t % K]) for t in range(steps // 4)]) / (steps // 4) for _ in range(4)]))
    step_kernel = env.last_kernel()
    env.rollout(K, actions=acts, trajectory=True, per_step=True)
    roll_us = float(np.median([timed(lambda: env.rollout(K, actions=acts, trajectory=True, per_step=True)) / K for _ in range(8)]))
    gb = lambda bytes_per, us: bytes_per * n / (us * 1e-6) / 1e9  # noqa: E731
    print(f"n_envs {n}  {'flat float32 rows' if flat else 'Dict slab'}  (kernels: {step_kernel}, {env.last_kernel()}; device bytes {env.device_bytes() / 2**20:.0f} MiB)")
    print(f"  reset()                         {float(np.median(resets)):10.1f} us")
    print(f"  step()   {steps} steps          {step_us:10.2f} us/step   obliged {step_bytes:.1f} B/env-step = {gb(step_bytes, step_us):7.1f} GB/s = "
          f"{gb(step_bytes, step_us) / copy_gbs:.3f} of copy")
    print(f"  rollout({K}, trajectory)        {roll_us:10.2f} us/step   obliged {roll_bytes:.1f} B/env-step = {gb(roll_bytes, roll_us):7.1f} GB/s = "
          f"{gb(roll_bytes, roll_us) / copy_gbs:.3f} of copy")
    env.close()
    del env, acts
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    copy_gbs = copy_bandwidth(dev)
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device-to-device copy (2-GiB buffers, read + written): {copy_gbs:.0f} GB/s")
    print("times: device events around work that ends in a synchronise; device-resident int32 actions, reuse_buffers=True, SameStep")
    for n in args.sizes:
        for flat in (False, True):
            run(n, flat, args.steps, copy_gbs)
