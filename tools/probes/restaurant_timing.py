"""RestaurantVectorEnv timing over whole episodes from a reset, at 131,072 and 1,048,576 envs, SAME_STEP, modelled on bus_timing.py:

  reset()     on its own (no draws: a cleared record and a slab of zeros)
  step()      500 calls with device-resident packed actions (the fixtures' `busy` policy: customers are seated, served, tables cleaned),
              device events around the episode -> us per step
  rollout()   4 fused launches of 125 steps with the full trajectory and per-step outputs (the same policy, as given actions) -> us
              per step.  A 125-step trajectory of 1,048,576 envs is 179 GB; where the device cannot hold it the launches shrink
              (--k) and the line says so.

with the obliged bytes per env-step of each path, spelled out, and the fraction of this box's device-to-device copy bandwidth they
amount to (measured in this process, on 2-GiB torch buffers: bytes read + written per second).  Run tools/probes/bus_timing.py in the
same call for the nearest neighbour's figures on the same box.

  python tools/probes/restaurant_timing.py [--episodes 2] [--sizes ...] [--k 125]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import custom_gymnasium_environments_amd as cge  # noqa: E402
from lane_timing import copy_bandwidth, timed  # noqa: E402

LIMIT = 500
RECORD = 11 * 16                                 # the record: eleven uint4 columns
OBS = 341 * 4                                    # one env's piece of a slab
STEP_BYTES = OBS + 4 + 1 + 16 + 2 * RECORD + 8   # observation, reward, flag, actions, the record in and out, two generator words


def roll_bytes(k):
    """section 3.0: obs + reward + flag + the generator words, which stay in HBM, + per launch the record in and out, reward_sum, done_count;
    given actions add their 16 bytes per step"""
    return OBS + 4 + 1 + 8 + 16 + (2 * RECORD + 8 + 4) / k


def busy_actions(n, steps):
    """[steps, n, 4] int32 on the device: type and customer_id over 0..2, waiter_id and table_id over 0..9"""
    g = torch.Generator(device="cuda").manual_seed(0)
    hi = torch.tensor([3, 10, 3, 10], device="cuda")
    return (torch.rand((steps, n, 4), generator=g, device="cuda") * hi).to(torch.int32)


def run(n, episodes, copy_gbs, k):
    env = cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    acts = busy_actions(n, k)                                    # cycled: step t takes acts[t % k], rollout launch j the whole block
    while True:
        try:
            env.rollout(k, actions=acts[:k], trajectory=True, per_step=True)
            break
        except torch.cuda.OutOfMemoryError:                           # the trajectory does not fit: shorter launches
            env._bufs.pop("traj", None)
            torch.cuda.empty_cache()
            k //= 5
    rows = {"reset": [], "step_episode": [], "roll_episode": [], "roll_first": []}
    for ep in range(episodes + 1):                               # the first episode warms up (buffers, code objects)
        env.reset(seed=ep)                                       # seeding is not part of the timed reset
        r = timed(lambda: env.reset())
        steps = timed(lambda: [env.step(acts[t % k]) for t in range(LIMIT)])
        step_kernel = env.last_kernel()
        assert int(env.info("timestep")[0]) == 0                 # the 500th step reset every env
        env.reset()
        launches = [timed(lambda: env.rollout(k, actions=acts[:k], trajectory=True, per_step=True)) for j in range(LIMIT // k)]
        assert int(env.info("timestep")[0]) == 0
        if ep:
            rows["reset"].append(r)
            rows["step_episode"].append(steps / LIMIT)
            rows["roll_episode"].append(sum(launches) / LIMIT); rows["roll_first"].append(launches[0] / k)
    med = {key: float(np.median(v)) for key, v in rows.items()}
    gb = lambda bytes_per, us: bytes_per * n / (us * 1e-6) / 1e9  # noqa: E731
    rb = roll_bytes(k)
    print(f"n_envs {n}  (kernels: {step_kernel}, {env.last_kernel()}; device bytes {env.device_bytes() / 2**20:.0f} MiB; medians of {episodes} episodes)")
    print(f"  reset()                         {med['reset']:10.1f} us   (writes {OBS} B per env = {gb(OBS, med['reset']):7.1f} GB/s)")
    print(f"  step()   whole episode          {med['step_episode']:10.2f} us/step   obliged {STEP_BYTES} B/env-step (obs {OBS} + reward 4 + flag 1 + actions 16 + "
          f"2 x record {RECORD} + generator 8) = {gb(STEP_BYTES, med['step_episode']):7.1f} GB/s = {gb(STEP_BYTES, med['step_episode']) / copy_gbs:.3f} of copy")
    print(f"  rollout({k}, trajectory) whole episode {med['roll_episode']:8.2f} us/step   obliged {rb:.1f} B/env-step (obs {OBS} + reward 4 + flag 1 + generator 8 + "
          f"actions 16 + (2 x record + 12) / {k}) = {gb(rb, med['roll_episode']):7.1f} GB/s = {gb(rb, med['roll_episode']) / copy_gbs:.3f} of copy")
    print(f"  rollout  first launch (arrivals only begin: the emptiest slabs) {med['roll_first']:8.2f} us/step;  trajectory buffer {k * n * OBS / 2**30:.1f} GiB")
    env.close()
    del env, acts
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--k", type=int, default=125)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    copy_gbs = copy_bandwidth(dev)
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device-to-device copy (2-GiB buffers, read + written): {copy_gbs:.0f} GB/s")
    print("times: device events around work that ends in a synchronise; packed device-resident int32 actions, reuse_buffers=True, SameStep")
    for n in args.sizes:
        run(n, args.episodes, copy_gbs, args.k)
