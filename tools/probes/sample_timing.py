"""Device action sampling vs the host `action_space.sample()` at the 1,048,576-env snake batch (sampling.py, csrc/sample.hip).

  python tools/probes/sample_timing.py                 host sample + upload, sampler call, step(sampler.sample(out=buf)) vs
                                                       step(fixed buf), eager and as 16-step captured graphs
  python tools/probes/sample_timing.py --kernels N     only N sampler launches of every kind (run it under
                                                       `rocprofv3 --kernel-trace --stats` for the kernels' own times)

Times are device events around work that ends in a synchronise; each A/B pair alternates in one process."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import custom_gymnasium_environments_amd as cge  # noqa: E402
from custom_gymnasium_environments_amd._spaces import Box, MultiBinary  # noqa: E402

N = 1 << 20


def events_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels_only(n_calls):
    env = cge.SnakeVectorEnv(N, grid_size=10)
    s = env.action_sampler(seed=0)
    buf = s.sample()
    others = [cge.DeviceSpaceSampler(Box(-1.0, 1.0, (N, 2), np.float32), "cuda:0", seed=1),
              cge.DeviceSpaceSampler(Box(0, 1, (N, 4), np.int8), "cuda:0", seed=2),
              cge.DeviceSpaceSampler(MultiBinary((N, 4)), "cuda:0", seed=3)]
    obufs = [o.sample() for o in others]
    for _ in range(n_calls):
        s.sample(out=buf)
        for o, ob in zip(others, obufs):
            o.sample(out=ob)
    torch.cuda.synchronize()
    print("kernels:", s.last_kernel(), *[o.last_kernel() for o in others])


def main():
    env = cge.SnakeVectorEnv(N, grid_size=10, reuse_buffers=True)
    env.reset(seed=0)
    space = env.action_space
    space.seed(0)
    # host: action_space.sample() + the upload / int32 conversion step() does with it
    host_ms, up_ms = [], []
    for _ in range(12):
        t0 = time.perf_counter()
        a = space.sample()
        t1 = time.perf_counter()
        d = torch.as_tensor(a, device=env.device).to(torch.int32)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host_ms.append((t1 - t0) * 1e3)
        up_ms.append((t2 - t1) * 1e3)
    print(f"host action_space.sample() at {N} envs: median {np.median(host_ms[2:]):.2f} ms; upload + int32 conversion: median {np.median(up_ms[2:]):.2f} ms "
          f"({a.nbytes / 2**20:.0f} MiB int64)")

    s = env.action_sampler(seed=0)
    buf = s.sample()
    fixed = buf.clone()
    print(f"sampler.sample(out=buf), {N} int32: {events_us(lambda: s.sample(out=buf), 500):.2f} us per call (events, back-to-back)")
    step_fixed = lambda: env.step(fixed)                                   # noqa: E731
    step_sampled = lambda: env.step(s.sample(out=buf))                     # noqa: E731
    for f in (step_fixed, step_sampled):
        events_us(f, 50)
    rows = {"step(fixed buf)": [], "step(sampler.sample(out=buf))": []}
    for _ in range(5):
        rows["step(fixed buf)"].append(events_us(step_fixed, 200))
        rows["step(sampler.sample(out=buf))"].append(events_us(step_sampled, 200))
    for k, v in rows.items():
        print(f"eager {k:32s} median {np.median(v):8.2f} us per step  (5 x 200 steps: {', '.join(f'{x:.2f}' for x in v)})")
    ratio = np.median(rows["step(sampler.sample(out=buf))"]) / np.median(rows["step(fixed buf)"])
    print(f"eager ratio sampled / fixed: {ratio:.3f}")

    # the same two loops as 16-step captured graphs (no host launch cost per step)
    graphs = {}
    for name, f in (("step(fixed buf)", step_fixed), ("step(sampler.sample(out=buf))", step_sampled)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            f()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(16):
                f()
        graphs[name] = g
    grows = {k: [] for k in graphs}
    for g in graphs.values():
        events_us(g.replay, 5)
    for _ in range(5):
        for k, g in graphs.items():
            grows[k].append(events_us(g.replay, 20) / 16)
    for k, v in grows.items():
        print(f"graph {k:32s} median {np.median(v):8.2f} us per step  (5 x 20 replays of 16: {', '.join(f'{x:.2f}' for x in v)})")
    gratio = np.median(grows["step(sampler.sample(out=buf))"]) / np.median(grows["step(fixed buf)"])
    print(f"graph ratio sampled / fixed: {gratio:.3f}")
    env.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if args.kernels:
        kernels_only(args.kernels)
    else:
        main()
