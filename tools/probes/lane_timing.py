"""The shared part of tools/probes/{airline,emergency,space_station,farm}_timing.py: the copy bandwidth of the box, device-event timing,
the measurement loop over reset(), step() and rollout(), the header lines, the common options and the float64 columns of a snapshot.
A type's probe keeps its byte constants, its roll_bytes() and the wording of its three report lines.  copy_bandwidth() and timed() also
serve the timing probes of the other env types.  Not a program of its own."""
import argparse
import os

import numpy as np
import torch


def copy_bandwidth(dev):
    x = torch.empty(1 << 29, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    y.copy_(x)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(8):
        y.copy_(x)
    b.record()
    torch.cuda.synchronize(dev)
    gbs = 2 * x.numel() * 4 / 1e9 / (a.elapsed_time(b) / 8 * 1e-3)
    del x, y
    torch.cuda.empty_cache()
    return gbs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def rng(v):
    return f"{min(v):9.2f} - {max(v):9.2f}"


def measure(make_env, n, k, count, runs, calls=None, label=""):
    """-> {"reset": us of reset(), "step": us per step() call, "roll": us per rollout step}, a list of `runs` each, of the env that
    make_env() builds, and prints the line on n, the two kernels and the device bytes.  The actions are device-resident int32 [k, n],
    uniform over 0..count-1.  A run is reset(seed), a timed reset(), `calls` timed step() calls over acts[t % k] (k of them by
    default), a reset() and a timed rollout(k) with the full trajectory and per-step outputs on the same actions.  Seeding is not part
    of the timed reset."""
    env = make_env()
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = (torch.rand((k, n), generator=g, device="cuda") * count).to(torch.int32)
    calls = calls or k
    rows = {"reset": [], "step": [], "roll": []}
    for ep in range(runs + 1):                                   # the first run warms up (buffers, code objects)
        env.reset(seed=ep)
        r = timed(lambda: env.reset())
        s = timed(lambda: [env.step(acts[t % k]) for t in range(calls)])
        step_kernel = env.last_kernel()
        env.reset()
        roll = timed(lambda: env.rollout(k, actions=acts, trajectory=True, per_step=True))
        if ep:
            rows["reset"].append(r); rows["step"].append(s / calls); rows["roll"].append(roll / k)
    print(f"n_envs {n}{label}  (kernels: {step_kernel}, {env.last_kernel()}; device bytes {env.device_bytes() / 2**20:.0f} MiB; ranges over {runs} runs)")
    env.close()
    del env, acts
    torch.cuda.empty_cache()
    return rows


def parser(k):
    """the options every probe has"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--k", type=int, default=k)
    return ap


def header(library=False):
    """prints the two lines on the box and the method; -> its device-to-device copy rate in GB/s"""
    assert torch.cuda.is_available(), "needs an MI355X"
    copy_gbs = copy_bandwidth(torch.device("cuda:0"))
    lib = f" library {os.environ.get('CGE_AMD_LIBRARY', 'libcge_amd.so')};" if library else ""
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__};{lib} device-to-device copy (2-GiB buffers, read + written): {copy_gbs:.0f} GB/s")
    print("times: device events around work that ends in a synchronise; device-resident int32 actions, reuse_buffers=True, SameStep")
    return copy_gbs


def float64_columns(snap, n, record_bytes, count):
    """the first `count` float64 of each env's record, as uint64 [n, count], from snapshot() bytes: the record's columns [word][env] lie
    behind the 32-byte header"""
    rec = snap[32:32 + record_bytes * n].view(np.uint32).reshape(record_bytes // 4, n)
    return (rec[0:2 * count:2].astype(np.uint64) | rec[1:2 * count:2].astype(np.uint64) << np.uint64(32)).T
