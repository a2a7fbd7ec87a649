"""Phase clocks of crypto's two-wave resident rollout (build with -DCGE_CRYPTO_TIMING).  No waits are inserted: the clocks sit at
the barriers that are there anyway.

usage: [CGE_AMD_LIBRARY=tools/ab/libcge_<name>.so] python tools/probes/crypto_timing.py [--wall N_ENVS [CALLS [ROUNDS]]]
--wall: no phase clocks (any build): us per step() call of N_ENVS envs between two events around CALLS back-to-back calls with
reuse_buffers=True, the same measured again from a captured graph of 50 calls; ROUNDS rounds, each printed."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import custom_gymnasium_environments_amd as cge
from custom_gymnasium_environments_amd import _native


def wall(n, calls=2000, rounds=5):
    env = cge.CryptoVectorEnv(n, device="cuda:0", reuse_buffers=True)
    env.reset(seed=1)
    acts = torch.randint(0, 5, (50, n), dtype=torch.int32, device="cuda")
    for t in range(200):
        env.step(acts[t % 50])
    g = torch.cuda.CUDAGraph()                                 # 50 calls = one length of the candle ring
    with torch.cuda.graph(g):
        for t in range(50):
            env.step(acts[t])
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds):
        a.record()
        for t in range(calls):
            env.step(acts[t % 50])
        b.record(); torch.cuda.synchronize()
        eager = a.elapsed_time(b) * 1e3 / calls
        a.record()
        for t in range(calls // 50):
            g.replay()
        b.record(); torch.cuda.synchronize()
        print(f"{os.path.basename(_native.LIB_PATH)} {n} envs round {r}: step() {eager:7.2f} us per call eager, {a.elapsed_time(b) * 1e3 / (calls // 50 * 50):7.2f} us in a replayed graph", flush=True)
    env.close()


if "--wall" in sys.argv:
    wall(*[int(x) for x in sys.argv[sys.argv.index("--wall") + 1:]])
    sys.exit(0)
L = ctypes.CDLL(_native.LIB_PATH)
env = cge.CryptoVectorEnv(1 << 20, device="cuda:0")
env.reset(seed=1)
buf = (ctypes.c_ulonglong * 16)()
names = ["A: first half, rest (ready-mark twist, next words' load issue)", "A: waiting at bar1", "A: second half (price, candle) + publish + bar2", "A: per-step outputs", "B: waiting for window(t) (bar1 + bar2)", "B: observation of step t", "C: ratio rows of step t (issue time, stores not awaited)"]
import sys
acts = torch.randint(0, 5, (16, 1 << 20), dtype=torch.int32, device="cuda")
for chunk in range(4):
    if chunk < 2:
        env.rollout(16, action_seed=7, t0=chunk * 16, trajectory=True)
    else:                                  # the step() entry (resident_kernel<true>, k = 1)
        for t in range(16):
            env.step(acts[t])
    torch.cuda.synchronize()
    L.cge_crypto_debug_timing(buf, 1)
    n = max(1, buf[15])
    print(f"{'rollout' if chunk < 2 else 'step()'} steps {chunk*16}..{chunk*16+15}: workgroup-steps {buf[15]}")
    for k, nm in ((8, 'A: first half, action (hash / load)'), (9, 'A: first half, waiting for the step\'s generator words'), (10, 'A: first half, trade + draws (market_step)')):
        print(f"   {nm:44s} {buf[k] * 10.0 / n / 1e3:8.2f} us")
    for k, nm in enumerate(names):
        print(f"   {nm:44s} {buf[k] * 10.0 / n / 1e3:8.2f} us")
