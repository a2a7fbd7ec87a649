"""Canonical get_state records of snake, crypto, traffic and the world builder, recorded from the device library itself.

Unlike the other generators this one needs an MI355X and the built library, and it was run ONCE, at the commit before the record
driver (csrc/cge_host.hpp: get_records / set_records) replaced the four hand-written get_state / set_state bodies: the fixtures
pin the driver to the bytes its predecessors wrote.  Do not regenerate them with a later library — that would compare the code
with itself.  tests/test_state_records_gpu.py imports CONFIGS, make, cursors_ok and replay from here.

Per config, 16 envs: seeded reset, a hash-action rollout of K steps, get_state(); then set_state() of those records into a fresh
env seeded differently, a 20-step hash rollout with per-step outputs, and get_state() again.  K is the first length from the
config's K0 on at which the cursors sit where the export has work to do (find_k); it is stored with the records.

    python tests/golden/gen/gen_state_records.py [OUT_DIR]        (default: tests/golden/state_records)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(os.path.dirname(HERE), "state_records")

N_ENVS, N_MT, TAIL = 16, 624, 20
SEED, SEED_FRESH, A_SEED = 1234, 99, 77

# name -> (env class, kwargs, K0, [(byte offset of the 624 words, byte offset of the int32 index)] of each generator stream)
CONFIGS = {
    "snake10": ("SnakeVectorEnv", dict(grid_size=10), 300, [(32, 28)]),
    "snake20": ("SnakeVectorEnv", dict(grid_size=20), 300, [(32, 28)]),
    "crypto_discrete": ("CryptoVectorEnv", dict(action_type="discrete"), 60, [(96, 16), (96 + 4 * N_MT, 20)]),
    "crypto_continuous": ("CryptoVectorEnv", dict(action_type="continuous"), 60, [(96, 16), (96 + 4 * N_MT, 20)]),
    "traffic": ("TrafficVectorEnv", {}, 40, [(32 + 64 * 9, 12)]),
    "world_builder": ("WorldBuilderVectorEnv", {}, 60, [(64 + 100, 52)]),
}


def make(cfg):
    import custom_gymnasium_environments_amd as cge
    cls, kw, _, _ = CONFIGS[cfg]
    return getattr(cge, cls)(N_ENVS, **kw)


def _i32(rec, off):
    return rec[:, off:off + 4].copy().view(np.int32)[:, 0]


def _u32(rec, off):
    return rec[:, off:off + 4].copy().view(np.uint32)[:, 0]


def twisted_ahead(cfg, rec):
    """per env: a generator block provably held words of the NEXT generation when it was exported.
    crypto: the export has no saved word 0, so a stream it took back reads word 0 with its dead low 31 bits zero (cge_host.hpp).
    traffic: a rollout keeps at least 49 twisted words parked beyond the cursor at the top of every step (traffic.hip: Draws::MINV)
    and a step consumes at most 32, so the ready mark ends at least 17 words past the cursor: a cursor in the generation's last
    16 words has a mark beyond 624."""
    streams = CONFIGS[cfg][3]
    if cfg.startswith("crypto"):
        return np.logical_or.reduce([(_u32(rec, w) & 0x7FFFFFFF) == 0 for w, _ in streams])
    if cfg == "traffic":
        idx = _i32(rec, streams[0][1])
        return (idx >= N_MT - 16) & (idx < N_MT)
    return np.zeros(len(rec), bool)


def cursors_ok(cfg, rec):
    """every stream has moved off word 0, and most cursors sit inside a generation"""
    idx = np.stack([_i32(rec, i) for _, i in CONFIGS[cfg][3]])
    inside = (idx > 0) & (idx < N_MT)
    if not ((idx > 0).all() and inside.mean() >= 0.75):
        return False
    return twisted_ahead(cfg, rec).any() if cfg.startswith("crypto") or cfg == "traffic" else True


def find_k(cfg):
    """the first K >= K0 whose records satisfy cursors_ok, each tried on a FRESH env (crypto's reset carries market state over from the
    handle's earlier episodes, so only a fresh env K steps after reset(seed=SEED) can be rebuilt by the test).  Returns (K, records)."""
    k0 = CONFIGS[cfg][2]
    for k in range(k0, k0 + 400):
        env = make(cfg)
        env.reset(seed=SEED)
        env.rollout(k, action_seed=A_SEED, want_obs=False)
        rec = env.get_state()
        env.close()
        if cursors_ok(cfg, rec):
            return k, rec
    raise AssertionError(f"{cfg}: no rollout length in {k0}..{k0 + 399} leaves the cursors where the export has work to do")


def _obs_bytes(env, obs):
    """the observation trajectory as one array (the world builder's Dict: the uint8 slab behind it)"""
    if isinstance(obs, dict):
        obs = env.obs_slab(obs)
    return obs.cpu().numpy()


def replay(cfg, rec, k):
    """records -> a fresh env with another seed -> get_state(), a TAIL-step hash rollout with per-step outputs, get_state()"""
    env = make(cfg)
    env.reset(seed=SEED_FRESH)
    env.set_state(rec)
    back = env.get_state()
    obs, rt, ft, rs, dc = env.rollout(TAIL, action_seed=A_SEED, t0=k, trajectory=True, per_step=True)
    out = dict(reexport=back, obs=_obs_bytes(env, obs), reward=rt.cpu().numpy(), flags=ft.cpu().numpy().astype(np.uint8),
               reward_sum=rs.cpu().numpy(), done_count=dc.cpu().numpy(), final=env.get_state())
    env.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    out_dir = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(out_dir, exist_ok=True)
    for cfg in CONFIGS:
        k, rec = find_k(cfg)
        assert cursors_ok(cfg, rec)
        d = replay(cfg, rec, k)
        path = os.path.join(out_dir, cfg + ".npz")
        np.savez_compressed(path, k=np.int64(k), records=rec, **d)
        idx = [_i32(rec, i).tolist() for _, i in CONFIGS[cfg][3]]
        print(f"{cfg}: K = {k}, record {rec.shape[1]} B, twisted ahead in {int(twisted_ahead(cfg, rec).sum())} envs, indices {idx}, "
              f"re-export equal: {np.array_equal(d['reexport'], rec)}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
