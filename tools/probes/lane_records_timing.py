"""Timing of the canonical records of the four record-lane types (cge_records_<env>_*): pack and unpack on the device beside a
device-to-device copy of the same bytes measured in the same process, and the host forms get_state() / set_state() beside
snapshot() / restore() of the same handle.  The numbers of profiles/lane_records_timing.txt:

    python tools/probes/lane_records_timing.py > profiles/lane_records_timing.txt

unpack's time includes the check of every record and the wait for its verdict; both calls allocate nothing that outlives them."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import custom_gymnasium_environments_amd as cge  # noqa: E402
import lane_timing as lt  # noqa: E402

TYPES = (("airline", "AirlineVectorEnv"), ("emergency", "EmergencyVectorEnv"), ("space_station", "SpaceStationVectorEnv"), ("farm", "AgriculturalFarmVectorEnv"))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out      # ms


def main():
    ap = lt.parser(20)
    ap.add_argument("--host-sizes", type=int, nargs="*", default=[131072], help="batch sizes at which the host forms are timed as well")
    args = ap.parse_args()
    lt.header()
    print("pack / unpack: us per call over the whole batch, device-resident records; copy: torch copy_ of n * state_bytes bytes, same process")
    for kind, name in TYPES:
        for n in args.sizes:
            env = getattr(cge, name)(n, autoreset_mode="SameStep")
            env.reset(seed=1)
            env.rollout(args.k, action_seed=2)
            rec = env.get_state(out="device")
            other = torch.empty_like(rec)
            pack, unpack, copy = [], [], []
            for run in range(args.runs + 1):             # the first run warms up
                p = lt.timed(lambda: env.get_state(out=rec))
                u = lt.timed(lambda: env.set_state(rec))
                c = lt.timed(lambda: other.copy_(rec))
                if run:
                    pack.append(p); unpack.append(u); copy.append(c)
            mid = sorted(copy)[len(copy) // 2]
            print(f"{kind:14s} n_envs {n:8d}  state_bytes {rec.shape[1]}  records {rec.numel() / 2**20:7.0f} MiB   pack {lt.rng(pack)} us ({sorted(pack)[len(pack) // 2] / mid:5.2f} x copy)"
                  f"   unpack {lt.rng(unpack)} us ({sorted(unpack)[len(unpack) // 2] / mid:5.2f} x copy)   copy {lt.rng(copy)} us")
            if n in args.host_sizes:
                g, host = wall(env.get_state)
                s, _ = wall(lambda: env.set_state(host))
                sg, snap = wall(env.snapshot)
                ss, _ = wall(lambda: env.restore(snap))
                print(f"{'':14s} host forms, ms wall clock: get_state {g:8.1f}  set_state {s:8.1f}  ({host.nbytes / 2**20:.0f} MiB)   snapshot {sg:8.1f}  restore {ss:8.1f}  ({snap.nbytes / 2**20:.0f} MiB)")
                del host, snap
            env.close()
            del env, rec, other
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
