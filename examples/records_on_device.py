"""Records on the device: overwrite the worse half of a batch with the better half, as population-based training does, and go on.

    python examples/records_on_device.py     (needs an MI355X; build first: python -m custom_gymnasium_environments_amd.build)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import custom_gymnasium_environments_amd as cge  # noqa: E402

N, K = 1 << 14, 30
env = cge.EmergencyVectorEnv(N, device="cuda:0", autoreset_mode="SameStep")
env.reset(seed=0)
_, score, _ = env.rollout(K, action_seed=1)                   # float64 [N]: each env's reward over K steps
order = torch.argsort(score, descending=True)
src, dst = order[:N // 2], order[N // 2:]                     # the better half, the worse half

rec = env.get_state(out="device")                             # uint8 [N, state_bytes] on the GPU: nothing goes through the host
rec[dst] = rec[src]                                           # state, episode clock and generator stream of each good env, twice
env.set_state(rec)                                            # checked on the device before a byte of the batch changes

_, again, _ = env.rollout(K, action_seed=2)                   # copies of one env now take different actions (the hash is per env index)
print(f"records: {rec.shape[1]} bytes per env, {rec.numel() / 2**20:.0f} MiB; mean reward over {K} steps before {float(score.mean()):.1f}, after {float(again.mean()):.1f}")
env.close()
