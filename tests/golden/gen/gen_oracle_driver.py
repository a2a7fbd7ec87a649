"""Recording of the CPU oracle's batch driver (create / seed / reset(mask) / step / rollout / episode_stats in the three
autoreset modes), taken from the oracle itself at the commit BEFORE the eight per-file drivers were folded into
oracle/orc_batch.h.  Unlike the other generators this one does not run the reference: the reference has no vector API, the
batch semantics are the build's own (oracle/orc_batch.h), and the recording pins them across refactors of the driver.

Script of one run (51 runs: the 17 CASES of tests/test_oracle_hash_rollout.py x NEXT_STEP, SAME_STEP, DISABLED):
  n = 12 envs, seeds arange(n) + 16, reset();
  72 calls of step() with the actions of _hash_actions.hash_actions(name, 0xBEEF, 72, 12, t0=77, env0=5), want_final=True in
  SAME_STEP; snake and discrete crypto get acts[7, 5] = -1 and acts[20, 2] = 9, the wrapper raises ValueError at those two
  steps and the run goes on; before step 16, reset(mask) with mask = arange(n) % 3 == 0;
  then episode_stats(), rollout(20, 0xBEEF + 1, t0=149, env0=5), episode_stats() again, get_state() where the type has it.
Each call contributes one sha256 (its first 64 bits, in hex) over the dtype name and the bytes of every array it returned
(last_reward64 included), or the ValueError's message.  tests/test_oracle_driver.py replays record() and compares whole lists
with tests/golden/oracle_driver.json.

Run from the repository root:  python tests/golden/gen/gen_oracle_driver.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(TESTS, "golden", "oracle_driver.json")

N, STEPS, A_SEED, T0, ENV0 = 12, 72, 0xBEEF, 77, 5
MASK_BEFORE, ROLLOUT_K, ROLLOUT_T0 = 16, 20, 149
BAD = ((7, 5, -1), (20, 2, 9))                       # (step, env, invalid action) for snake and discrete crypto
MODES = ("NEXT_STEP", "SAME_STEP", "DISABLED")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(a.dtype.name.encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def record_run(oracle, case, mode):
    """-> (list of one entry per call, int64[n] number of episodes each env finished within the stepped part)"""
    from _hash_actions import at, hash_actions
    from test_oracle_hash_rollout import CASES, make_oracle
    name, cls, kw, hkw = CASES[case]
    o = make_oracle(oracle, cls, kw, N, getattr(oracle, mode))
    o.seed(np.arange(N, dtype=np.uint64) + np.uint64(16))
    calls = ["reset " + digest(o.reset())]
    acts = hash_actions(name, A_SEED, STEPS, N, t0=T0, env0=ENV0, **hkw)
    if name == "snake" or (name == "crypto" and not hkw.get("continuous")):
        for t, i, a in BAD:
            acts[t, i] = a
    done = np.zeros(N, np.int64)
    final = dict(want_final=True) if mode == "SAME_STEP" else {}
    for t in range(STEPS):
        if t == MASK_BEFORE:
            calls.append("reset(mask) " + digest(o.reset(np.arange(N) % 3 == 0)))
        a = at(acts, t)
        try:
            out = o.step(*a, **final) if isinstance(a, tuple) else o.step(a, **final)
        except ValueError as err:
            calls.append(f"step {t} ValueError: {err}")
            continue
        done += (out[2] | out[3]).astype(np.int64)
        extra = (o.last_reward64,) if hasattr(o, "last_reward64") else ()
        calls.append(f"step {t} " + digest(*out, *extra))
    calls.append("episode_stats " + digest(*o.episode_stats()))
    calls.append("rollout " + digest(*o.rollout(ROLLOUT_K, A_SEED + 1, t0=ROLLOUT_T0, env0=ENV0)))
    calls.append("episode_stats " + digest(*o.episode_stats()))
    if hasattr(o, "get_state"):
        calls.append("get_state " + digest(o.get_state()))
    return calls, done


def record(oracle):
    """-> {"<case>/<mode>": [calls]} for all 51 runs; asserts the conditions the recording stands on."""
    from test_oracle_hash_rollout import CASES
    runs = {}
    for case in CASES:
        for mode in MODES:
            calls, done = record_run(oracle, case, mode)
            if mode != "DISABLED":
                assert done.min() >= 2, f"{case}/{mode}: an env finished only {done.min()} episode(s) within {STEPS} steps"
            runs[f"{case}/{mode}"] = calls
    assert len(runs) == 3 * len(CASES) == 51, len(runs)
    return runs


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(TESTS), TESTS]
    import oracle
    runs = record(oracle)
    assert runs == record(oracle), "the recording is not deterministic"
    with open(OUT, "w") as f:
        json.dump(runs, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(runs)} runs, {sum(len(c) for c in runs.values())} calls, {os.path.getsize(OUT)} bytes")
