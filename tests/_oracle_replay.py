"""Replays on the CPU oracles alone everything the GPU tests feed them: every run of tests/_action_streams.py (REPLAYS), the reference
fixtures the GPU tests replay (FIXTURES) and the directed scenarios (tests/_directed_scenarios.py).

    python tests/_oracle_replay.py ORACLE_PARENT_DIR [streams] [fixtures] [scenarios]

imports `oracle` from ORACLE_PARENT_DIR (test_oracle_branch_coverage.py passes a copy built with --coverage) and runs the named
parts, all three by default.  Nothing is asserted about the dynamics here; the scenarios assert that their event happened."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def replay_streams(oracle):
    import _action_streams as S
    for rid, stream, env, okw, n, T, seed0, mode, skw, hash_rollout in S.REPLAYS:
        o = S.make_oracle(oracle, env, okw, n, S.MODES[mode])
        o.seed(np.arange(n, dtype=np.uint64) + np.uint64(seed0))
        o.reset()
        if stream is not None:
            ctor = {k: v for k, v in okw.items() if k != "max_steps"}
            for a in S.STREAMS[stream](env, ctor, n, T, **skw):
                S.orc_step(o, a, want_final=mode == "SameStep")
        if hash_rollout is not None:
            a_seed, t0, env0, k = hash_rollout
            o.rollout(k, a_seed, t0=t0, env0=env0)


def replay_fixtures(oracle):
    import _action_streams as S
    for env, names in S.FIXTURES.items():
        for name in names:
            with np.load(os.path.join(HERE, "golden", name), allow_pickle=False) as z:
                fx = {k: z[k] for k in z.files}
            ctor = json.loads(str(fx["ctor"])) if "ctor" in fx else {}
            n = (fx["ac_temp"] if env == "climate" else fx["actions"]).shape[0]
            if env == "snake":
                o = oracle.SnakeOracle(n, int(fx["grid"]), oracle.SAME_STEP, max_steps=int(fx["max_steps"]))
            elif env == "crypto":
                o = oracle.CryptoOracle(n, str(fx["kind"]), oracle.SAME_STEP, config=json.loads(str(fx["config"])) if "config" in fx else None)
            elif env == "climate":
                o = oracle.ClimateOracle(n, oracle.SAME_STEP, max_steps=ctor.get("episode_minutes"), max_occupancy=ctor.get("max_occupancy"))
            else:
                o = getattr(oracle, S.ENV_TYPES[env][0])(n, oracle.SAME_STEP, **ctor)
            o.seed(np.arange(n, dtype=np.uint64) + np.uint64(int(fx["seed0"])))
            o.reset()
            if env == "climate":
                for t in range(fx["ac_temp"].shape[1]):
                    o.step(fx["ac_temp"][:, t], fx["lights"][:, t], want_final=True)
            else:
                for t in range(fx["actions"].shape[1]):
                    o.step(np.ascontiguousarray(fx["actions"][:, t]), want_final=True)


def replay_scenarios(oracle):
    import _directed_scenarios as D
    for scn in D.SCENARIOS:
        for mode in (oracle.SAME_STEP, oracle.NEXT_STEP):
            run = D.run_oracle(oracle, scn, mode)
            assert run["hit"].any(), f"scenario {scn.name}: the event '{scn.event}' happened in no env"


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import oracle as orc
    assert os.path.dirname(os.path.abspath(orc.__file__)) == os.path.join(os.path.abspath(sys.argv[1]), "oracle"), orc.__file__
    orc.lib()
    parts = sys.argv[2:] or ["streams", "fixtures", "scenarios"]
    for p in parts:
        {"streams": replay_streams, "fixtures": replay_fixtures, "scenarios": replay_scenarios}[p](orc)
