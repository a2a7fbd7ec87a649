"""bench.py end to end on the GPU at a small size (snake_64k): the --full line carries every field of the contract, the
roofline and cpu_baseline objects, the repeats' spread and the steady_state block; and the numbers are consistent with each other
(value = envs x K / wall, frac = achieved / peak, the steady state is not faster than physics allows).  A plain run times exactly K
steps once, carries the headline fields only, and its --dump-outputs files are the same from run to run and agree with the oracle.
A child process, as the driver runs it; the pytest process itself may already hold the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contracts_fields():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "CGE_BENCH_DRYRUN")}
    p = subprocess.run([sys.executable, "bench.py", "--workload", "snake_64k", "--steps", "10", "--warmup", "2", "--repeats", "3", "--steady-steps", "100", "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    n, K = 1 << 16, 10
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == K and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "i8" and d["data"] == "synthetic" and d["unit"] == "env-steps/s"
    assert d["config"]["workload"].startswith("snake_64k") and d["config"]["envs_per_gpu"] == n and "model" not in d["config"]
    assert d["value"] == pytest.approx(n * K / (d["ms_per_step"] * 1e-3 * K), rel=1e-9)
    sp = d["spread"]
    assert sp["repeats"] == 3 and len(sp["all_ms_per_step"]) == 3 and sp["min_ms_per_step"] <= d["ms_per_step"] <= sp["max_ms_per_step"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9) and 0.0 < r["frac"] < 1.0
    assert "snake::rollout_kernel" in r["kernel"] and r["avg_launch_us"] > 0
    assert r["traffic"] is None or r["traffic"] > 0
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_env_step"] * r["env_steps_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9, rel=1e-6)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "env-steps/s" and c["value"] > 0 and c["cores"] >= 1 and "orc_snake" in c["sample"]
    s = d["steady_state"]
    assert s["after_steps"] == 100 and s["value"] > 0 and 0.0 < s["frac"] < 1.0 and s["kernel"] == r["kernel"] and s["spread"]["repeats"] == 3
    a = d["api_step"]
    assert a["path"] == "step" and a["value"] > 0 and "snake::step_kernel" in a["roofline"]["kernel"]
    w = d["rollout_with_final_obs"]
    assert w["dropped_last_launch"] == 0 and w["delivered_last_launch"] > 0


def _plain_line(args, dump_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "CGE_BENCH_DRYRUN")}
    p = subprocess.run([sys.executable, "bench.py", "--workload", "snake_64k", *args, "--dump-outputs", str(dump_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["rollout", "step"])
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path, path):
    n, K = 1 << 16, 10
    dirs = [tmp_path / "a", tmp_path / "b"]
    for dump_dir in dirs:
        d = _plain_line(["--steps", str(K), "--warmup", "2", "--path", path], dump_dir)
        assert d["steps"] == K and d["spread"]["repeats"] == 1 and d["spread"]["all_ms_per_step"] == [d["ms_per_step"]]
        assert d["metric"].startswith("env steps/sec") and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "i8"
        assert d["value"] == pytest.approx(n * K / (d["ms_per_step"] * 1e-3 * K), rel=1e-9)
        for k in ("roofline", "phases", "api_step", "fused_rollout", "rollout_with_final_obs", "steady_state", "cpu_baseline"):
            assert k not in d, k
    names = sorted(os.listdir(dirs[0]))
    want = ({"obs", "reward", "flags", "reward_sum", "done_count"} if path == "rollout" else {"obs", "reward", "terminated", "truncated", "final_obs"})
    assert {f"snake_{k}.npy" for k in want | {"env_index"}} <= set(names) and names == sorted(os.listdir(dirs[1]))
    total = 0
    for f in names:
        a, b = np.load(dirs[0] / f), np.load(dirs[1] / f)
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == n and np.array_equal(a, b), f
        total += os.path.getsize(dirs[0] / f)
    assert total <= 64e6
    assert np.array_equal(np.load(dirs[0] / "snake_env_index.npy"), np.arange(n))    # 65,536 envs fit the budget whole


@pytest.mark.gpu
def test_dumped_rollout_is_what_the_oracle_computes(tmp_path, oracle):
    """The plain rollout run: a priming launch of K steps from reset(seed=0), max(W, 1) warm-up steps, the K timed steps; the dump
    holds the last timed step's observation and the timed launch's reward sum / episode ends."""
    n, K, W = 1 << 16, 10, 2
    _plain_line(["--steps", str(K), "--warmup", str(W)], tmp_path)
    ref = oracle.SnakeOracle(n, 10, oracle.SAME_STEP)
    ref.seed(np.arange(n, dtype=np.uint64))
    ref.reset()
    ref.rollout(K, 123, 0)
    ref.rollout(W, 123, K)
    obs, rs, dc = ref.rollout(K, 123, K + W)
    assert np.array_equal(np.load(tmp_path / "snake_obs.npy"), obs.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "snake_reward_sum.npy"), rs.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "snake_done_count.npy"), dc.astype(np.float64))
