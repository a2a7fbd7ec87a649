"""GPU parity tests for the traffic hot path (through the C ABI via TrafficVectorEnv): bit-exact obs
(float32), rewards (float32 of the bit-identical float64), flags and internal counters against the golden
vectors recorded from the reference and against the CPU oracle."""
import json

import numpy as np
import pytest
import torch

from conftest import golden
from _action_streams import RUNS, TRAFFIC_LAYOUTS, traffic_sparse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


def _np(t):
    return t.cpu().numpy()


# traffic_3x3 / traffic_6x6: the reference built the way its own scripts do (simple_test.py:71-76, USAGE_EXAMPLES.md:32-38)
@pytest.mark.parametrize("name", ["traffic_hash.npz", "traffic_lazy.npz", "traffic_3x3.npz", "traffic_6x6.npz"])
def test_same_step_matches_reference_fixture(cge, name):
    fx = golden(name)
    A = fx["actions"]
    n, T, ni = A.shape[0], A.shape[1], A.shape[2]
    ctor = json.loads(str(fx["ctor"])) if "ctor" in fx else {}
    env = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", **ctor)
    assert env.num_intersections == ni and env.obs_dim == fx["obs"].shape[2]
    obs, _ = env.reset(seed=int(fx["seed0"]))
    assert np.array_equal(_np(obs), fx["obs0"])
    reset_at = {(int(i), int(t)): k for k, (i, t) in enumerate(fx["reset_index"])}
    A_dev = torch.from_numpy(A).cuda()
    for t in range(T):
        obs, rew, te, tr, info = env.step(A_dev[:, t])
        obs, rew, te, fin = _np(obs), _np(rew), _np(te), _np(info["final_obs"])
        assert np.array_equal(te, fx["terminated"][:, t].astype(bool)), t
        assert np.array_equal(rew, fx["reward"][:, t].astype(np.float32)), (t, rew, fx["reward"][:, t])
        step_obs = np.where(te[:, None], fin, obs)
        assert np.array_equal(step_obs.view(np.uint32), fx["obs"][:, t].view(np.uint32)), t
        for i in np.nonzero(te)[0]:
            assert np.array_equal(obs[i], fx["reset_obs"][reset_at[(int(i), t)]])
        if t % 100 == 7:
            S, live = fx["internal"][:, t], ~te
            for it in range(ni):
                assert np.array_equal(_np(env.info("light_phase", it))[live], S[live, it * 8])
                assert np.array_equal(_np(env.info("light_timer", it))[live], S[live, it * 8 + 1])
                assert np.array_equal(_np(env.info("vehicles_passed", it))[live], S[live, it * 8 + 2])
                assert np.array_equal(_np(env.info("total_waiting_time", it))[live], S[live, it * 8 + 3])
            assert np.array_equal(_np(env.info("num_vehicles"))[live], S[live, 8 * ni])
    env.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_step_matches_oracle_all_modes(cge, oracle, mode):
    code = {"NextStep": oracle.NEXT_STEP, "SameStep": oracle.SAME_STEP, "Disabled": oracle.DISABLED}[mode]
    R = RUNS["traffic_all_modes"]
    n, T = R["n"], R["T"]
    env = cge.TrafficVectorEnv(n, autoreset_mode=mode, env_index0=R["env0"])
    o = oracle.TrafficOracle(n, code)
    o.seed(np.arange(n, dtype=np.uint64) + np.uint64(R["env0"] + R["seed"]))
    od, _ = env.reset(seed=R["seed"])
    assert np.array_equal(_np(od), o.reset())
    for t, a in enumerate(traffic_sparse("traffic", {}, n, T)):      # long stretches on the lights' own random timers
        od, rd, ted, trd, _ = env.step(a)
        oo, ro, teo, tro = o.step(a)
        assert np.array_equal(_np(od).view(np.uint32), oo.view(np.uint32)), t
        assert np.array_equal(_np(rd), ro) and np.array_equal(_np(ted), teo.astype(bool)), t
    assert np.array_equal(_np(env.total_reward()), o.total_reward())
    for f in ["timestep", "num_vehicles", "episodes", "needs_reset"]:
        assert np.array_equal(_np(env.info(f)), o.info(f)), f
    for q in range(36):
        for f in ["queue_len", "queue_dest", "queue_wait"]:
            assert np.array_equal(_np(env.info(f, q)), o.info(f, q)), (f, q)
    env.close()


LAYOUTS = TRAFFIC_LAYOUTS


@pytest.mark.parametrize("ctor", LAYOUTS, ids=lambda c: f"{c['grid_size'][0]}x{c['grid_size'][1]}_{c['num_intersections']}_{c['max_vehicles']}_{c['spawn_rate']}")
def test_layouts_and_knobs_match_oracle(cge, oracle, ctor):
    """Every constructor argument the reference takes (environment.py:62-83) against the oracle built with the same ones:
    step() with explicit actions in SameStep mode through a short time limit, then the fused rollout on top, a state round
    trip through the oracle, and the rollout's trajectory against step() on a twin."""
    R = RUNS["traffic_layouts"]
    n, limit = R["n"], R["limit"]
    env = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", env_index0=R["env0"], max_steps=limit, **ctor)
    o = oracle.TrafficOracle(n, oracle.SAME_STEP, max_steps=limit, **ctor)
    ni = env.num_intersections
    assert ni == o.ni and env.obs_dim == o.obs_dim == 14 * ni + 4
    assert env.single_action_space.nvec.shape == (ni,) and env.single_observation_space.shape == (env.obs_dim,)
    o.seed(np.arange(n, dtype=np.uint64) + np.uint64(R["env0"] + R["seed"]))
    od, _ = env.reset(seed=R["seed"])
    assert np.array_equal(_np(od), o.reset())
    for t, a in enumerate(traffic_sparse("traffic", ctor, n, 2 * limit + 10, seed=8)):
        assert a.shape == (n, ni)
        od, rd, ted, _, info = env.step(a)
        oo, ro, teo, _, fo = o.step(a, want_final=True)
        assert np.array_equal(_np(od).view(np.uint32), oo.view(np.uint32)), t
        assert np.array_equal(_np(rd), ro) and np.array_equal(_np(ted), teo.astype(bool)), t
        done = teo.astype(bool)
        assert np.array_equal(_np(info["final_obs"])[done], fo[done]), t
    a_seed, t0, env0, k = R["rollout"]
    obs, rs, dc = env.rollout(k, action_seed=a_seed, t0=t0)
    oo, ro, do = o.rollout(k, a_seed, t0=t0, env0=env0)
    assert np.array_equal(_np(obs), oo) and np.array_equal(_np(rs), ro) and np.array_equal(_np(dc), do) and do.min() >= 1
    assert np.array_equal(_np(env.total_reward()), o.total_reward())
    for q in range(4 * ni):
        for f in ["queue_len", "queue_dest", "queue_wait"]:
            assert np.array_equal(_np(env.info(f, q)), o.info(f, q)), (f, q)
    assert bool((env.info("num_vehicles") <= max(ctor["max_vehicles"], 0)).all())
    if ctor["spawn_rate"] == 0.0:
        assert int(env.info("num_vehicles").max()) == 0
    o2 = oracle.TrafficOracle(n, oracle.SAME_STEP, max_steps=limit, **ctor)
    o2.set_state(env.get_state())
    twin = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", env_index0=R["env0"], max_steps=limit, **ctor)
    twin.set_state(o2.get_state())
    assert np.array_equal(twin.get_state(), env.get_state())
    acts = torch.randint(0, 3, (40, n, ni), dtype=torch.int32, device="cuda")
    traj, rt, tt, rs, dc = env.rollout(40, actions=acts, trajectory=True, per_step=True)
    for t in range(40):
        ob, r, te, _, _ = twin.step(acts[t])
        assert torch.equal(ob, traj[t]) and torch.equal(r, rt[t]) and torch.equal(te, tt[t]), t
    env.close(); twin.close()


@pytest.mark.parametrize("ctor", [dict(), dict(grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4),
                                  dict(grid_size=(4, 5), num_intersections=13, max_vehicles=60, spawn_rate=0.5)], ids=["default", "3x3_4", "4x5_13"])
def test_same_step_rollout_delivers_terminal_observations(cge, ctor):
    """SAME_STEP rollout(trajectory=True) + the compacted final-obs output == k step() calls' (obs, infos["final_obs"]): the reference
    returns the terminal observation from step() (environment.py:193-203); the trajectory's slot holds the reset observation.
    (All eight env types: tests/test_final_obs_gpu.py; here: the traffic layouts, with desynchronised episodes.)"""
    n, limit, k = 300, 37, 100
    env = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", max_steps=limit, **ctor)
    twin = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", max_steps=limit, **ctor)
    env.reset(seed=3); twin.reset(seed=3)
    warm = torch.randint(0, 3, (11, n, env.num_intersections), dtype=torch.int32, device="cuda")
    mask = (torch.arange(n, device="cuda") % 3 == 0).to(torch.uint8)
    for e in (env, twin):                                  # desynchronise the episodes: a third of the envs restarts 11 steps late
        for t in range(11):
            e.step(warm[t])
        e.reset(options={"reset_mask": mask})
    env.collect_final_obs(rows_per_env=4)                  # every env finishes two or three episodes in the k steps
    assert env.final_obs_segment == 16
    acts = torch.randint(0, 3, (k, n, env.num_intersections), dtype=torch.int32, device="cuda")
    traj, rt, tt, rs, dc = env.rollout(k, actions=acts, trajectory=True, per_step=True)
    rows, step, who = env.final_obs()
    assert env.final_obs_dropped() == 0 and rows.shape[0] == int(tt.sum())
    j = 0
    for t in range(k):
        ob, r, te, _, info = twin.step(acts[t])
        assert torch.equal(ob, traj[t]) and torch.equal(te, tt[t])
        done = torch.nonzero(te).flatten()
        m = done.numel()
        if m:
            assert torch.equal(step[j:j + m], torch.full((m,), t, device="cuda")) and torch.equal(who[j:j + m], done)
            assert torch.equal(rows[j:j + m], info["final_obs"][done]), t
            j += m
    assert j == rows.shape[0] and j >= n * (k // limit)
    env.close(); twin.close()


def test_unsupported_layouts_and_out_of_range_knobs_are_refused(cge):
    with pytest.raises(ValueError, match="not supported"):
        cge.TrafficVectorEnv(4, grid_size=(5, 5), num_intersections=17)
    with pytest.raises(ValueError, match="not supported"):
        cge.TrafficVectorEnv(4, grid_size=(1, 1), num_intersections=9)       # one intersection: the reference raises at the first spawn
    with pytest.raises(ValueError):
        cge.TrafficVectorEnv(4, max_vehicles=128)
    with pytest.raises(ValueError):
        cge.TrafficVectorEnv(4, max_vehicles=100, max_steps=5000)       # a queue's waiting sum would not fit its 18 bits
    with pytest.raises(ValueError):
        cge.TrafficVectorEnv(4, spawn_rate=-0.1)
    env = cge.make_vec("TrafficManagement-v0", 8, grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4)
    assert env.num_intersections == 4 and env.reset(seed=1)[0].shape == (8, 60)
    env.close()


def test_rollout_state_roundtrip_and_trajectory(cge, oracle):
    n = 2048 + 9
    env = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", env_index0=77)
    o = oracle.TrafficOracle(n, oracle.SAME_STEP)
    o.seed(np.arange(n, dtype=np.uint64) + np.uint64(77 + 1))
    env.reset(seed=1); o.reset()
    obs, rs, dc = env.rollout(700, action_seed=9)
    oo, ro, do = o.rollout(700, 9, env0=77)
    assert np.array_equal(_np(obs), oo) and np.array_equal(_np(rs), ro) and np.array_equal(_np(dc), do)
    # device state -> oracle -> continue both
    o2 = oracle.TrafficOracle(n, oracle.SAME_STEP)
    o2.set_state(env.get_state())
    obs, rs, dc = env.rollout(500, action_seed=9, t0=700)
    oo, ro, do = o2.rollout(500, 9, t0=700, env0=77)
    assert np.array_equal(_np(obs), oo) and np.array_equal(_np(rs), ro) and np.array_equal(_np(dc), do) and do.min() == 1
    # oracle state -> device twin; explicit-action trajectory == step-by-step
    twin = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", env_index0=77)
    twin.set_state(o2.get_state())
    assert np.array_equal(twin.get_state(), env.get_state())
    acts = torch.randint(0, 3, (30, n, 9), dtype=torch.int32, device="cuda")
    traj, rt, tt, rs, dc = env.rollout(30, actions=acts, trajectory=True, per_step=True)
    for t in range(30):
        ob, r, te, _, _ = twin.step(acts[t])
        assert torch.equal(ob, traj[t]) and torch.equal(r, rt[t]) and torch.equal(te, tt[t]), t
    env.close(); twin.close()


def test_config4_size_properties_and_sampled_parity(cge, oracle):
    """BASELINE config 4: 262,144 envs.  Whole-batch invariants + bit-exact oracle parity on end slices, and
    sharding invariance (a handle owning only the upper half reproduces the same rows)."""
    n, T = 1 << 18, 250
    env = cge.TrafficVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    obs, _ = env.reset(seed=0)
    assert float(obs.sum()) == 9.0 * n                       # only the NS_GREEN one-hots are set after reset
    obs, rs, dc = env.rollout(T, action_seed=123)
    assert torch.equal(obs[:, :36].reshape(n, 9, 4).sum(-1), torch.ones(n, 9, device="cuda"))     # one phase per light
    nveh = env.info("num_vehicles")
    assert bool((nveh <= 50).all()) and torch.equal(obs[:, 126], nveh.float())
    qsum = sum(env.info("queue_len", q) for q in range(36))
    assert bool((qsum <= nveh).all())                        # queued vehicles are a subset of live vehicles
    for lo in [0, n - 1500]:
        m = 1500
        o = oracle.TrafficOracle(m, oracle.SAME_STEP)
        o.seed(np.arange(lo, lo + m, dtype=np.uint64)); o.reset()
        oo, ro, do = o.rollout(T, 123, env0=lo)
        assert np.array_equal(_np(obs[lo:lo + m]), oo) and np.array_equal(_np(rs[lo:lo + m]), ro)
    half = cge.TrafficVectorEnv(n // 2, autoreset_mode="SameStep", env_index0=n // 2)
    half.reset(seed=0)
    oh, rh, dh = half.rollout(T, action_seed=123)
    assert torch.equal(oh, obs[n // 2:]) and torch.equal(rh, rs[n // 2:])
    env.close(); half.close()


def test_reference_info_keys(cge):
    """`reference_info=True`: the reference's `_get_info()` keys (environment.py:365-384, utils.py:251-267) against the fixture's recorded
    per-intersection state."""
    fx = golden("traffic_3x3.npz")
    A = fx["actions"]
    n, T, ni = A.shape
    ctor = json.loads(str(fx["ctor"]))
    env = cge.TrafficVectorEnv(n, autoreset_mode="Disabled", reference_info=True, **ctor)
    env.reset(seed=int(fx["seed0"]))
    A_dev = torch.from_numpy(A).cuda()
    for t in range(400):
        _, _, te, _, info = env.step(A_dev[:, t])
        if t % 100 != 99:
            continue
        S = fx["internal"][:, t].astype(np.int64)
        per = S[:, :8 * ni].reshape(n, ni, 8)
        st = info["intersection_states"]
        assert np.array_equal(_np(st["light_phase"]), per[:, :, 0]) and np.array_equal(_np(st["vehicles_passed"]), per[:, :, 2])
        assert np.array_equal(_np(st["total_waiting_time"]), per[:, :, 3]) and np.array_equal(_np(st["queue_lengths"]), per[:, :, 4:8])
        tp, tw, tq = per[:, :, 2].sum(1), per[:, :, 3].sum(1), per[:, :, 4:8].sum((1, 2))
        m = info["metrics"]
        assert np.array_equal(_np(m["total_vehicles_passed"]), tp) and np.array_equal(_np(m["total_queue_length"]), tq)
        assert np.array_equal(_np(m["average_waiting_time"]), tw / np.maximum(tp, 1)) and np.array_equal(_np(m["throughput"]), tp / ni)
        assert np.array_equal(_np(m["average_queue_length"]), tq / ni)
        assert np.array_equal(_np(info["num_vehicles"]), S[:, 8 * ni]) and np.array_equal(_np(info["timestep"]), S[:, 8 * ni + 1])
        assert np.array_equal(_np(info["total_reward"]), np.cumsum(fx["reward"][:, :t + 1], axis=1)[:, -1]) or \
            np.allclose(_np(info["total_reward"]), fx["reward"][:, :t + 1].sum(1), rtol=1e-12)
    env.close()
