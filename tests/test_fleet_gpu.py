"""GPU parity tests for the fleet hot path (through the C ABI via FleetVectorEnv): bit-exact obs, rewards,
terminated/truncated flags and float64 fuel against the reference's golden vectors and the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import golden
from _action_streams import RUNS, HASH_ROLLOUTS, fleet_uniform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", ["fleet_hash.npz", "fleet_courier.npz"])
def test_same_step_matches_reference_fixture(cge, name):
    fx = golden(name)
    A = fx["actions"]
    n, T = A.shape[0], A.shape[1]
    env = cge.FleetVectorEnv(n, autoreset_mode="SameStep")
    obs, _ = env.reset(seed=int(fx["seed0"]))
    assert np.array_equal(_np(obs), fx["obs0"])
    reset_at = {(int(i), int(t)): k for k, (i, t) in enumerate(fx["reset_index"])}
    A_dev = torch.from_numpy(A).cuda()
    for t in range(T):
        obs, rew, te, tr, info = env.step(A_dev[:, t])
        obs, rew, te, tr, fin = _np(obs), _np(rew), _np(te), _np(tr), _np(info["final_obs"])
        assert np.array_equal(te, fx["terminated"][:, t].astype(bool)) and np.array_equal(tr, fx["truncated"][:, t].astype(bool)), t
        assert np.array_equal(rew, fx["reward"][:, t].astype(np.float32)), (t, rew, fx["reward"][:, t])
        done = te | tr
        step_obs = np.where(done[:, None], fin, obs)
        assert np.array_equal(step_obs.view(np.uint32), fx["obs"][:, t].view(np.uint32)), (t, np.argwhere(step_obs != fx["obs"][:, t])[:5])
        for i in np.nonzero(done)[0]:
            assert np.array_equal(obs[i], fx["reset_obs"][reset_at[(int(i), t)]]), (i, t)
        if t % 53 == 3:
            live = ~done
            for k in range(3):
                assert np.array_equal(_np(env.info(f"fuel{k}"))[live], fx["fuel"][live, t, k])
            assert np.array_equal(_np(env.info("missed_deadlines"))[live], fx["internal"][live, t, 13])
    env.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_step_matches_oracle_all_modes(cge, oracle, mode):
    code = {"NextStep": oracle.NEXT_STEP, "SameStep": oracle.SAME_STEP, "Disabled": oracle.DISABLED}[mode]
    R = RUNS["fleet_all_modes"]
    n, T = R["n"], R["T"]
    env = cge.FleetVectorEnv(n, autoreset_mode=mode, env_index0=R["env0"])
    o = oracle.FleetOracle(n, code)
    o.seed(np.arange(n, dtype=np.uint64) + np.uint64(R["env0"] + R["seed"]))
    od, _ = env.reset(seed=R["seed"])
    assert np.array_equal(_np(od), o.reset())
    for t, a in enumerate(fleet_uniform("fleet", {}, n, T)):         # uniform, with a few invalid actions (-10) every 11th step
        od, rd, ted, trd, _ = env.step(a)
        oo, ro, teo, tro = o.step(a)
        assert np.array_equal(_np(od).view(np.uint32), oo.view(np.uint32)), t
        assert np.array_equal(_np(rd), ro) and np.array_equal(_np(ted), teo.astype(bool)) and np.array_equal(_np(trd), tro.astype(bool)), t
    for f in ["timestep", "missed_deadlines", "completed_deliveries", "num_requests", "weather_effect", "total_reward", "episodes",
              "needs_reset", "fuel0", "fuel1", "fuel2"]:
        assert np.array_equal(_np(env.info(f)), o.info(f)), f
    env.close()


def test_rollout_config5_size_and_sharding(cge, oracle):
    n, T = 1 << 17, HASH_ROLLOUTS["config5"]["k"]["fleet"]
    env = cge.FleetVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    env.reset(seed=0)
    obs, rs, dc = env.rollout(T, action_seed=123)
    for lo in [0, n - 2500]:
        m = 2500
        o = oracle.FleetOracle(m, oracle.SAME_STEP)
        o.seed(np.arange(lo, lo + m, dtype=np.uint64)); o.reset()
        oo, ro, do = o.rollout(T, 123, env0=lo)
        assert np.array_equal(_np(obs[lo:lo + m]), oo) and np.array_equal(_np(rs[lo:lo + m]), ro) and np.array_equal(_np(dc[lo:lo + m]), do)
    half = cge.FleetVectorEnv(n // 2, autoreset_mode="SameStep", env_index0=n // 2)
    half.reset(seed=0)
    oh, rh, dh = half.rollout(T, action_seed=123)
    assert torch.equal(oh, obs[n // 2:]) and torch.equal(rh, rs[n // 2:]) and torch.equal(dh, dc[n // 2:])
    env.close(); half.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_pipelined_rollout_equals_step_by_step(cge, mode):
    """cge_fleet_rollout runs step t + 1's step launch beside the dense launch that finishes step t (two streams, fleet.hip
    launch_rollout); the per-step trajectory it returns must be the one K single step() calls give, in every autoreset mode,
    across the every-50-steps traffic redraw (all envs on the work list at once) and across a second call."""
    n, K = 700, 130
    g = torch.Generator().manual_seed(5)
    acts = torch.randint(0, 8, (2 * K, n, 3), generator=g, dtype=torch.int32).cuda()
    a, b = cge.FleetVectorEnv(n, autoreset_mode=mode, env_index0=3), cge.FleetVectorEnv(n, autoreset_mode=mode, env_index0=3)
    a.reset(seed=11); b.reset(seed=11)
    for call in range(2):
        A = acts[call * K:(call + 1) * K].contiguous()
        obs, rew, term, rs, dc = a.rollout(K, actions=A, trajectory=True, per_step=True)
        obs, rew, term = obs.clone(), rew.clone(), term.clone()
        tot = torch.zeros(n, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        for t in range(K):
            o, r, te, tr, _ = b.step(A[t])
            assert torch.equal(obs[t], o), (call, t, (obs[t] != o).nonzero()[:4])
            assert torch.equal(rew[t], r) and torch.equal(term[t].to(torch.uint8) & 1, te.to(torch.uint8)), (call, t)
            cnt += (te | tr).to(torch.int32)
        assert torch.equal(dc, cnt)
        for f in ["timestep", "episodes", "total_reward", "needs_reset", "fuel0"]:
            assert torch.equal(a.info(f), b.info(f)), f
    # rows in place (obs_step_stride 0: the dense launch skips the row its own step rewrites), hash actions replaced by explicit ones
    A = acts[:57].contiguous()
    obs, rs, dc = a.rollout(57, actions=A)
    tot = torch.zeros(n, dtype=torch.float64, device="cuda")
    for t in range(57):
        o, r, te, tr, _ = b.step(A[t])
        tot += r.to(torch.float64)
    assert torch.equal(obs, o) and torch.equal(rs, tot)
    a.close(); b.close()


def test_pipelined_rollout_with_full_sublists_and_snapshots(cge):
    """(a) NEXT_STEP with max_timesteps = 50 and n a multiple of 4,096 — every env is truncated at step 50 (the traffic
    redraw lists it), takes its reset-only step at 51 (listed again), so a pipelined dense launch re-lists the whole population while
    step blocks append to the same three rotating lists: the sub-lists have zero slack there (sub_cap = ceil(blocks / 64) * 64), and
    an env filed under the LAUNCHING block instead of its own overflowed one.  One rollout across steps 50 / 51 / 100 / 101 must
    equal step-by-step.  (b) snapshot -> rollout -> restore -> rollout gives the same trajectory: the per-env `seq` / `pending` bits
    and the handle's list parity survive the snapshot."""
    n, K = 4096, 110
    acts = torch.randint(0, 8, (K, n, 3), dtype=torch.int32, device="cuda")
    a = cge.FleetVectorEnv(n, autoreset_mode="NextStep", max_timesteps=50)
    b = cge.FleetVectorEnv(n, autoreset_mode="NextStep", max_timesteps=50)
    a.reset(seed=2); b.reset(seed=2)
    a.rollout(7, actions=acts[:7].contiguous())                # an odd number of pipelined launches before the snapshot
    for t in range(7):
        b.step(acts[t])
    snap = a.snapshot()
    obs, rew, fl, rs, dc = a.rollout(K, actions=acts, trajectory=True, per_step=True)
    obs, rew, fl = obs.clone(), rew.clone(), fl.clone()
    for t in range(K):
        o, r, te, tr, _ = b.step(acts[t])
        assert torch.equal(obs[t], o), (t, (obs[t] != o).nonzero()[:4])
        assert torch.equal(rew[t], r) and torch.equal(fl[t], te.to(torch.uint8) | (tr.to(torch.uint8) << 1)), t
    assert int((fl != 0).sum()) >= 2 * n                       # everybody ran into the time limit twice
    a.restore(snap)
    obs2, rew2, fl2, rs2, dc2 = a.rollout(K, actions=acts, trajectory=True, per_step=True)
    assert torch.equal(obs2, obs) and torch.equal(rew2, rew) and torch.equal(fl2, fl)
    a.close(); b.close()
