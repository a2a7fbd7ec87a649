"""AirlineVectorEnv on the device against the unmodified reference (tests/golden/airline_*.npz) and, where the fixtures cannot reach,
against the model that tests/test_airline_cpu.py pins to them (tests/airline_model.py).  Every comparison is array_equal on bit
patterns and skips no rows; rewards are the reference's float64 values rounded to the float32 of the output buffer."""
import types

import numpy as np
import pytest
import torch

import _lane_kit as kit
import airline_model as am
from _lane_kit import cge, dev, f32, same  # noqa: F401
from conftest import golden

pytestmark = pytest.mark.gpu

PER_ENV = 1656 + 2560                                                     # the documented device bytes per env: record + generator
SAME_STEP_FIXTURES = ["airline_hash.npz", "airline_dispatch.npz", "airline_cancel.npz"]
SPEC = types.SimpleNamespace(
    m=am, kind="airline", env="AirlineVectorEnv", model=am.AirlineModel, limit=None, obs=160, actions=45, info=am.INFO, clock="timestep", live=kit.whole,
    ending=SAME_STEP_FIXTURES,
    disabled=("airline_cancel.npz", lambda ends: ends >= 16),
    overrun=("airline_overrun.npz", lambda z: (z["wraps"] >= 4).all()),
    next_step=("airline_hash.npz", lambda n: n),
    kernel=(80, 3, None, 1),                                              # T, seed, limit, ends per env
    bad=(45, 52),
    rollout=(4, (7, 1, 80, 7), None, None, lambda n, given: 0),           # seed, k of every rollout, limit, the idling action, ends
    sampled_steps=20,
    # snapshot: the 40 steps cross the end on the clock of every env still in its first episode (an env that ended early within the
    # 50 steps has no end in these 40)
    snapshot=(None, lambda env: True),
    statistics=(150, None, 2, 71),                                        # T, limit, ends per env, the longest episode
    sharding=(333, 80, None, [(0, 167), (167, 166)]),                     # n, k, limit, the shards
    captured_limit=None)


def info5(env):
    return kit.info_of(SPEC, env)


def test_surface(cge):
    env = cge.AirlineVectorEnv(300, autoreset_mode="SameStep")
    obs, infos = env.reset(seed=1)
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (300, 160) and obs.is_cuda and infos == {}
    assert int(env.single_action_space.n) == 45 and tuple(env.single_observation_space.shape) == (160,)
    assert [int(v) for v in env.action_space.nvec] == [45] * 300 and tuple(env.observation_space.shape) == (300, 160)
    o, r, te, tr, infos = env.step(torch.zeros(300, dtype=torch.int32, device="cuda"))
    assert r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool and not tr.any() and "final_obs" in infos
    assert env.last_kernel() == "cge::airline::step_kernel<1>"            # the instance a profile of this call shows (1 = SameStep)
    traj, rs, dc = env.rollout(3, action_seed=1, trajectory=True)
    assert tuple(traj.shape) == (3, 300, 160) and env.last_kernel() == "cge::airline::rollout_kernel<1, false>"
    assert env.device_bytes() == 300 * PER_ENV + 8
    env.close()
    env = cge.AirlineVectorEnv(5, reference_info=True, info_fields=("timestep", "flights_in_air"))
    _, infos = env.reset(seed=1)
    assert list(infos)[2:] == list(am.INFO) and (infos["current_hour"] == 6.0).all() and (infos["on_time_performance"] == 0.95).all()
    infos = env.step(torch.full((5,), 44, dtype=torch.int32, device="cuda"))[4]
    assert (infos["timestep"] == 1).all() and (infos["current_hour"] == 6.25).all() and infos["daily_costs"].dtype == torch.float64
    assert not infos["daily_revenue"].any() and (infos["daily_costs"] > 0).all()
    env.close()


@pytest.mark.parametrize("name", SAME_STEP_FIXTURES)
def test_fixtures_same_step(cge, name):
    kit.fixtures_same_step(cge, SPEC, name)


def test_cancel_fixture_disabled_with_masked_resets(cge):
    kit.disabled_with_masked_resets(cge, SPEC)


def test_overrun_fixture_steps_on_past_termination(cge):
    """Disabled, never reset: the midnight wrap, maintenance events and the fuel floor run nowhere else."""
    kit.overrun_fixture_steps_on_past_termination(cge, SPEC)


def test_hash_fixture_next_step_against_the_model(cge):
    kit.hash_fixture_next_step_against_the_model(cge, SPEC)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_kernel_equals_the_model(cge, n):
    """a single lane, a partial last wave, whole waves; 80 steps hold one end on the clock"""
    kit.kernel_equals_the_model(cge, SPEC, n)


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
@pytest.mark.parametrize("given", [False, True])
def test_rollout_equals_steps(cge, mode, given):
    kit.rollout_equals_steps(cge, SPEC, mode, given)


def test_rollout_replays_dispatch_in_chunks_with_info_parity(cge):
    z = golden("airline_dispatch.npz")
    n, T = z["reward"].shape
    ref = am.fixture_obs(z)
    env = cge.AirlineVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=int(z["seed0"]))
    acts = dev(z["actions"].T)
    t = 0
    for k in (1, 40, 30, 71, 8):
        traj, rt, tt, _, _ = env.rollout(k, actions=acts[t:t + k], trajectory=True, per_step=True)
        tm = z["terminated"][:, t:t + k].T.astype(bool)
        assert np.array_equal(tt.cpu().numpy(), tm), t
        same(rt, f32(z["reward"][:, t:t + k].T), t)
        same(traj, ref[:, t:t + k].transpose(1, 0, 2), t, ~tm)            # a terminated step holds the reset observation
        t += k
    assert t == T
    env.close()
    env = cge.AirlineVectorEnv(n, autoreset_mode="Disabled", reference_info=True)      # info and reference_info() at every step
    m = am.AirlineModel(int(z["seed0"]) + np.arange(n), am.DISABLED)
    env.reset(seed=int(z["seed0"])); m.reset()
    for t in range(T):
        term, _, infos = env.step(acts[t])[2:]
        m.step(z["actions"][:, t])
        assert list(infos) == list(am.INFO)
        same(np.stack([infos[k].cpu().numpy() for k in am.INFO], 1), z["info"][:, t], t)
        extra = np.stack([env.info(k).cpu().numpy() for k in ("timestep", "needs_reset", "flights_in_air", "delay_compensation", "fuel_costs")], 1)
        same(extra, m.extra(), (t, "extra"))
        tm = term.cpu().numpy()
        if tm.any():
            env.reset(options={"reset_mask": tm.astype(np.uint8)}); m.reset(tm)
    env.close()


def test_out_of_range_and_negative_actions(cge):
    kit.out_of_range_and_negative_actions(cge, SPEC)


def test_action_sampler_matches_host_sampling(cge):
    kit.action_sampler_matches_host_sampling(cge, SPEC)


def test_snapshot_round_trip_into_a_fresh_handle(cge):
    kit.snapshot_round_trip_into_a_fresh_handle(cge, SPEC)


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_episode_statistics(cge, mode):
    kit.episode_statistics(cge, SPEC, mode)


def test_sharding_invariance(cge):
    kit.sharding_invariance(cge, SPEC)


# graph capture: the method of tests/test_graph_capture_gpu.py (tests/_lane_kit.py)
def test_captured_steps_replay_and_match_an_eager_twin(cge):
    kit.captured_steps_replay_and_match_an_eager_twin(cge, SPEC)


def test_captured_rollout_replays_and_matches_an_eager_twin(cge):
    kit.captured_rollout_replays_and_matches_an_eager_twin(cge, SPEC)


def test_refusals(cge):
    with pytest.raises(cge.NativeLibraryError):
        cge.AirlineVectorEnv(8, device="cpu")
    with pytest.raises(ValueError):
        cge.AirlineVectorEnv(0)
    with pytest.raises(ValueError):
        cge.AirlineVectorEnv(8, autoreset_mode="Sometimes")
    with pytest.raises(ValueError):
        cge.AirlineVectorEnv(8, info_fields=("no_such_field",))
    env = cge.AirlineVectorEnv(8, info_fields=("timestep",))
    env.reset(seed=0)
    for shape in ((7,), (8, 1), (2, 8)):
        with pytest.raises(ValueError):
            env.step(torch.zeros(shape, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.rollout(3, actions=torch.zeros((2, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.reset(seed=-1)
    with pytest.raises(TypeError):
        env.info("timestep", 1)                                           # the fields are not indexed
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    odd = torch.zeros(8 * 160 + 1, device="cuda")[1:]                     # 4 bytes off a 16-byte boundary
    buf = torch.zeros(8 * 160, device="cuda")
    assert env._lib.cge_airline_step(env._h, a.data_ptr(), odd.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert b"16-byte aligned" in env._lib.cge_airline_last_error(env._h)
    assert env._lib.cge_airline_step(env._h, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert env._lib.cge_airline_rollout(env._h, 2, None, 0, 0, buf.data_ptr(), 8 * 160 - 4, None, None, None, None, None) == -1
    assert env._lib.cge_airline_info(env._h, 10, buf.data_ptr(), None) == -1
    _, _, _, _, infos = env.step(a)
    assert (infos["timestep"] == 1).all()
    env.close()


def test_one_million_envs(cge):
    n, T, a_seed, seed = 1 << 20, 3, 31, 6
    sample = np.concatenate([np.arange(1365), n // 2 + np.arange(1366), n - 1365 + np.arange(1365)])   # first, middle, last: 4,096 envs
    sidx = torch.from_numpy(sample).cuda()
    env = cge.AirlineVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    assert env.device_bytes() == n * PER_ENV + 8
    m = am.AirlineModel(seed + sample, am.SAME_STEP)
    obs, _ = env.reset(seed=seed)
    same(obs[sidx], m.reset(), "reset")
    acts = am.hash_actions(a_seed, T, len(sample), envs=sample)
    traj, rt, tt, rs, dc = env.rollout(T, action_seed=a_seed, trajectory=True, per_step=True)
    hours = torch.from_numpy(((6.0 + 0.25 * np.arange(1, T + 1)) / 24.0).astype(np.float32)).cuda()
    assert not tt.any() and bool((traj[:, :, 152] == hours[:, None]).all())
    sub, rsub = traj[:, sidx].cpu().numpy(), rt[:, sidx].cpu().numpy()
    for j in range(T):
        mo, mr, mt = m.step(acts[j])[:3]
        same(sub[j], mo, j); same(rsub[j], f32(mr), j)
        assert not mt.any()
    env.close()
