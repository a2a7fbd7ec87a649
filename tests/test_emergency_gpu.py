"""EmergencyVectorEnv on the device against the unmodified reference (tests/golden/emergency_*.npz) and, where the fixtures cannot
reach, against the model that tests/test_emergency_cpu.py pins to them (tests/emergency_model.py).  Every comparison is array_equal on
bit patterns and skips no rows; rewards are the reference's float64 values rounded to the float32 of the output buffer."""
import types

import numpy as np
import pytest
import torch

import _lane_kit as kit
import emergency_model as em
from _lane_kit import cge, dev, f32, same  # noqa: F401
from conftest import golden

pytestmark = pytest.mark.gpu

PER_ENV = 808 + 2560                                                      # the documented device bytes per env: record + generator
EXTRA = ("timestep", "needs_reset", "busy_units", "mutual_aid_requested", "national_guard_active", "state_of_emergency")
SAME_STEP_FIXTURES = ["emergency_hash.npz", "emergency_dispatch.npz", "emergency_idle.npz", "emergency_timeout.npz"]
SPEC = types.SimpleNamespace(
    m=em, kind="emergency", env="EmergencyVectorEnv", model=em.EmergencyModel, limit="max_timesteps", short=("emergency_timeout.npz", 90),
    obs=276, actions=50, info=em.INFO, clock="timestep", live=kit.whole,
    ending=SAME_STEP_FIXTURES,
    disabled=("emergency_idle.npz", lambda ends: ends >= 8),
    overrun=("emergency_overrun.npz", lambda z: z["terminated"][:, -1].all()),
    next_step=("emergency_hash.npz", lambda n: 8),
    # kernel: T, seed, limit, ends per env
    kernel=(120, 3, 50, 2),
    bad=(50, 57),
    # rollout: seed, k of every rollout (a twist every ten steps or so: every rollout but the second straddles one), limit, the idling
    # action, ends: the step limit of 60 ends every env's first episode in these 95 steps
    rollout=(4, (7, 1, 80, 7), 60, None, lambda n, given: n),
    sampled_steps=20,
    snapshot=(70, lambda env: env.info("mutual_aid_requested").any() and env.info("busy_units").any()),   # mid-episode, mutual-aid units present
    statistics=(150, 40, 3, 41),        # T, limit, ends per env, the longest episode: one ends at the latest in the step that starts at minute 40
    sharding=(200, 80, 60, [(0, 67), (67, 67), (134, 66)]),               # n, k, limit, the shards
    captured_limit=60)


def info6(env):
    return kit.info_of(SPEC, env)


def test_surface(cge):
    env = cge.EmergencyVectorEnv(300, autoreset_mode="SameStep")
    obs, infos = env.reset(seed=1)
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (300, 276) and obs.is_cuda and infos == {}
    assert int(env.single_action_space.n) == 50 and tuple(env.single_observation_space.shape) == (276,)
    assert float(env.single_observation_space.low.min()) == 0.0 and float(env.single_observation_space.high.max()) == 10.0
    assert [int(v) for v in env.action_space.nvec] == [50] * 300 and tuple(env.observation_space.shape) == (300, 276)
    o, r, te, tr, infos = env.step(torch.full((300,), 49, dtype=torch.int32, device="cuda"))
    assert r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool and not tr.any() and "final_obs" in infos
    assert env.last_kernel() == "cge::emergency::step_kernel<1>"          # the instance a profile of this call shows (1 = SameStep)
    traj, rs, dc = env.rollout(3, action_seed=1, trajectory=True)
    assert tuple(traj.shape) == (3, 300, 276) and env.last_kernel() == "cge::emergency::rollout_kernel<1, false>"
    assert env.device_bytes() == 300 * PER_ENV + 8
    env.close()
    env = cge.EmergencyVectorEnv(5, reference_info=True, info_fields=("timestep", "busy_units"))
    _, infos = env.reset(seed=1)
    assert list(infos)[2:] == list(em.INFO) and (infos["active_emergencies"] >= 1).all() and (infos["active_emergencies"] <= 3).all()
    infos = env.step(torch.full((5,), 49, dtype=torch.int32, device="cuda"))[4]
    assert (infos["timestep"] == 1).all() and not infos["busy_units"].any() and infos["avg_response_time"].dtype == torch.float64
    assert not infos["termination_reason"].any()
    env.close()


@pytest.mark.parametrize("name", SAME_STEP_FIXTURES)
def test_fixtures_same_step(cge, name):
    kit.fixtures_same_step(cge, SPEC, name)


def test_idle_fixture_disabled_with_masked_resets(cge):
    kit.disabled_with_masked_resets(cge, SPEC)


def test_overrun_fixture_steps_on_past_termination(cge):
    """Disabled, never reset: twenty incidents for hundreds of steps, escalations of worked incidents, the casualty counter far past 50."""
    kit.overrun_fixture_steps_on_past_termination(cge, SPEC)


def test_day_fixture_runs_through_every_hour(cge):
    """emergency_day.npz: Disabled, never reset, on to 22:10 on the env's clock, so that the traffic's hour-of-day chain (:787-792) takes
    every arm: the morning and the evening rush, the hours between and after them, the night on both sides of midnight.  Chunks of
    fused steps, every step's row, reward and flag compared with the recorded reference."""
    z = golden("emergency_day.npz")
    n, T = z["reward"].shape
    assert (n, T) == (4, 1330) and not int(z["autoreset"])
    ref = em.fixture_obs(z)
    env = cge.EmergencyVectorEnv(n, autoreset_mode="Disabled")
    same(env.reset(seed=int(z["seed0"]))[0], z["obs0"], "reset")
    acts = dev(z["actions"].T)
    for t in range(0, T, 70):
        k = min(70, T - t)
        traj, rt, tt, rs, dc = env.rollout(k, actions=acts[t:t + k], trajectory=True, per_step=True)
        same(traj, ref[:, t:t + k].transpose(1, 0, 2), t); same(rt, f32(z["reward"][:, t:t + k].T), t)
        assert np.array_equal(tt.cpu().numpy(), z["terminated"][:, t:t + k].T.astype(bool)), t
        same(info6(env), z["info"][:, t + k - 1], (t, "info"))
    assert (env.info("timestep") == T).all()
    env.close()


def test_hash_fixture_next_step_against_the_model(cge):
    kit.hash_fixture_next_step_against_the_model(cge, SPEC)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_kernel_equals_the_model(cge, n):
    """a single lane, a partial wave, exactly one wave, one lane into the next, several waves; 120 steps pass a generator twist (624
    words at 58 or more a step) and, with the step limit at 50, at least two episode ends in every env"""
    kit.kernel_equals_the_model(cge, SPEC, n)


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
@pytest.mark.parametrize("given", [False, True])
def test_rollout_equals_steps(cge, mode, given):
    kit.rollout_equals_steps(cge, SPEC, mode, given)


def test_rollout_replays_dispatch_in_chunks_with_info_parity(cge):
    z = golden("emergency_dispatch.npz")
    n, T = z["reward"].shape
    ref = em.fixture_obs(z)
    env = cge.EmergencyVectorEnv(n, autoreset_mode="SameStep")
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
    env = cge.EmergencyVectorEnv(n, autoreset_mode="Disabled", reference_info=True)    # info and reference_info() at every step
    m = em.EmergencyModel(int(z["seed0"]) + np.arange(n), em.DISABLED)
    env.reset(seed=int(z["seed0"])); m.reset()
    for t in range(T):
        term, _, infos = env.step(acts[t])[2:]
        m.step(z["actions"][:, t])
        assert list(infos) == list(em.INFO)
        same(np.stack([infos[k].cpu().numpy() for k in em.INFO], 1), z["info"][:, t], t)
        same(np.stack([env.info(k).cpu().numpy() for k in EXTRA], 1), m.extra(), (t, "extra"))
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
        cge.EmergencyVectorEnv(8, device="cpu")
    with pytest.raises(ValueError):
        cge.EmergencyVectorEnv(0)
    with pytest.raises(ValueError):
        cge.EmergencyVectorEnv(8, autoreset_mode="Sometimes")
    with pytest.raises(ValueError):
        cge.EmergencyVectorEnv(8, info_fields=("no_such_field",))
    for bad in (0, -5, 65536):
        with pytest.raises(ValueError, match="max_timesteps"):
            cge.EmergencyVectorEnv(8, max_timesteps=bad)
    env = cge.EmergencyVectorEnv(8, info_fields=("timestep",), max_timesteps=65535)
    env.reset(seed=0)
    for shape in ((7,), (8, 1), (2, 8)):
        with pytest.raises(ValueError):
            env.step(torch.zeros(shape, dtype=torch.int32, device="cuda"))
    o1 = env.step(torch.full((8,), 49, dtype=torch.int64))[0]             # host / int64 actions are converted, as for every type
    assert o1.is_cuda and (env.info("timestep") == 1).all()
    env.reset(seed=0)
    with pytest.raises(ValueError):
        env.rollout(3, actions=torch.zeros((2, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.reset(seed=-1)
    with pytest.raises(TypeError):
        env.info("timestep", 1)                                           # the fields are not indexed
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    odd = torch.zeros(8 * 276 + 1, device="cuda")[1:]                     # 4 bytes off a 16-byte boundary
    buf = torch.zeros(8 * 276, device="cuda")
    assert env._lib.cge_emergency_step(env._h, a.data_ptr(), odd.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert b"16-byte aligned" in env._lib.cge_emergency_last_error(env._h)
    assert env._lib.cge_emergency_step(env._h, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert env._lib.cge_emergency_rollout(env._h, 2, None, 0, 0, buf.data_ptr(), 8 * 276 - 4, None, None, None, None, None) == -1
    assert env._lib.cge_emergency_info(env._h, 12, buf.data_ptr(), None) == -1
    _, _, _, _, infos = env.step(a)
    assert (infos["timestep"] == 1).all()
    env.close()
