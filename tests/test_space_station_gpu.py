"""SpaceStationVectorEnv on the device against the unmodified reference (tests/golden/station_*.npz) and, where the fixtures cannot
reach, against the model that tests/test_space_station_cpu.py pins to them (tests/space_station_model.py).  Every comparison is
array_equal on bit patterns and skips no rows; rewards are the reference's float64 values rounded to the float32 of the output buffer."""
import types

import numpy as np
import pytest
import torch

import _lane_kit as kit
import space_station_model as sm
from _lane_kit import cge, dev, f32, same  # noqa: F401
from conftest import golden

pytestmark = pytest.mark.gpu

PER_ENV = 752 + 2560                                                      # the documented device bytes per env: record + generator
INFO10 = sm.INFO + ("system_failure_mask",)
IDLE_SEED = 300                                                           # station_idle's: action 39 ends most first episodes in step 33 by the cascade
SAME_STEP_FIXTURES = ["station_hash.npz", "station_keep.npz", "station_idle.npz", "station_evacuate.npz", "station_timeout.npz"]
SPEC = types.SimpleNamespace(
    m=sm, kind="space_station", env="SpaceStationVectorEnv", model=sm.SpaceStationModel, limit="max_steps", short=("station_timeout.npz", 20),
    obs=120, actions=40, info=INFO10, clock="time_step", live=kit.whole,
    ending=SAME_STEP_FIXTURES,
    disabled=("station_idle.npz", lambda ends: ends >= 32),
    overrun=("station_overrun.npz", lambda z: (z["terminated"].sum(1) >= 50).sum() >= 2),
    next_step=("station_hash.npz", lambda n: 8),
    # kernel: T, seed, limit, ends per env
    kernel=(60, IDLE_SEED, 25, 2),
    bad=(40, 57),
    # rollout: seed, k of every rollout (the third straddles step 33, where the idling envs' episodes end), limit, the idling action, ends
    rollout=(IDLE_SEED, (7, 1, 30, 7), None, 39, lambda n, given: n // 2 if given else 1),
    sampled_steps=20,
    snapshot=(70, lambda env: env.info("evacuated").any() and not env.info("evacuated").all() and (env.info("time_step") > 0).any()),    # mid-episode
    statistics=(100, 30, 3, 30),                                          # T, limit, ends per env, the longest episode
    sharding=(200, 60, 40, [(0, 67), (67, 67), (134, 66)]),               # n, k, limit, the shards
    captured_limit=60)


def info10(env):
    return kit.info_of(SPEC, env)


def test_surface(cge):
    env = cge.SpaceStationVectorEnv(300, autoreset_mode="SameStep")
    obs, infos = env.reset(seed=1)
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (300, 120) and obs.is_cuda and infos == {}
    assert int(env.single_action_space.n) == 40 and tuple(env.single_observation_space.shape) == (120,)
    assert float(env.single_observation_space.low.max()) == -np.inf and float(env.single_observation_space.high.min()) == np.inf
    assert [int(v) for v in env.action_space.nvec] == [40] * 300 and tuple(env.observation_space.shape) == (300, 120)
    o, r, te, tr, infos = env.step(torch.full((300,), 39, dtype=torch.int32, device="cuda"))
    assert r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool and not tr.any() and "final_obs" in infos
    assert env.last_kernel() == "cge::station::step_kernel<1>"            # the instance a profile of this call shows (1 = SameStep)
    traj, rs, dc = env.rollout(3, action_seed=1, trajectory=True)
    assert tuple(traj.shape) == (3, 300, 120) and env.last_kernel() == "cge::station::rollout_kernel<1, false>"
    assert env.device_bytes() == 300 * PER_ENV + 8
    env.close()
    env = cge.SpaceStationVectorEnv(5, reference_info=True, info_fields=("crew_casualties", "evacuated"))
    _, infos = env.reset(seed=1)
    assert list(infos)[2:] == list(sm.INFO) and (infos["crew_alive"] == 6).all() and (infos["battery_level"] == 100.0).all()
    infos = env.step(torch.full((5,), 38, dtype=torch.int32, device="cuda"))[4]
    assert (infos["time_step"] == 1).all() and infos["evacuated"].all() and infos["avg_crew_health"].dtype == torch.float64
    assert not infos["crew_casualties"].any() and not infos["mission_success"].any()
    env.close()


@pytest.mark.parametrize("name", SAME_STEP_FIXTURES)
def test_fixtures_same_step(cge, name):
    kit.fixtures_same_step(cge, SPEC, name)


def test_poked_fixture_same_step(cge):
    """station_poked.npz: the reference with resources, module air and temperature, crew values and a system's efficiency set from outside
    between steps (states no run a fixture can hold reaches, the three ends behind the cascade of failed systems among them).  The
    device gets the same pokes through snapshot() and restore(), at the word offsets the host build of csrc/space_station_env.hpp
    reports, and is then compared like any other fixture, the three ends and their resets included."""
    pokes = sm.fixture_pokes(golden("station_poked.npz"))
    assert sorted(pokes) == list(range(1, 16))
    assert kit.replay_same_step(cge, SPEC, "station_poked.npz", pokes) == (3, 3)


def test_idle_fixture_disabled_with_masked_resets(cge):
    kit.disabled_with_masked_resets(cge, SPEC)


def test_overrun_fixture_steps_on_past_termination(cge):
    """Disabled, never reset: some envs run fifty steps and more past their first `terminated`, the casualty counter still growing"""
    kit.overrun_fixture_steps_on_past_termination(cge, SPEC)


def test_hash_fixture_next_step_against_the_model(cge):
    kit.hash_fixture_next_step_against_the_model(cge, SPEC)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_kernel_equals_the_model(cge, n):
    """a single lane, a partial wave, exactly one wave, one lane into the next, several waves; 60 hashed steps from the idle fixture's
    seeds pass two generator twists and the power cascade (battery below 10 from step ~25 on, thermal drift draws after it); with the
    step limit at 25 every env also ends two episodes by the limit, both flags raised"""
    kit.kernel_equals_the_model(cge, SPEC, n)


@pytest.mark.parametrize("n", [65])
def test_kernel_equals_the_model_through_a_cascade(cge, n):
    """the same without a step limit: the idle fixture's seeds under hashed actions run into the cascade (three critical systems below
    10 %) or lose the crew within 60 steps in some envs; step() this time, with both flags and the info values at every step"""
    T = 60
    env = cge.SpaceStationVectorEnv(n, autoreset_mode="SameStep")
    m = sm.SpaceStationModel(IDLE_SEED + np.arange(n), sm.SAME_STEP)
    same(env.reset(seed=IDLE_SEED)[0], m.reset(), "reset")
    acts = sm.hash_actions(9, T, n)
    acts[:, ::2] = 39                                                     # every other env idles: most of their first episodes end in step 33
    ends = 0
    for t in range(T):
        obs, rew, term, trunc, infos = env.step(dev(acts[t]))
        mo, mr, mt, mtr, mf, mi = m.step(acts[t])
        same(obs, mo, t); same(rew, f32(mr), t)
        assert np.array_equal(term.cpu().numpy(), mt) and not trunc.any(), t
        same(info10(env), mi, (t, "info"), ~mt)
        if mt.any():
            same(infos["final_obs"], mf, (t, "final_obs"), mt)
        ends += int(mt.sum())
    assert ends >= n // 2
    env.close()


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
@pytest.mark.parametrize("given", [False, True])
def test_rollout_equals_steps(cge, mode, given):
    kit.rollout_equals_steps(cge, SPEC, mode, given)


def test_rollout_replays_keep_in_chunks_with_info_parity(cge):
    z = golden("station_keep.npz")
    n, T = z["reward"].shape
    ref = sm.fixture_obs(z)
    env = cge.SpaceStationVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=int(z["seed0"]))
    acts = dev(z["actions"].T)
    t = 0
    for k in (1, 40, 130, 271, 150, 8):
        traj, rt, tt, _, _ = env.rollout(k, actions=acts[t:t + k], trajectory=True, per_step=True)
        tm = z["terminated"][:, t:t + k].T.astype(bool)
        assert np.array_equal(tt.cpu().numpy(), tm), t
        same(rt, f32(z["reward"][:, t:t + k].T), t)
        same(traj, ref[:, t:t + k].transpose(1, 0, 2), t, ~tm)            # a terminated step holds the reset observation
        t += k
        if not tm[-1].any():
            same(info10(env), z["info"][:, t - 1], (t, "info"))
    assert t == T
    env.close()
    env = cge.SpaceStationVectorEnv(n, autoreset_mode="Disabled", reference_info=True)    # reference_info() at every step
    env.reset(seed=int(z["seed0"]))
    for t in range(T):
        term, _, infos = env.step(acts[t])[2:]
        assert list(infos) == list(sm.INFO)
        same(np.stack([infos[k].cpu().numpy() for k in sm.INFO], 1), z["info"][:, t, :9], t)
        tm = term.cpu().numpy()
        if tm.any():
            env.reset(options={"reset_mask": tm.astype(np.uint8)})
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
        cge.SpaceStationVectorEnv(8, device="cpu")
    with pytest.raises(ValueError):
        cge.SpaceStationVectorEnv(0)
    with pytest.raises(ValueError):
        cge.SpaceStationVectorEnv(8, autoreset_mode="Sometimes")
    with pytest.raises(ValueError):
        cge.SpaceStationVectorEnv(8, info_fields=("no_such_field",))
    for bad in (0, -5, 65536):
        with pytest.raises(ValueError, match="max_steps"):
            cge.SpaceStationVectorEnv(8, max_steps=bad)
    env = cge.SpaceStationVectorEnv(8, info_fields=("time_step",), max_steps=65535)
    env.reset(seed=0)
    for shape in ((7,), (8, 1), (2, 8)):
        with pytest.raises(ValueError):
            env.step(torch.zeros(shape, dtype=torch.int32, device="cuda"))
    o1 = env.step(torch.full((8,), 39, dtype=torch.int64))[0]             # host / int64 actions are converted, as for every type
    assert o1.is_cuda and (env.info("time_step") == 1).all()
    env.reset(seed=0)
    with pytest.raises(ValueError):
        env.rollout(3, actions=torch.zeros((2, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.reset(seed=-1)
    with pytest.raises(TypeError):
        env.info("time_step", 1)                                          # the fields are not indexed
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    odd = torch.zeros(8 * 120 + 1, device="cuda")[1:]                     # 4 bytes off a 16-byte boundary
    buf = torch.zeros(8 * 120, device="cuda")
    assert env._lib.cge_space_station_step(env._h, a.data_ptr(), odd.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert b"16-byte aligned" in env._lib.cge_space_station_last_error(env._h)
    assert env._lib.cge_space_station_step(env._h, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert env._lib.cge_space_station_rollout(env._h, 2, None, 0, 0, buf.data_ptr(), 8 * 120 - 4, None, None, None, None, None) == -1
    assert env._lib.cge_space_station_info(env._h, 13, buf.data_ptr(), None) == -1
    _, _, _, _, infos = env.step(a)
    assert (infos["time_step"] == 1).all()
    env.close()
