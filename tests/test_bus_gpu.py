"""BusVectorEnv on the device against the unmodified reference (tests/golden/bus_*.npz) and, where the fixtures cannot reach, against
the counts model that tests/test_bus_cpu.py pins to them (tests/bus_model.py).  The helpers and the bodies shared with world builder
and restaurant are in tests/_slab_kit.py.  Every comparison is bit-exact and skips no rows."""
import types

import numpy as np
import pytest
import torch

import _slab_kit as kit
import bus_model as bm
from _slab_kit import MODES, cge, dev, host, same, take, warm_up  # noqa: F401

pytestmark = pytest.mark.gpu

SPEC = types.SimpleNamespace(
    m=bm, env="BusVectorEnv", model=bm.BusModel, limit="max_timesteps", from_fixture={"max_timesteps": "max_timesteps"}, flag="truncated",
    keys=bm.KEYS, shapes=bm.KEY_SHAPES, dtypes=dict.fromkeys(bm.KEYS, np.int32), column=(), exact_reward=True,
    rollout=types.SimpleNamespace(
        n=300, limit=150, longest=600, ends=3, info=(),
        given=lambda *a, **kw: (dev(bm.hash_actions(*a, **kw)) * 7 + 3) % 11,
        pre=lambda n, env0: bm.hash_actions(1, 40, n, env0=env0)),                        # host arrays
    sharding=types.SimpleNamespace(n=1000, k=520, kw={}, shards=[(0, 500), (500, 500)], ends=lambda dw: int(dw.min()) == 1))


def test_observation_is_a_dict_of_views_of_one_slab(cge):
    env = cge.BusVectorEnv(300, autoreset_mode="SameStep")
    obs, _ = env.reset(seed=1)
    assert list(obs) == list(bm.KEYS)
    base = obs["bus_stops"].data_ptr()
    start = 0                                                          # plane starts inside the slab, in ints
    for k in bm.KEYS:
        t = obs[k]
        assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (300,) + bm.KEY_SHAPES[k] and t.is_contiguous(), k
        assert t.data_ptr() == base + 4 * start, k
        start += 300 * int(np.prod(bm.KEY_SHAPES[k]))
    assert tuple(env.obs_slab(obs).shape) == (300 * 56,)
    a = env.action_sampler(0).sample()
    assert a.dtype == torch.int32 and tuple(a.shape) == (300, 4) and int(a.min()) >= 0 and int(a.max()) <= 10
    o, r, te, tr, _ = env.step(env.action_sampler(0).sample())
    assert r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool and not te.any()
    assert env.last_kernel() == "cge::bus::step_kernel<1>"             # the instance a profile of this call shows (1 = SameStep)
    env.rollout(3, action_seed=1)
    assert env.last_kernel() == "cge::bus::rollout_kernel<1, false>"
    env.close()


@pytest.mark.parametrize("name", ["bus_hash.npz", "bus_dwell.npz", "bus_short.npz"])
def test_fixtures_same_step(cge, name):
    kit.fixtures_same_step(cge, SPEC, name)


@pytest.mark.parametrize("shape", [(4096, 1100, 500), (333, 260, 13)], ids=["4096x1100", "limit13"])
@pytest.mark.parametrize("mode", list(MODES))
def test_model_parity(cge, mode, shape):
    n, T, limit = shape
    seeds = (np.arange(n, dtype=np.int64) * 7919 + 12345) % 1000003    # a per-env seed array
    kit.model_parity(cge, SPEC, mode, limit, seeds, bm.hash_actions(5, T, n, env0=70001), (limit + 3, 2 * limit + 7), env0=70001)


@pytest.mark.parametrize("k", [1, 20, 600])
@pytest.mark.parametrize("given", [False, True], ids=["hash", "given"])
@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_rollout_equals_k_steps(cge, mode, given, k):
    kit.rollout_equals_k_steps(cge, SPEC, mode, given, k)


def test_sharding_invariance(cge):
    kit.sharding_invariance(cge, SPEC)


def test_episode_statistics(cge):
    n, limit = 300, 60
    env = cge.BusVectorEnv(n, autoreset_mode="SameStep", max_timesteps=limit, record_episode_statistics=True)
    env.reset(seed=5)
    acts = torch.from_numpy(bm.hash_actions(2, 2 * limit, n)).cuda()
    total = np.zeros(n, np.float64)
    for t in range(2 * limit):
        _, rew, _, trunc, infos = env.step(acts[t])
        total += rew.cpu().numpy().astype(np.float64)                 # the float64 sum of the rewards in step order
        assert torch.equal(infos["_episode"], trunc)
        if (t + 1) % limit == 0:
            assert trunc.all()
            assert np.array_equal(infos["episode"]["r"].cpu().numpy(), total) and total.min() < 0
            assert (infos["episode"]["l"] == limit).all()
            total[:] = 0
        else:
            assert not trunc.any()
    env.close()


def test_snapshot_restores_the_whole_state(cge):
    n = 300
    env = cge.BusVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=8)
    env.rollout(237, action_seed=4)
    snap = env.snapshot()
    first = env.rollout(400, action_seed=6, t0=237, trajectory=True, per_step=True)      # crosses the time limit: resets draw
    first = [host(env, first[0])] + [x.clone() for x in first[1:]]
    env.restore(snap)
    again = env.rollout(400, action_seed=6, t0=237, trajectory=True, per_step=True)
    same(host(env, again[0]), first[0], "trajectory")
    for x, y in zip(again[1:], first[1:]):
        assert torch.equal(x, y)
    assert int(first[4].sum()) == n
    env.close()


def test_invalid_action_leaves_the_env_untouched(cge):
    n = 300
    env = cge.BusVectorEnv(n, autoreset_mode="SameStep", reference_info=True)
    env.reset(seed=2)
    acts = torch.from_numpy(bm.hash_actions(3, 12, n)).cuda()
    for t in range(10):
        obs, *_ = env.step(acts[t])
    before = host(env, obs)
    env.check_actions()                                                # nothing so far
    bad = acts[10].clone()
    bad[5, 2] = 11
    bad[77, 0] = -1
    obs, rew, term, trunc, infos = env.step(bad)
    after = host(env, obs)
    good = np.ones(n, bool)
    good[[5, 77]] = False
    same(after, before, "refused envs", ~good)
    assert (after["timestep"][good] == 11).all() and (rew[[5, 77]] == 0).all() and not trunc.any()
    for key, obs_key in [("timestep", "timestep"), ("total_delivered", "total_delivered"), ("total_waiting", "total_waiting"),
                         ("total_onboard", "total_onboard"), ("bus_positions", "bus_stops"), ("bus_states", "bus_states"),
                         ("bus_capacities", "bus_capacities"), ("stop_waiting", "stop_waiting_counts")]:
        assert np.array_equal(infos[key].cpu().numpy(), after[obs_key]), key      # the reference's info dict, its keys
    with pytest.raises(ValueError):
        env.check_actions()
    env.check_actions()                                                # the counter was read: clean again
    twin = cge.BusVectorEnv(n, autoreset_mode="SameStep")              # the refused envs go on as if the bad step had not happened
    twin.reset(seed=2)
    for t in range(10):
        twin.step(acts[t])
    o1, *_ = env.step(acts[11])
    o2, *_ = twin.step(acts[11])
    same(host(env, o1), host(twin, o2), "after the refusal", ~good)
    env.close(); twin.close()


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_captured_steps_replay_and_match_the_model(cge, mode):
    K, n, limit = 32, 1000, 13
    env = cge.BusVectorEnv(n, autoreset_mode=mode, max_timesteps=limit, reuse_buffers=True)
    m = bm.BusModel(9 + np.arange(n), limit, MODES[mode])
    env.reset(seed=9)
    m.reset()
    acts_h = bm.hash_actions(21, K, n)
    acts = torch.from_numpy(acts_h).cuda()
    w = warm_up(lambda: env.step(acts[0]))                             # on a side stream: the persistent buffers get allocated
    same(host(env, w[0]), m.step(acts_h[0])[0], "warm-up")
    hist = {"obs": torch.empty((K, n * 56), dtype=torch.int32, device="cuda"), "rew": torch.empty((K, n), device="cuda"),
            "trunc": torch.empty((K, n), dtype=torch.bool, device="cuda")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(K):
            ob, r, te, tr, _ = env.step(acts[t])
            hist["obs"][t].copy_(env.obs_slab(ob)); hist["rew"][t].copy_(r); hist["trunc"][t].copy_(tr)
    for rep in range(2):                                               # the same graph twice: the state carries over, the actions repeat
        g.replay()
        torch.cuda.synchronize()
        got = kit.decode(env, hist["obs"])
        for t in range(K):
            mo, mr, _, mtr, _ = m.step(acts_h[t])
            same(take(got, t), mo, (rep, t))
            assert np.array_equal(hist["rew"][t].cpu().numpy().astype(np.float64), mr) and np.array_equal(hist["trunc"][t].cpu().numpy(), mtr)
    assert int(hist["trunc"].sum()) > 0                                # in-kernel resets happened inside the graph
    env.close()


def test_one_million_envs(cge):
    n, T, chunk, a_seed, seed = 1 << 20, 520, 8, 31, 6
    sample = np.arange(512, dtype=np.int64) * 2048 + 7                 # a fixed sample of envs for the model
    sidx = torch.from_numpy(sample).cuda()
    env = cge.BusVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    m = bm.BusModel(seed + sample, 500, bm.SAME_STEP)
    obs, _ = env.reset(seed=seed)
    same(take(host(env, obs), sample), m.reset(), "reset")
    total = obs["total_waiting"].clone()                               # waiting + onboard + delivered of the running episode
    assert int(total.min()) >= 50 and int(total.max()) <= 150 and int(obs["total_delivered"].max()) == 0
    acts = bm.hash_actions(a_seed, T, 512, envs=sample)
    ends = 0
    for t0 in range(0, T, chunk):
        traj, rt, tt, rs, dc = env.rollout(chunk, action_seed=a_seed, t0=t0, trajectory=True, per_step=True)
        cap = traj["bus_capacities"]
        assert int(cap.min()) >= 0 and int(cap.max()) <= 20
        assert torch.equal(20 - traj["bus_passenger_destinations"].sum(-1, dtype=torch.int32), cap)
        assert torch.equal(traj["stop_destination_distributions"].sum(-1, dtype=torch.int32), traj["stop_waiting_counts"])
        tot = traj["total_waiting"] + traj["total_onboard"] + traj["total_delivered"]
        for j in range(chunk):
            fresh = tt[j]                                              # truncated: the slot holds the new episode's reset observation
            assert bool(((tot[j] == total) | fresh).all()), t0 + j
            if bool(fresh.any()):
                assert bool(fresh.all()) and t0 + j == 499             # every env hits the time limit in the same step
                assert int(tot[j].min()) >= 50 and int(tot[j].max()) <= 150
                assert int(traj["total_delivered"][j].max()) == 0 and int(traj["timestep"][j].max()) == 0
                ends += 1
            total = tot[j].clone()
        sub = {k: traj[k][:, sidx].cpu().numpy() for k in bm.KEYS}
        rsub, tsub = rt[:, sidx].cpu().numpy(), tt[:, sidx].cpu().numpy()
        for j in range(chunk):
            mo, mr, _, mtr, _ = m.step(acts[t0 + j])
            same(take(sub, j), mo, t0 + j)
            assert np.array_equal(rsub[j].astype(np.float64), mr) and np.array_equal(tsub[j], mtr), t0 + j
    assert ends == 1
    env.close()
