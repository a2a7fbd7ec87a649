"""RestaurantVectorEnv on the device against the unmodified reference (tests/golden/restaurant_*.npz) and, where the fixtures cannot
reach, against the model that tests/test_restaurant_cpu.py pins to them (tests/restaurant_model.py).  The helpers and the bodies shared
with bus and world builder are in tests/_slab_kit.py.  Every comparison is array_equal and skips no rows; rewards are the reference's
float64 sums rounded to the float32 of the output buffer."""
import json
import types

import numpy as np
import pytest
import torch

import _slab_kit as kit
import restaurant_model as rm
from _slab_kit import MODES, cge, f32, host, same, take, warm_up  # noqa: F401
from _slab_kit import dev as packed
from conftest import golden

pytestmark = pytest.mark.gpu

FIXTURES = ["restaurant_hash.npz", "restaurant_busy.npz", "restaurant_short.npz", "restaurant_short40.npz", "restaurant_long.npz"]
SPEC = types.SimpleNamespace(
    m=rm, env="RestaurantVectorEnv", model=rm.RestaurantModel, limit="max_episode_steps", from_fixture={"max_episode_steps": "max_episode_steps"},
    flag="truncated", keys=rm.KEYS, shapes=rm.KEY_SHAPES, dtypes=dict.fromkeys(rm.KEYS, np.int32), column=(), exact_reward=False,
    rollout=types.SimpleNamespace(
        n=200, limit=90, longest=125, ends=1, info=("total_reward", "wait_time_sum", "num_customers"),
        given=lambda *a, **kw: packed(rm.busy_actions(*a, **kw)),
        pre=lambda n, env0: packed(rm.busy_actions(1, 40, n, env0=env0))),
    sharding=types.SimpleNamespace(n=333, k=130, kw={"max_episode_steps": 100}, shards=[(0, 167), (167, 166)], ends=lambda dw: int(dw.min()) == 1))


def test_observation_is_a_dict_of_views_of_one_slab(cge):
    env = cge.RestaurantVectorEnv(300, autoreset_mode="SameStep")
    obs, _ = env.reset(seed=1)
    assert list(obs) == list(rm.KEYS)
    base = obs["waiting_customers"].data_ptr()
    start = 0                                                             # plane starts inside the slab, in ints
    for k in rm.KEYS:
        t = obs[k]
        assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (300,) + rm.KEY_SHAPES[k] and t.is_contiguous(), k
        assert t.data_ptr() == base + 4 * start, k
        start += 300 * int(np.prod(rm.KEY_SHAPES[k]))
        assert not t.any(), k                                             # an empty restaurant
    assert tuple(env.obs_slab(obs).shape) == (300 * 341,)
    assert sorted(env.single_action_space.spaces) == sorted(rm.ACTION_KEYS)
    for c, k in enumerate(rm.ACTION_KEYS):
        assert [int(v) for v in env.action_space[k].nvec] == [rm.NVEC[c]] * 300
    a = env.action_sampler(0).sample()
    assert sorted(a) == sorted(rm.ACTION_KEYS) and all(v.dtype == torch.int32 and tuple(v.shape) == (300,) for v in a.values())
    o, r, te, tr, infos = env.step(a)
    assert r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool and not te.any() and "final_obs" in infos
    assert env.last_kernel() == "cge::restaurant::step_kernel<1>"         # the instance a profile of this call shows (1 = SameStep)
    traj, rs, dc = env.rollout(3, action_seed=1, trajectory=True)
    assert tuple(traj["kitchen_queue"].shape) == (3, 300, 50, 3) and tuple(env.obs_slab(traj).shape) == (3, 300 * 341)
    assert env.last_kernel() == "cge::restaurant::rollout_kernel<1, false>"
    assert env.device_bytes() == 300 * (11 * 16 + 640 * 4) + 8
    env.close()
    env = cge.RestaurantVectorEnv(5, reference_info=True, info_fields=("idle_waiters",))     # the reference's info keys in every infos
    _, infos = env.reset(seed=1)
    assert (infos["idle_waiters"] == 10).all() and not infos["average_wait_time"].any() and not infos["episode_stats"]["customers_served"].any()
    infos = env.step(torch.zeros((5, 4), dtype=torch.int32, device="cuda"))[4]
    assert (infos["current_timestep"] == 1).all() and infos["total_reward"].dtype == torch.float64 and (infos["total_reward"] == 0.9).all()
    env.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_same_step(cge, name):
    kit.fixtures_same_step(cge, SPEC, name)


@pytest.mark.parametrize("name", ["restaurant_short.npz", "restaurant_short40.npz"])
@pytest.mark.parametrize("mode", ["NextStep", "Disabled"])
def test_short_fixture_in_the_other_modes(cge, mode, name):
    z = golden(name)
    limit, seed, acts = int(z["max_episode_steps"]), int(z["seed0"]), z["actions"].transpose(1, 0, 2).astype(np.int32)
    kit.model_parity(cge, SPEC, mode, limit, seed + np.arange(len(acts[0])), acts, (limit + 3, 3 * limit + 1), seed=seed)


def test_info_parity_at_every_step(cge):
    """info() and reference_info() against the reference's recorded _get_info: Disabled mode with the caller's reset after each
    time limit, so the counters of the truncated steps are the reference's too."""
    z = golden("restaurant_busy.npz")
    n, T = z["reward"].shape
    env = cge.RestaurantVectorEnv(n, autoreset_mode="Disabled", info_fields=("total_reward", "wait_time_sum"))
    env.reset(seed=int(z["seed0"]))
    acts = packed(z["actions"].transpose(1, 0, 2))
    fields = ("timestep",) + rm.INFO[1:]
    info_keys, stat_keys = ([str(k) for k in json.loads(str(z[name]))] for name in ("info_keys", "stat_keys"))
    top = ("current_timestep", "waiting_customers", "idle_waiters", "kitchen_queue_length", "ready_orders", "dirty_tables")
    assert stat_keys[:4] == ["customers_served", "customers_left", "tables_cleaned", "orders_served"] and len(stat_keys) == 6
    for t in range(T):
        _, _, _, trunc, infos = env.step(acts[t])
        got = torch.stack([env.info(f) for f in fields] + [infos["total_reward"], infos["wait_time_sum"]], 1)
        assert got.dtype == torch.float64
        got = got.cpu().numpy()                                           # one copy per step
        want = z["info"][:, t].astype(np.float64)
        assert np.array_equal(got[:, :12], want) and np.array_equal(got[:, 13], want[:, 10]), t
        assert np.array_equal(got[:, 12].view(np.uint64), z["total_reward"][:, t].view(np.uint64)), t
        ri = env.reference_info()                                         # the reference's own dict, at every step as well
        assert list(ri) == info_keys and list(ri["episode_stats"]) == stat_keys
        flat = [ri[k] for k in top] + [ri["episode_stats"][k] for k in stat_keys] + [ri["average_wait_time"], ri["total_reward"]]
        assert all(v.dtype == torch.float64 and tuple(v.shape) == (n,) for v in flat)
        flat = torch.stack(flat, 1).cpu().numpy()
        assert np.array_equal(flat[:, :10], want[:, :10]) and not flat[:, 10:12].any(), t        # (total_wait_time, average_wait_time: never updated)
        assert np.array_equal(flat[:, 12].view(np.uint64), z["average_wait_time"][:, t].view(np.uint64)), t
        assert np.array_equal(flat[:, 13].view(np.uint64), z["total_reward"][:, t].view(np.uint64)), t
        if trunc.any():
            assert trunc.all()
            env.reset()
    env.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_kernel_against_the_model(cge, n):
    """A partial last wave and plane runs that end mid-line: 520 steps of the busy policy across the step-500 reset."""
    T, env0 = 520, 1000
    env = cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", env_index0=env0)
    m = rm.RestaurantModel(5 + env0 + np.arange(n), 500, rm.SAME_STEP)
    obs, _ = env.reset(seed=5)
    same(host(env, obs), m.reset(), "reset")
    acts = rm.busy_actions(11, T, n, env0=env0)
    dacts = packed(acts)
    for t in range(T):
        obs, rew, term, trunc, infos = env.step(dacts[t])
        mo, mr, _, mtr, mf = m.step(acts[t])
        same(host(env, obs), mo, (t, "obs"))
        assert np.array_equal(rew.cpu().numpy(), f32(mr)) and not term.any() and np.array_equal(trunc.cpu().numpy(), mtr), t
        if mtr.any():
            assert t == 499 and mtr.all()
            same(host(env, infos["final_obs"]), mf, (t, "final_obs"))
    assert np.array_equal(env.info("total_reward").cpu().numpy().view(np.uint64), m.total_reward().view(np.uint64))
    assert np.array_equal(env.info("customers_served").cpu().numpy(), m.info()[:, 6].astype(np.float64))
    env.close()


@pytest.mark.parametrize("k", [1, 7, 125])
@pytest.mark.parametrize("given", [False, True], ids=["hash", "given"])
@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_rollout_equals_k_steps(cge, mode, given, k):
    kit.rollout_equals_k_steps(cge, SPEC, mode, given, k)


def test_rollout_replays_the_busy_fixture(cge):
    z = golden("restaurant_busy.npz")
    n = z["reward"].shape[0]
    env = cge.RestaurantVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=int(z["seed0"]))
    acts = packed(z["actions"].transpose(1, 0, 2))
    recorded = kit.pieces(SPEC, z, "obs_")
    t0 = 0
    for k in (125, 125, 125, 125, 20):
        traj, rt, tt, rs, dc = env.rollout(k, actions=acts[t0:t0 + k], trajectory=True, per_step=True)
        th = host(env, traj)
        tr = tt.cpu().numpy()
        assert np.array_equal(rt.cpu().numpy(), f32(z["reward"][:, t0:t0 + k].T)) and np.array_equal(tr, z["truncated"][:, t0:t0 + k].T.astype(bool))
        for j in range(k):
            ref = take(recorded, slice(None), t0 + j)
            same(take(th, j), ref, t0 + j, ~tr[j])
            if tr[j].any():                                               # the slot of a truncated step holds the reset observation
                assert t0 + j == 499 and tr[j].all() and not th["waiting_customers"][j].any() and not th["current_timestep"][j].any()
        t0 += k
    env.close()


def test_dict_actions_equal_packed_actions(cge):
    n, k = 130, 60
    a, b = (cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", max_episode_steps=40) for _ in range(2))
    a.reset(seed=12); b.reset(seed=12)
    acts = rm.busy_actions(3, k + 10, n)
    for t in range(k):
        form = {key: torch.from_numpy(acts[t, :, c].astype(np.int64)).cuda() for c, key in enumerate(rm.ACTION_KEYS)}
        if t % 2:
            form = {key: acts[t, :, c] for c, key in enumerate(rm.ACTION_KEYS)}     # host arrays too
        ra, rb = a.step(form), b.step(packed(acts[t]))
        same(host(a, ra[0]), host(b, rb[0]), t)
        assert torch.equal(ra[1], rb[1]) and torch.equal(ra[3], rb[3]), t
    form = {key: packed(acts[k:, :, c]) for c, key in enumerate(rm.ACTION_KEYS)}
    ra = a.rollout(10, actions=form, trajectory=True, per_step=True)
    rb = b.rollout(10, actions=packed(acts[k:]), trajectory=True, per_step=True)
    same(host(a, ra[0]), host(b, rb[0]), "rollout")
    assert all(torch.equal(x, y) for x, y in zip(ra[1:], rb[1:]))
    with pytest.raises(ValueError):
        a.step({key: acts[0, :, c] for c, key in enumerate(rm.ACTION_KEYS[:3])})
    a.close(); b.close()


def test_step_on_sampled_actions(cge):
    """env.step(env.action_sampler(3).sample()) equals stepping on what the batched Dict space seeded with 3 samples on the host: one
    PCG64 stream per key in sorted key order, one random() per element, int(u * n)."""
    n = 200
    env, twin = (cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", max_episode_steps=30) for _ in range(2))
    env.reset(seed=4); twin.reset(seed=4)
    sampler = env.action_sampler(3)
    keys = sorted(rm.ACTION_KEYS)
    sub = np.random.default_rng(3).integers(2**31 - 1, size=4)
    rngs = {k: np.random.default_rng(int(s)) for k, s in zip(keys, sub)}
    bound = dict(zip(rm.ACTION_KEYS, rm.NVEC))
    for t in range(50):
        ref = {k: (rngs[k].random(n) * bound[k]).astype(np.int64) for k in keys}
        s = sampler.sample()
        for k in keys:
            assert np.array_equal(s[k].cpu().numpy(), ref[k]), (t, k)
        r1 = env.step(s)
        r2 = twin.step(packed(np.stack([ref[k] for k in rm.ACTION_KEYS], 1)))
        same(host(env, r1[0]), host(twin, r2[0]), t)
        assert torch.equal(r1[1], r2[1]) and torch.equal(r1[3], r2[3]), t
    assert env.invalid_action_count() == 0
    env.close(); twin.close()


def test_out_of_range_and_negative_components_change_nothing(cge):
    n = 130
    env, twin = (cge.RestaurantVectorEnv(n, autoreset_mode="SameStep") for _ in range(2))
    m = rm.RestaurantModel(2 + np.arange(n), 500, rm.SAME_STEP)
    env.reset(seed=2); twin.reset(seed=2); m.reset()
    acts = rm.busy_actions(3, 90, n)
    for t in range(60):                                                   # a busy restaurant first
        env.step(packed(acts[t])); twin.step(packed(acts[t])); m.step(acts[t])
    env.check_actions()                                                   # nothing so far
    bad_count = 0
    for t in range(60, 90):
        bad, noop = acts[t].copy(), acts[t].copy()
        rows = np.arange(n) % 5 == t % 5
        col = t % 4
        bad[rows, col] = [rm.NVEC[col], rm.NVEC[col] + 7, -1, -(2 ** 31), 2 ** 31 - 1][t % 5]
        noop[rows, 0] = 3                                                 # "Do Nothing"
        r1, r2 = env.step(packed(bad)), twin.step(packed(noop))
        mo, mr, _, _, _ = m.step(bad)
        same(host(env, r1[0]), host(twin, r2[0]), t)
        same(host(env, r1[0]), mo, (t, "model"))
        assert torch.equal(r1[1], r2[1]) and np.array_equal(r1[1].cpu().numpy(), f32(mr)), t
        bad_count += int(rows.sum())
    assert m.invalid == bad_count == 30 * 26 and env.invalid_action_count() == bad_count   # one per env-step, whatever the component
    assert env.invalid_action_count() == 0 and twin.invalid_action_count() == 0           # reading clears it; the twin saw none
    two = acts[0].copy()
    two[[3, 129], 1] = [10, -1]                                           # two more, the last lane of the partial wave among them
    two[3, 2] = 50                                                        # (two bad components of one env count once)
    env.step(packed(two))
    with pytest.raises(ValueError, match="Invalid action in 2 env-step"):
        env.check_actions()
    env.check_actions()                                                   # the counter was read: clean again
    env.step(packed(acts[0]))
    assert env.invalid_action_count() == 0
    env.close(); twin.close()


def test_snapshot_round_trip_into_a_fresh_handle(cge):
    n = 200
    env = cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", max_episode_steps=300)
    env.reset(seed=8)
    env.rollout(237, actions=packed(rm.busy_actions(4, 237, n)))
    fresh = cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", max_episode_steps=300)
    fresh.restore(env.snapshot())
    acts = packed(rm.busy_actions(6, 100, n, t0=237))
    for t in range(100):                                                  # crosses the time limit
        r1, r2 = env.step(acts[t]), fresh.step(acts[t])
        same(host(env, r1[0]), host(fresh, r2[0]), t)
        assert torch.equal(r1[1], r2[1]) and torch.equal(r1[3], r2[3]), t
    assert torch.equal(env.info("total_reward"), fresh.info("total_reward")) and int(env.info("timestep")[0]) == 37
    other = cge.RestaurantVectorEnv(n + 1)
    with pytest.raises(ValueError):
        other.restore(env.snapshot())
    env.close(); fresh.close(); other.close()


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_episode_statistics(cge, mode):
    n, limit, T = 130, 45, 140
    env = cge.RestaurantVectorEnv(n, autoreset_mode=mode, max_episode_steps=limit, record_episode_statistics=True)
    m = rm.RestaurantModel(5 + np.arange(n), limit, MODES[mode])
    env.reset(seed=5); m.reset()
    acts = rm.busy_actions(2, T, n)
    ends = 0
    for t in range(T):
        _, rew, _, trunc, infos = env.step(packed(acts[t]))
        _, mr, _, mtr, _ = m.step(acts[t])
        assert torch.equal(infos["_episode"], trunc) and np.array_equal(trunc.cpu().numpy(), mtr), t
        er, el = m.episode_stats()
        assert np.array_equal(infos["episode"]["r"].cpu().numpy().view(np.uint64), er.view(np.uint64)), t
        assert np.array_equal(infos["episode"]["l"].cpu().numpy(), el), t
        ends += int(mtr.sum())
    assert ends >= 2 * n and (m.episode_stats()[1] == limit).all()
    # a fused launch keeps them too
    r, l = env.episode_statistics()
    before = r.clone()
    env.rollout(limit, action_seed=1)
    assert not torch.equal(env.episode_statistics()[0], before) and (l == limit).all()
    env.close()


def test_sharding_invariance(cge):
    kit.sharding_invariance(cge, SPEC)


# ---------------------------------------------------------------------------------------------------------------- graph capture
# the method of tests/test_graph_capture_gpu.py: reuse_buffers=True, a warm-up on a side stream, the calls captured into one
# torch.cuda.CUDAGraph, replayed four times, every output compared with an eager twin that makes the same calls one by one
REPLAYS = 4


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_captured_steps_replay_and_match_an_eager_twin(cge, mode):
    K, n, limit = 32, 333, 13
    env = cge.RestaurantVectorEnv(n, autoreset_mode=mode, max_episode_steps=limit, reuse_buffers=True)
    twin = cge.RestaurantVectorEnv(n, autoreset_mode=mode, max_episode_steps=limit)
    env.reset(seed=9); twin.reset(seed=9)
    acts = packed(rm.busy_actions(21, K, n))
    w = warm_up(lambda: env.step(acts[0]))
    t0 = twin.step(acts[0])
    assert torch.equal(env.obs_slab(w[0]), twin.obs_slab(t0[0])) and torch.equal(w[1], t0[1])
    hist = {"obs": torch.empty((K, n * 341), dtype=torch.int32, device="cuda"), "rew": torch.empty((K, n), device="cuda"),
            "trunc": torch.empty((K, n), dtype=torch.bool, device="cuda")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(K):
            ob, r, te, tr, _ = env.step(acts[t])
            hist["obs"][t].copy_(env.obs_slab(ob)); hist["rew"][t].copy_(r); hist["trunc"][t].copy_(tr)
    for rep in range(REPLAYS):                                            # the same graph again: the state carries over, the actions repeat
        g.replay()
        torch.cuda.synchronize()
        for t in range(K):
            ob, r, te, tr, _ = twin.step(acts[t])
            assert torch.equal(hist["obs"][t], twin.obs_slab(ob)) and torch.equal(hist["rew"][t], r) and torch.equal(hist["trunc"][t], tr), (rep, t)
    assert int(hist["trunc"].sum()) > 0                                   # in-kernel resets happened inside the graph
    r1, r2 = env.step(acts[1]), twin.step(acts[1])                        # the host's view after the replays: one more eager step
    assert torch.equal(env.obs_slab(r1[0]), twin.obs_slab(r2[0])) and torch.equal(r1[1], r2[1])
    env.close(); twin.close()


@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_captured_rollout_replays_and_matches_an_eager_twin(cge, mode):
    k, n, limit = 16, 333, 13
    env = cge.RestaurantVectorEnv(n, autoreset_mode=mode, max_episode_steps=limit, reuse_buffers=True)
    twin = cge.RestaurantVectorEnv(n, autoreset_mode=mode, max_episode_steps=limit)
    env.reset(seed=6); twin.reset(seed=6)

    def call(e):
        traj, rt, tt, rs, dc = e.rollout(k, action_seed=77, t0=1000, trajectory=True, per_step=True)
        return [e.obs_slab(traj), rt, tt, rs, dc]

    w = warm_up(lambda: call(env))
    for x, y in zip(w, call(twin)):
        assert torch.equal(x, y)
    hist = [torch.empty_like(x) for x in w]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for dst, src in zip(hist, call(env)):
            dst.copy_(src)
    ends = 0
    for rep in range(REPLAYS):
        g.replay()
        torch.cuda.synchronize()
        for j, (x, y) in enumerate(zip(hist, call(twin))):
            assert x.dtype == y.dtype and torch.equal(x, y), (rep, j)
        ends += int(hist[4].sum())
    assert ends > 0
    env.close(); twin.close()


def test_refusals(cge):
    for bad in (0, 1001, -5):
        with pytest.raises(ValueError, match="max_episode_steps"):
            cge.RestaurantVectorEnv(8, max_episode_steps=bad)
    for ok in (1, 1000):
        cge.RestaurantVectorEnv(8, max_episode_steps=ok).close()
    with pytest.raises(cge.NativeLibraryError):
        cge.RestaurantVectorEnv(8, device="cpu")
    env = cge.RestaurantVectorEnv(8, info_fields=("timestep",))
    env.reset(seed=0)
    for shape in ((8,), (8, 3), (7, 4), (2, 8, 4)):
        with pytest.raises(ValueError):
            env.step(torch.zeros(shape, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.rollout(3, actions=torch.zeros((2, 8, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.step({k: torch.zeros(7, dtype=torch.int32, device="cuda") for k in rm.ACTION_KEYS})
    odd = torch.zeros(8 * 4 + 1, dtype=torch.int32, device="cuda")[1:].view(8, 4)     # contiguous, but 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte"):
        env.step(odd)
    with pytest.raises(ValueError, match="16-byte"):
        env.rollout(1, actions=odd[None])
    assert env._lib.cge_restaurant_step(env._h, odd.data_ptr(), odd.data_ptr(), odd.data_ptr(), odd.data_ptr(), odd.data_ptr(), None, None) == -1
    assert b"16-byte aligned" in env._lib.cge_restaurant_last_error(env._h)
    with pytest.raises(ValueError):
        cge.RestaurantVectorEnv(8, info_fields=("no_such_field",))
    with pytest.raises(TypeError):
        env.info("timestep", 1)                                           # the fields are not indexed
    _, _, _, _, infos = env.step(torch.zeros((8, 4), dtype=torch.int32, device="cuda"))
    assert (infos["timestep"] == 1).all()
    env.close()


def test_one_million_envs(cge):
    n, T, a_seed, seed = 1 << 20, 3, 31, 6
    sample = np.concatenate([np.arange(1365), n // 2 + np.arange(1366), n - 1365 + np.arange(1365)])   # first, middle, last: 4,096 envs
    sidx = torch.from_numpy(sample).cuda()
    env = cge.RestaurantVectorEnv(n, autoreset_mode="SameStep", reuse_buffers=True)
    assert env.device_bytes() == n * (11 * 16 + 640 * 4) + 8
    m = rm.RestaurantModel(seed + sample, 500, rm.SAME_STEP)
    obs, _ = env.reset(seed=seed)
    assert not env.obs_slab(obs).any()
    m.reset()
    acts = rm.hash_actions(a_seed, T, len(sample), envs=sample)
    traj, rt, tt, rs, dc = env.rollout(T, action_seed=a_seed, trajectory=True, per_step=True)
    assert not tt.any() and int(traj["current_timestep"].min()) == 1 and int(traj["current_timestep"].max()) == T
    assert bool((traj["current_timestep"][:, :, 0] == torch.arange(1, T + 1, device="cuda", dtype=torch.int32)[:, None]).all())
    assert 0 < int((traj["waiting_customers"][T - 1, :, 0, 1] > 0).sum()) < n      # some envs have had an arrival, not all
    assert int(traj["table_occupancy"].max()) == 0 and not traj["waiting_customers"][:, :, 2:].any()
    sub = {k: traj[k][:, sidx].cpu().numpy() for k in rm.KEYS}
    rsub = rt[:, sidx].cpu().numpy()
    for j in range(T):
        mo, mr, _, mtr, _ = m.step(acts[j])
        same(take(sub, j), mo, j)
        assert np.array_equal(rsub[j], f32(mr)) and not mtr.any(), j
    env.close()
