"""AgriculturalFarmVectorEnv on the device against the unmodified reference (tests/golden/farm_*.npz) and, where the fixtures cannot
reach, against the model that tests/test_farm_cpu.py pins to them (tests/farm_model.py).  Every comparison is array_equal on bit
patterns and skips no rows; rewards are the reference's float64 values rounded to the float32 of the output buffer (integers: exact)."""
import types

import numpy as np
import pytest
import torch

import _lane_kit as kit
import farm_model as fm
from _lane_kit import cge, dev, f32, same  # noqa: F401
from conftest import golden

pytestmark = pytest.mark.gpu

MODES = kit.MODES
PER_ENV = 832 + 2 * 2560                                                  # the documented device bytes per env: record + two generators
INFO27 = fm.INFO + fm.FIELD_INFO                                          # eleven [N] and four [N, 4]: the 27 columns of a fixture's info row
NO_PRICE = [c for c in range(27) if c not in (3, 4, 6)]                   # all but cash_flow, total_revenue, profit_margin: what no price reaches
ENDING = ["farm_hash.npz", "farm_bankrupt.npz", "farm_orchard.npz", "farm_chores.npz", "farm_two_years.npz"]      # every one holds an end and its reset


def live(obs, rows=None):
    """the 134 live columns of full rows (of `rows` only: final_obs is specified where terminated), after asserting that the padding is zero"""
    o = obs.cpu().numpy() if isinstance(obs, torch.Tensor) else obs
    o = o if rows is None else o[rows]
    assert o.shape[-1] == 620 and not o[..., 134:].view(np.uint32).any()
    return o[..., :134]


SPEC = types.SimpleNamespace(
    m=fm, kind="farm", env="AgriculturalFarmVectorEnv", model=fm.FarmModel, limit="max_years", short=("farm_two_years.npz", 2),
    obs=620, actions=45, info=INFO27, clock="day", live=live,
    ending=ENDING,
    disabled=("farm_bankrupt.npz", lambda ends: ends == 8),
    overrun=("farm_overrun.npz", lambda z: z["terminated"].any()),
    next_step=("farm_hash.npz", lambda n: 8),
    bad=(45, 57),
    sampled_steps=2)


def info27(env):
    return kit.info_of(SPEC, env)


def test_surface(cge):
    env = cge.AgriculturalFarmVectorEnv(300, autoreset_mode="SameStep")
    obs, infos = env.reset(seed=1)
    assert obs.dtype == torch.float32 and tuple(obs.shape) == (300, 620) and obs.is_cuda and infos == {}
    assert int(env.single_action_space.n) == 45 and tuple(env.single_observation_space.shape) == (620,) and env.single_observation_space.dtype == np.float32
    assert float(env.single_observation_space.low.max()) == -np.inf and float(env.single_observation_space.high.min()) == np.inf
    assert [int(v) for v in env.action_space.nvec] == [45] * 300 and tuple(env.observation_space.shape) == (300, 620)
    o, r, te, tr, infos = env.step(torch.full((300,), 41, dtype=torch.int32, device="cuda"))
    assert r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool and not tr.any() and "final_obs" in infos
    assert env.last_kernel() == "cge::farm::step_kernel<1>"               # the instance a profile of this call shows (1 = SameStep)
    traj, rs, dc = env.rollout(3, action_seed=1, trajectory=True)
    assert tuple(traj.shape) == (3, 300, 620) and env.last_kernel() == "cge::farm::rollout_kernel<1, false>"
    assert env.device_bytes() == 300 * PER_ENV + 8
    env.close()
    env = cge.AgriculturalFarmVectorEnv(300, compact_obs=True)
    assert tuple(env.single_observation_space.shape) == (134,) and tuple(env.reset(seed=1)[0].shape) == (300, 134) and env.device_bytes() == 300 * PER_ENV + 8
    env.close()
    env = cge.AgriculturalFarmVectorEnv(5, reference_info=True, info_fields=("water_quality", "needs_reset"))
    _, infos = env.reset(seed=1)
    assert list(infos)[2:] == list(INFO27) and (infos["cash_flow"] == 50000.0).all() and (infos["year"] == 1).all() and (infos["water_quality"] == 0.9).all()
    assert all(tuple(infos[k].shape) == (5,) for k in fm.INFO) and all(tuple(infos[k].shape) == (5, 4) and infos[k].dtype == torch.float64 for k in fm.FIELD_INFO)
    assert infos["field_crop"].tolist() == [[-1.0, 1.0, 2.0, -1.0]] * 5 and (infos["field_stage"] == 7).all()    # wheat prints "None"
    infos = env.step(torch.full((5,), 41, dtype=torch.int32, device="cuda"))[4]
    assert (infos["day"] == 1).all() and (infos["season"] == 0).all() and (infos["carbon_sequestered"] > 1.0).all() and infos["profit_margin"].dtype == torch.float64
    env.close()


@pytest.mark.parametrize("name", ENDING + ["farm_soil.npz"])
def test_fixtures_same_step(cge, name):
    kit.fixtures_same_step(cge, SPEC, name)


def test_poked_fixture_same_step(cge):
    """farm_poked.npz: the reference with maintenance_needed, excessive_rain_days, a pest level and a yield potential set from outside
    between steps (states its own arithmetic keeps out of reach from reset()).  The device gets the same pokes through snapshot() and
    restore(), at the word offsets the host build of csrc/farm_env.hpp reports, and is then compared like any other fixture."""
    pokes = fm.fixture_pokes(golden("farm_poked.npz"))
    assert len(pokes) >= 15
    assert kit.replay_same_step(cge, SPEC, "farm_poked.npz", pokes) == (0, 0)


def test_bankrupt_fixture_disabled_with_masked_resets(cge):
    kit.disabled_with_masked_resets(cge, SPEC)


def test_overrun_fixture_steps_on_past_termination(cge):
    """Disabled, never reset: every env runs on past its first `terminated` into the second year's climate"""
    kit.overrun_fixture_steps_on_past_termination(cge, SPEC)


def test_hash_fixture_next_step_against_the_model(cge):
    kit.hash_fixture_next_step_against_the_model(cge, SPEC)


@pytest.mark.parametrize("mode", ["SameStep", "NextStep", "Disabled"])
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_rollout_equals_steps_and_the_model(cge, mode, given, n):
    """a single lane, a partial wave, one lane into the next wave.  rollout(37) against 37 step() calls of a twin and against the
    model, after 330 fused steps that both have taken: the window holds the year's end at day 360 (and the autoreset or the overrun
    that follows) and several twists of the NumPy stream.  Observations, rewards and flags are compared with the model at every step.
    The float64 info values at the end are compared with the model where no price can reach them, and with the twin everywhere:
    a price holds the device's `log`, which is a last place off glibc's in one Gaussian pair of a few thousand (the documented caveat;
    profiles/farm_timing.txt), and cash_flow, total_revenue and profit_margin add such prices up over the 367 steps of this run, in
    Disabled mode without a reset in between; their float32 forms in the observation are compared above."""
    k, lead, a_seed = 37, 330, 12
    env, twin = (cge.AgriculturalFarmVectorEnv(n, autoreset_mode=mode, env_index0=1000) for _ in range(2))
    m = fm.FarmModel(40 + 1000 + np.arange(n), MODES[mode])
    same(env.reset(seed=40)[0], m.reset(), "reset"); twin.reset(seed=40)
    acts = fm.hash_actions(a_seed, lead + k, n, env0=1000)                # what rollout(actions=None) stands for
    if given:
        acts[:, ::2] = np.where(acts[:, ::2] == 40, 3, acts[:, ::2])      # another policy for every other env
    early = np.zeros(n, bool)                                             # a bankruptcy during the lead moves that env's year
    for t in range(lead):
        mo, _, mt = m.step(acts[t])[:3]
        early |= mt
    d = dev(acts)
    lead_obs = env.rollout(lead, actions=d[:lead] if given else None, action_seed=a_seed)[0]
    twin.rollout(lead, actions=d[:lead] if given else None, action_seed=a_seed)
    same(lead_obs, mo, "the last row of the lead")
    traj, rt, tt, rs, dc = env.rollout(k, actions=d[lead:] if given else None, action_seed=a_seed, t0=lead, trajectory=True, per_step=True)
    sums = np.zeros(n)
    for t in range(k):
        o, r, te, _, _ = twin.step(d[lead + t])
        assert torch.equal(traj[t], o) and torch.equal(rt[t], r) and torch.equal(tt[t], te), t
        mo, mr, mt = m.step(acts[lead + t])[:3]
        same(o, mo, t); same(r, f32(mr), t)
        assert np.array_equal(te.cpu().numpy(), mt), t
        sums += f32(mr).astype(np.float64)
    same(rs, sums, "reward_sum")
    assert torch.equal(dc, tt.sum(0).int()) and not early[0] and (dc.cpu().numpy()[~early] >= 1).all()   # day 360 is inside, for env 0 too
    same(info27(env)[:, NO_PRICE], m.info()[:, NO_PRICE], "info")          # cash_flow, total_revenue, profit_margin: see the docstring
    for f in env.INFO_FIELDS:
        assert torch.equal(env.info(f), twin.info(f)), f
    env.close(); twin.close()


def test_compact_rows_are_the_leading_columns(cge):
    n, k = 130, 40
    full, small = (cge.AgriculturalFarmVectorEnv(n, autoreset_mode="SameStep", compact_obs=c) for c in (False, True))
    o1, o2 = full.reset(seed=100)[0], small.reset(seed=100)[0]            # farm_bankrupt's seeds: action 40 ends every episode at day 80 or 81
    assert tuple(o2.shape) == (n, 134)
    same(live(o1), o2, "reset")
    acts = torch.full((85, n), 40, dtype=torch.int32, device="cuda")
    t1, r1, e1, _, _ = full.rollout(k, actions=acts[:k], trajectory=True, per_step=True)
    t2, r2, e2, _, _ = small.rollout(k, actions=acts[:k], trajectory=True, per_step=True)
    assert tuple(t2.shape) == (k, n, 134) and torch.equal(r1, r2) and torch.equal(e1, e2)
    same(live(t1), t2, "trajectory")
    ends = 0
    for t in range(k, 85):
        a, b = full.step(acts[t]), small.step(acts[t])
        same(live(a[0]), b[0], t)
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        tm = a[2].cpu().numpy()
        if tm.any():
            same(live(a[4]["final_obs"], tm), b[4]["final_obs"].cpu().numpy()[tm], (t, "final_obs"))
        ends += int(tm.sum())
    assert ends >= 8
    same(live(full.rollout(3, action_seed=5)[0]), small.rollout(3, action_seed=5)[0], "the last step's rows")
    full.close(); small.close()


def test_two_shards_equal_one_batch(cge):
    k = 370
    whole = cge.AgriculturalFarmVectorEnv(10, autoreset_mode="SameStep")
    whole.reset(seed=77)
    tw, rw, cw, sw, dw = whole.rollout(k, action_seed=9, trajectory=True, per_step=True)
    for first in (0, 5):
        part = cge.AgriculturalFarmVectorEnv(5, autoreset_mode="SameStep", env_index0=first)
        part.reset(seed=77)
        tp, rp, cp, sp, dp = part.rollout(k, action_seed=9, trajectory=True, per_step=True)
        s = slice(first, first + 5)
        assert torch.equal(tp, tw[:, s]) and torch.equal(rp, rw[:, s]) and torch.equal(cp, cw[:, s]) and torch.equal(sp, sw[s]) and torch.equal(dp, dw[s])
        part.close()
    assert int(dw.min()) >= 1
    whole.close()


def test_snapshot_restore_repeats_the_steps(cge):
    n = 130
    env = cge.AgriculturalFarmVectorEnv(n, autoreset_mode="SameStep")
    env.reset(seed=8)
    env.rollout(345, action_seed=4)
    day = env.info("day")
    assert (day > 0).all() and (env.info("water_quality") != 0.9).any()   # mid-episode
    snap = env.snapshot()
    acts = dev(fm.hash_actions(6, 20, n, t0=345))
    first = [env.step(acts[t])[:3] for t in range(20)]
    first = [[x.clone() for x in r] for r in first]
    info = {f: env.info(f) for f in env.INFO_FIELDS}
    assert sum(int(r[2].sum()) for r in first) > 0                        # the year's end and its reset are inside
    env.restore(snap)
    assert torch.equal(env.info("day"), day)
    for t in range(20):
        again = env.step(acts[t])
        assert all(torch.equal(x, y) for x, y in zip(first[t], again[:3])), t
    for f in env.INFO_FIELDS:
        assert torch.equal(env.info(f), info[f]), f
    fresh = cge.AgriculturalFarmVectorEnv(n, autoreset_mode="SameStep")   # and into another handle
    fresh.restore(snap)
    for t in range(20):
        assert all(torch.equal(x, y) for x, y in zip(first[t], fresh.step(acts[t])[:3])), t
    other = cge.AgriculturalFarmVectorEnv(n + 1)
    with pytest.raises(ValueError):
        other.restore(snap)
    env.close(); fresh.close(); other.close()


def test_out_of_range_and_negative_actions(cge):
    kit.out_of_range_and_negative_actions(cge, SPEC)


def test_action_sampler_matches_host_sampling(cge):
    kit.action_sampler_matches_host_sampling(cge, SPEC)


def test_refusals(cge):
    with pytest.raises(cge.NativeLibraryError):
        cge.AgriculturalFarmVectorEnv(8, device="cpu")
    with pytest.raises(ValueError):
        cge.AgriculturalFarmVectorEnv(0)
    with pytest.raises(ValueError):
        cge.AgriculturalFarmVectorEnv(8, info_fields=("no_such_field",))
    for bad in (0, -5, 256):
        with pytest.raises(ValueError, match="max_years"):
            cge.AgriculturalFarmVectorEnv(8, max_years=bad)
    env = cge.AgriculturalFarmVectorEnv(8, info_fields=("day",), max_years=255)
    env.reset(seed=0)
    for shape in ((7,), (8, 1), (2, 8)):
        with pytest.raises(ValueError):
            env.step(torch.zeros(shape, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        env.info("day", 1)                                                # the fields are not indexed
    with pytest.raises(TypeError):
        env.info("field_crop", 1)
    a = torch.zeros(8, dtype=torch.int32, device="cuda")
    odd = torch.zeros(8 * 620 + 1, device="cuda")[1:]                     # 4 bytes off a 16-byte boundary
    buf = torch.zeros(8 * 620, device="cuda")
    assert env._lib.cge_farm_step(env._h, a.data_ptr(), odd.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert b"16-byte aligned" in env._lib.cge_farm_last_error(env._h)
    assert env._lib.cge_farm_step(env._h, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, None) == -1
    assert env._lib.cge_farm_rollout(env._h, 2, None, 0, 0, buf.data_ptr(), 8 * 620 - 4, None, None, None, None, None) == -1
    assert env._lib.cge_farm_info(env._h, 29, buf.data_ptr(), None) == -1
    _, _, _, _, infos = env.step(a)
    assert (infos["day"] == 1).all()
    env.close()
