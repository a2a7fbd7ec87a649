"""Terminal rows of fused SAME_STEP rollouts against the ORACLE, at every kernel instance that writes them.

`rollout()` with `collect_final_obs()` delivers the terminal observation of every SAME_STEP episode end through a per-segment side
output (include/cge_amd.h).  Each kernel writes it through its own code paths: explicit or hash actions, a trajectory, the last
observation or none (snake: terminal rows copied from the LDS obs rows, or built by each finishing lane; odd grids by bytes).  Here
the expected rows come from the oracle stepped in SAME_STEP with `want_final=True`: the delivered (step, env) pairs must be exactly
the pairs where terminated | truncated, and each row must equal the oracle's bit for bit (crypto: test_edges_gpu's stated fp32
tolerance, at most one diverged env).  The side-output buffer is filled with a sentinel before every rollout, so an unwritten dword
cannot pass by being zero.  Hash-action rollouts are checked with the actions tests/_hash_actions.py rebuilds (pinned against the
oracle's own hash rollouts by test_oracle_hash_rollout.py)."""
import numpy as np
import pytest
import torch

from _action_streams import RUNS, HASH_ROLLOUTS, final_obs_actions as _random_actions
from _hash_actions import at, hash_actions
from test_edges_gpu import _rows_ok
from test_oracle_hash_rollout import make_oracle

pytestmark = pytest.mark.gpu

ENV0, SEED, A_SEED, T0 = RUNS["final_obs"]["env0"], RUNS["final_obs"]["seed"], HASH_ROLLOUTS["final_obs"]["a_seed"], HASH_ROLLOUTS["final_obs"]["t0"]
VIEWS = ["trajectory", "last_obs", "no_obs"]

# id: (env type, VectorEnv class, device kwargs, oracle class, oracle kwargs; the same short time limit on both sides, helper kwargs)
CASES = {
    "snake10": ("snake", "SnakeVectorEnv", dict(grid_size=10, max_steps=9), "SnakeOracle", dict(grid=10, max_steps=9), {}),
    "crypto": ("crypto", "CryptoVectorEnv", dict(action_type="discrete", max_steps=13), "CryptoOracle", dict(action_type="discrete", max_steps=13), {}),
    "crypto_continuous": ("crypto", "CryptoVectorEnv", dict(action_type="continuous", max_steps=13), "CryptoOracle",
                          dict(action_type="continuous", max_steps=13), dict(continuous=True)),
    "crypto_config": ("crypto", "CryptoVectorEnv", dict(action_type="discrete", max_steps=13, config="golden"), "CryptoOracle",
                      dict(action_type="discrete", max_steps=13, config="golden"), {}),
    "traffic3x3_4": ("traffic", "TrafficVectorEnv", dict(max_steps=11, grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4),
                     "TrafficOracle", dict(max_steps=11, grid_size=(3, 3), num_intersections=4, max_vehicles=20, spawn_rate=0.4), dict(ni=4)),
    "traffic9": ("traffic", "TrafficVectorEnv", dict(max_steps=11), "TrafficOracle", dict(max_steps=11), dict(ni=9)),
    "traffic4x4_16": ("traffic", "TrafficVectorEnv", dict(max_steps=11, grid_size=(4, 4), num_intersections=16), "TrafficOracle",
                      dict(max_steps=11, grid_size=(4, 4), num_intersections=16), dict(ni=16)),
    "traffic4x5_13": ("traffic", "TrafficVectorEnv", dict(max_steps=11, grid_size=(4, 5), num_intersections=13, max_vehicles=60, spawn_rate=0.5),
                      "TrafficOracle", dict(max_steps=11, grid_size=(4, 5), num_intersections=13, max_vehicles=60, spawn_rate=0.5), dict(ni=13)),
    "parking": ("parking", "ParkingVectorEnv", dict(max_steps=17), "ParkingOracle", dict(max_steps=17), {}),
    "climate": ("climate", "ClimateVectorEnv", dict(episode_minutes=9), "ClimateOracle", dict(max_steps=9), {}),
    "climate_occ1": ("climate", "ClimateVectorEnv", dict(episode_minutes=9, max_occupancy=1), "ClimateOracle", dict(max_steps=9, max_occupancy=1), {}),
    "climate_occ15": ("climate", "ClimateVectorEnv", dict(episode_minutes=9, max_occupancy=15), "ClimateOracle", dict(max_steps=9, max_occupancy=15), {}),
    "fleet": ("fleet", "FleetVectorEnv", dict(max_timesteps=15), "FleetOracle", dict(max_steps=15), {}),
    "manufacturing": ("manufacturing", "ManufacturingVectorEnv", dict(max_steps=19), "ManufacturingOracle", dict(max_steps=19), {}),
    "hospital": ("hospital", "HospitalVectorEnv", dict(max_episode_length=12), "HospitalOracle", dict(max_steps=12), {}),
}
NACT = {"snake": 4, "crypto": 5, "traffic": 3, "parking": 8, "fleet": 8, "manufacturing": 25, "hospital": 35}


def _snake_case(grid, max_steps=15):
    # grid=None: the constructor's default grid (grid_size not passed); the oracle needs the number
    dkw = dict(max_steps=max_steps) if grid is None else dict(grid_size=grid, max_steps=max_steps)
    return ("snake", "SnakeVectorEnv", dkw, "SnakeOracle", dict(grid=20 if grid is None else grid, max_steps=max_steps), {})   # snake.py: 20


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


def _device_kwargs(dkw):
    if dkw.get("config") == "golden":
        from test_oracle_hash_rollout import crypto_config
        return dict(dkw, config=crypto_config())
    return dkw


def _dev(a):
    return tuple(torch.from_numpy(x).cuda() for x in a) if isinstance(a, tuple) else torch.from_numpy(a).cuda()


class Setup:
    """A SAME_STEP device batch and its oracle twin on the same seeds: n = 3 segments + a ragged remainder, env_index0 = 3."""

    def __init__(self, cge, oracle, case, n=None, seg_extra=37):
        self.name, cls, dkw, ocls, okw, self.hkw = case
        self.Env, self.dkw = getattr(cge, cls), _device_kwargs(dkw)
        probe = self.Env(1, autoreset_mode="SameStep", **self.dkw)
        self.seg = int(probe._fn("final_obs_segment")(probe._h))
        probe.close()
        self.n = n if n is not None else 3 * self.seg + seg_extra % self.seg
        assert self.n % self.seg != 0 or n is not None
        self.env = self.Env(self.n, autoreset_mode="SameStep", env_index0=ENV0, **self.dkw)
        self.o = make_oracle(oracle, ocls, okw, self.n, oracle.SAME_STEP)
        self.o.seed(np.arange(self.n, dtype=np.uint64) + np.uint64(ENV0 + SEED))
        self.env.reset(seed=SEED)
        self.o.reset()
        self.crypto = self.name == "crypto"

    def poison(self):
        rows, index = self.env._fin[0], self.env._fin[1]
        if rows.dtype == torch.int8:
            rows.fill_(0x7F)                                   # snake obs are 0 / 1 / 2
        else:
            rows.view(torch.int32).fill_(0x7FBADBAD)            # a NaN: no oracle row holds it, and it compares unequal bit for bit
        index.fill_(-1)

    def rollout(self, k, actions, view, per_step=False):
        """actions: numpy explicit actions, or None for the hash source (action_seed=A_SEED, t0=T0)."""
        kw = dict(trajectory=view == "trajectory", want_obs=view != "no_obs", per_step=per_step)
        if actions is None:
            return self.env.rollout(k, action_seed=A_SEED, t0=T0, **kw)
        return self.env.rollout(k, actions=_dev(actions), **kw)

    def step_oracle(self, acts, k, keep_obs):
        """k oracle steps with want_final: per-step (obs or None, reward, flags); the terminal pairs (step, env) in (step, env) order
        and their rows; reward sums as the rollout accumulates them; done counts."""
        obs, rew, flags, steps, envs, rows = [], [], [], [], [], []
        rs = np.zeros(self.n, np.float32 if self.name == "snake" else np.float64)
        dc = np.zeros(self.n, np.int32)
        for t in range(k):
            a = at(acts, t)
            oo, ro, te, tr, fin = self.o.step(*a, want_final=True) if isinstance(a, tuple) else self.o.step(a, want_final=True)
            done = (te | tr).astype(bool)
            d = np.nonzero(done)[0]
            steps.append(np.full(d.size, t, np.int64)); envs.append(d.astype(np.int64)); rows.append(fin[d])
            obs.append(oo if keep_obs or t == k - 1 else None)
            rew.append(ro); flags.append(te.astype(np.uint8) | (tr.astype(np.uint8) << 1))
            rs += ro if self.name == "snake" else self.o.last_reward64
            dc += done
        return dict(obs=obs, rew=rew, flags=flags, step=np.concatenate(steps), env=np.concatenate(envs), rows=np.concatenate(rows), rs=rs, dc=dc)

    def close(self):
        self.env.close()


def _check_rows(name, dev_rows, ref_rows):
    """per-row ok flags (bit-exact; crypto: the stated tolerance)"""
    return _rows_ok("Crypto" if name == "crypto" else name, dev_rows, ref_rows)


def _assert_delivered(s, exp, what):
    """The delivered side output equals the oracle's terminal pairs as a set, and every row equals the oracle's row."""
    rows, step, who = (x.cpu().numpy() for x in s.env.final_obs())
    assert s.env.final_obs_dropped() == 0, what
    key_d, key_e = step * s.n + who, exp["step"] * s.n + exp["env"]
    assert np.unique(key_d).size == key_d.size, (what, "a (step, env) pair delivered twice")
    assert np.bincount(exp["env"], minlength=s.n).min() >= 2, (what, "every env ends several episodes")
    bad_envs = set()
    if not np.array_equal(key_d, key_e):
        missing, extra = np.setdiff1d(key_e, key_d), np.setdiff1d(key_d, key_e)
        bad_envs |= set((missing % s.n).tolist()) | set((extra % s.n).tolist())
        assert s.crypto, (what, "pairs missing", [(int(x // s.n), int(x % s.n)) for x in missing[:5]],
                          "unexpected", [(int(x // s.n), int(x % s.n)) for x in extra[:5]], len(missing), len(extra))
    common, i_d, i_e = np.intersect1d(key_d, key_e, return_indices=True)
    ok = _check_rows(s.name, rows[i_d], exp["rows"][i_e])
    if not ok.all():
        bad = common[~ok]
        bad_envs |= set((bad % s.n).tolist())
        first = i_d[np.argmax(~ok)]
        diff = np.nonzero(rows[first].reshape(-1).view(np.uint8) != exp["rows"][i_e[np.argmax(~ok)]].reshape(-1).view(np.uint8))[0]
        assert s.crypto, (what, f"{int((~ok).sum())} of {ok.size} rows differ; first (step, env) = {(int(step[first]), int(who[first]))}, "
                                f"differing bytes {diff[:4]}..{diff[-4:]} of {rows[first].nbytes}")
    assert len(bad_envs) <= (1 if s.crypto else 0), (what, sorted(bad_envs)[:5])
    return bad_envs


def _assert_outputs(s, exp, out, view, per_step, bad_envs, what):
    """The rollout's own outputs against the same oracle steps: trajectory / last obs, per-step reward and flags, sums, counts.
    Crypto: the envs outside the tolerance anywhere, those of the side output included, are at most one."""
    if per_step:
        obs, rt, ft, rs, dc = out
        rt, ft = rt.cpu().numpy(), ft.cpu().numpy()
    else:
        obs, rs, dc = out
    bad = set(bad_envs)

    def expect(ok, *where):
        if s.crypto:
            bad.update(np.nonzero(~ok)[0].tolist())
        else:
            assert ok.all(), (what,) + where + (np.argwhere(~ok)[:5],)

    k = len(exp["rew"])
    if view == "trajectory":
        traj = obs.cpu().numpy()
        for t in range(k):
            expect(_check_rows(s.name, traj[t], exp["obs"][t]), "trajectory", t)
    elif view == "last_obs":
        expect(_check_rows(s.name, obs.cpu().numpy(), exp["obs"][-1]), "last obs")
    else:
        assert obs is None
    if per_step:
        for t in range(k):
            expect(ft[t].astype(np.uint8) == exp["flags"][t], "flags", t)     # bool flags (terminated only) or terminated | truncated << 1
            if s.crypto:
                expect(np.isclose(rt[t], exp["rew"][t], rtol=1e-6, atol=1e-3), "reward", t)
            else:
                expect(rt[t] == exp["rew"][t], "reward", t)
    rs, dc = rs.cpu().numpy(), dc.cpu().numpy()
    expect(dc == exp["dc"], "done counts")
    if s.crypto:
        expect(np.isclose(rs, exp["rs"], rtol=1e-7, atol=1e-3), "reward sums")
        print(f"crypto {what}: {len(bad)}/{s.n} envs outside the tolerance")
        assert len(bad) <= 1, (what, sorted(bad)[:5])
    else:
        assert rs.dtype == exp["rs"].dtype, what
        expect(rs == exp["rs"], "reward sums")


def _run(s, actions, view, k, rows_per_env=None, per_step=None):
    """One poisoned rollout with the side output on; returns the oracle's steps and the rollout's outputs."""
    per_step = view == "trajectory" if per_step is None else per_step
    s.env.collect_final_obs(rows_per_env=k if rows_per_env is None else rows_per_env)
    s.poison()
    acts = actions if actions is not None else hash_actions(s.name, A_SEED, k, s.n, t0=T0, env0=ENV0, **s.hkw)
    out = s.rollout(k, actions, view, per_step=per_step)
    exp = s.step_oracle(acts, k, keep_obs=view == "trajectory")
    return exp, out


def _matrix(cge, oracle, case, actions, view, k=RUNS["final_obs"]["k"]):
    s = Setup(cge, oracle, case)
    what = (s.name, s.dkw, actions, view)
    acts = _random_actions(s.name, s.hkw, k, s.n, np.random.default_rng(k)) if actions == "explicit" else None
    exp, out = _run(s, acts, view, k)
    bad = _assert_delivered(s, exp, what)
    _assert_outputs(s, exp, out, view, view == "trajectory", bad, what)
    s.close()


# ---------------------------------------------------------------------------------------------------------------- snake, every grid
# (actions, view): explicit actions with a trajectory; hash actions with the last obs (both: terminal rows copied from the LDS obs rows
# on even grids); hash actions without obs (every finishing lane writes its own row).  The grids' classes: odd G (byte rows, not
# PACKED), even G with OBS_DW < 64, G = 16 (OBS_DW == 64), even G >= 18 (OBS_DW > 64), G >= 13 (64-thread workgroups); None = the
# constructor's default grid, grid_size not passed.
SNAKE_VARIANTS = [("explicit", "trajectory"), ("hash", "last_obs"), ("hash", "no_obs")]


@pytest.mark.parametrize("actions,view", SNAKE_VARIANTS, ids=lambda v: v)
@pytest.mark.parametrize("grid", list(range(4, 31)) + [None], ids=lambda g: f"G{g}" if g else "Gdefault")
def test_snake_terminal_rows_every_grid(cge, oracle, grid, actions, view):
    _matrix(cge, oracle, _snake_case(grid), actions, view)


@pytest.mark.parametrize("actions,view", SNAKE_VARIANTS, ids=lambda v: v)
@pytest.mark.parametrize("grid", [4, 5, 6, 8])
def test_snake_every_kind_of_episode_end(cge, oracle, grid, actions, view):
    """A small max_steps on a big batch: crashes (reward < 0), time limits without eating (reward 0) and time limits on a step that ate
    (reward > 0: the deferred path, which shares its wave with the LDS-row copy) all occur, and all are delivered."""
    k = 40
    s = Setup(cge, oracle, _snake_case(grid, max_steps=6), n=2048 + 29)
    acts = _random_actions("snake", {}, k, s.n, np.random.default_rng(grid)) if actions == "explicit" else None
    exp, out = _run(s, acts, view, k, per_step=True)
    what = ("snake", grid, actions, view)
    _assert_delivered(s, exp, what)
    _assert_outputs(s, exp, out, view, True, set(), what)
    _, rt, ft = out[0], out[1].cpu().numpy(), out[2].cpu().numpy()
    r = rt[exp["step"], exp["env"]]
    assert ft[exp["step"], exp["env"]].all()
    kinds = {"crash": int((r < 0).sum()), "time limit": int((r == 0).sum()), "time limit on a step that ate": int((r > 0).sum())}
    assert min(kinds.values()) > 0, (what, kinds)
    s.close()


# ---------------------------------------------------------------------------------------------------------------- all eight env types
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("actions", ["explicit", "hash"])
@pytest.mark.parametrize("case", list(CASES))
def test_terminal_rows_every_env_type(cge, oracle, case, actions, view):
    _matrix(cge, oracle, CASES[case], actions, view)


@pytest.mark.parametrize("case", ["snake10", "snake20", "crypto", "traffic9", "traffic4x5_13", "parking", "climate", "fleet", "manufacturing", "hospital"])
def test_segment_capacity_overflow(cge, oracle, case):
    """rows_per_env=1 over a long run: every segment stores min(capacity, its terminal rows), final_obs_dropped() counts the rest,
    no (step, env) pair appears twice, and every stored row is the oracle's row for its pair (which rows a full segment keeps is not
    asserted: fleet takes its slots by atomicAdd)."""
    c = _snake_case(20, max_steps=15) if case == "snake20" else CASES[case]
    s = Setup(cge, oracle, c)
    k = 100
    exp, _ = _run(s, None, "last_obs", k, rows_per_env=1)
    rows, step, who = (x.cpu().numpy() for x in s.env.final_obs())
    cap = s.seg
    seg_d = np.bincount(who // s.seg, minlength=-(-s.n // s.seg))
    seg_e = np.bincount(exp["env"] // s.seg, minlength=-(-s.n // s.seg))
    key_d = step * s.n + who
    assert np.unique(key_d).size == key_d.size, (case, "a (step, env) pair delivered twice")
    if s.crypto:                                               # a diverged env may move one row between steps; counts as in test_edges
        assert np.abs(seg_d - np.minimum(cap, seg_e)).max() <= 1, (case, seg_d, seg_e)
    else:
        assert np.array_equal(seg_d, np.minimum(cap, seg_e)), (case, seg_d, seg_e, cap)
        assert s.env.final_obs_dropped() == int(np.maximum(0, seg_e - cap).sum()), case
    assert (seg_e > cap).all(), (case, "every segment overflows", seg_e, cap)
    key_e = exp["step"] * s.n + exp["env"]
    idx = np.searchsorted(key_e, key_d)
    found = (idx < key_e.size) & (key_e[np.minimum(idx, key_e.size - 1)] == key_d)
    ok = np.zeros(key_d.size, bool)
    ok[found] = _check_rows(s.name, rows[found], exp["rows"][idx[found]])
    bad_envs = set(who[~ok].tolist())
    assert len(bad_envs) <= (1 if s.crypto else 0), (case, int((~ok).sum()), "of", ok.size, "stored rows are not the oracle's", sorted(bad_envs)[:5])
    s.close()
