"""Directed scenarios against the oracle: the dynamics branches that random actions never reach.

tests/test_oracle_branch_coverage.py measures which branches of the oracles the other GPU tests' action streams enter; the ones they
miss (terminations other than the time limit, observation caps, out-of-box actions, ...) are driven here by the policies of
tests/_directed_scenarios.py.  Per scenario, with 65 envs (one full wave plus one lane) at env_index0 = 3, in SameStep and NextStep:

1. the policy runs closed-loop on the oracle and the scenario's event must have happened in at least one env, judged on the
   oracle's own outputs;
2. the device is stepped with the same actions: observation bits, reward, terminated and truncated equal the oracle's at every step
   (SameStep: the terminal rows too), and the info fields at the end (crypto: test_edges_gpu's stated tolerance, at most one env
   outside it);
3. the actions are replayed through rollout(k, actions=..., trajectory=True, per_step=True) on a fresh batch, with the terminal-row
   side output in SameStep: trajectory, per-step rewards and flags, reward sums, done counts and the delivered terminal rows equal
   the same oracle run (the fused rollout kernels are separate template instances from step())."""
import numpy as np
import pytest
import torch

import _action_streams as S
import _directed_scenarios as D
from test_edges_gpu import _rows_ok

pytestmark = pytest.mark.gpu

MODES = ["SameStep", "NextStep"]
_runs = {}


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


def _oracle_run(oracle, scn, mode):
    """one oracle run per (scenario, mode), shared by the step and the rollout test and left unchanged"""
    key = (scn.name, mode)
    if key not in _runs:
        _runs[key] = D.run_oracle(oracle, scn, S.MODES[mode])
    return _runs[key]


def _dev(a):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a) if isinstance(a, tuple) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stack(acts):
    if isinstance(acts[0], tuple):
        return tuple(np.stack([a[j] for a in acts]) for j in range(len(acts[0])))
    return np.stack(acts)


def _np(t):
    return t.cpu().numpy()


class Tally:
    """Bit-exact for every type but crypto, where the envs outside test_edges_gpu's stated tolerance anywhere in the run are counted
    and at most one is allowed."""

    def __init__(self, scn, n):
        self.crypto, self.name, self.bad, self.what = scn.env == "crypto", scn.env.capitalize(), np.zeros(n, bool), scn.name

    def rows(self, dev, ref, *where, sel=None):
        self.flag(_rows_ok(self.name, dev, ref), *where, sel=sel)

    def reward(self, dev, ref, *where):
        self.flag(np.isclose(dev, ref, rtol=1e-6, atol=1e-3) if self.crypto else dev == ref, *where)

    def flag(self, ok, *where, sel=None):
        if not self.crypto:
            assert ok.all(), (self.what,) + where + (np.argwhere(~ok)[:5],)
        elif sel is None:
            self.bad |= ~ok
        else:
            self.bad[sel[~ok]] = True

    def close(self):
        if self.crypto:
            print(f"{self.what}: {int(self.bad.sum())}/{self.bad.size} envs outside the crypto tolerance")
            assert int(self.bad.sum()) <= 1, (self.what, np.nonzero(self.bad)[0][:5])


def _make(cge, scn, mode):
    env = getattr(cge, S.ENV_TYPES[scn.env][1])(D.N_ENVS, autoreset_mode=mode, env_index0=D.ENV0, **scn.device_kwargs())
    obs, _ = env.reset(seed=scn.seed)
    return env, obs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scn", D.SCENARIOS, ids=lambda s: s.name)
def test_step_matches_oracle_through_the_event(cge, oracle, scn, mode):
    run = _oracle_run(oracle, scn, mode)
    assert run["hit"].any(), f"{scn.name}: '{scn.event}' happened in no env of the oracle run"
    n, same, tally = D.N_ENVS, mode == "SameStep", Tally(scn, D.N_ENVS)
    env, od = _make(cge, scn, mode)
    tally.rows(_np(od), run["obs0"], "reset")
    for t in range(scn.T):
        od, rd, ted, trd, info = env.step(_dev(run["actions"][t]))
        te, tr = run["te"][t].astype(bool), run["tr"][t].astype(bool)
        tally.rows(_np(od), run["obs"][t], "obs", t)
        tally.reward(_np(rd), run["rew"][t], "reward", t)
        tally.flag(_np(ted) == te, "terminated", t)
        tally.flag(_np(trd) == tr, "truncated", t)
        if same:
            done = te | tr
            tally.flag(_np(info["_final_obs"]) == done, "_final_obs", t)
            idx = np.nonzero(done)[0]
            tally.rows(_np(info["final_obs"])[idx], run["fin"][t][idx], "final_obs", t, sel=idx)
    o = run["oracle"]
    for f in D.INFO[scn.env]:
        d, r = _np(env.info(f)).astype(np.float64), np.asarray(D.oracle_info(o, scn.env, f), np.float64)
        loose, rtol, atol = D.INFO_TOL.get(scn.env, ((), 0, 0))
        tally.flag(np.isclose(d, r, rtol=rtol, atol=atol) if f in loose else d == r, "info", f)
    tally.close()
    env.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scn", D.SCENARIOS, ids=lambda s: s.name)
def test_fused_rollout_matches_oracle_through_the_event(cge, oracle, scn, mode):
    run = _oracle_run(oracle, scn, mode)
    assert run["hit"].any(), f"{scn.name}: '{scn.event}' happened in no env of the oracle run"
    n, k, same, tally = D.N_ENVS, scn.T, mode == "SameStep", Tally(scn, D.N_ENVS)
    env, _ = _make(cge, scn, mode)
    if same:
        env.collect_final_obs(rows_per_env=k)
    traj, rt, ft, rs, dc = env.rollout(k, actions=_dev(_stack(run["actions"])), trajectory=True, per_step=True)
    traj, rt, ft = _np(traj), _np(rt), _np(ft)
    sums, counts = np.zeros(n, np.float32 if scn.env == "snake" else np.float64), np.zeros(n, np.int32)   # snake: float32 sums in step order
    for t in range(k):
        te, tr = run["te"][t].astype(np.uint8), run["tr"][t].astype(np.uint8)
        tally.rows(traj[t], run["obs"][t], "trajectory", t)
        tally.reward(rt[t], run["rew"][t], "reward", t)
        tally.flag(ft[t].astype(np.uint8) == ((te | tr) if ft.dtype == np.bool_ else (te | (tr << 1))), "flags", t)   # bool: types that never truncate
        sums += run["rew64"][t]
        counts += (te | tr)
    tally.flag(_np(dc) == counts, "done counts")
    assert _np(rs).dtype == sums.dtype, scn.name
    tally.flag(np.isclose(_np(rs), sums, rtol=1e-7, atol=1e-3) if tally.crypto else _np(rs) == sums, "reward sums")
    if same:
        rows, step, who = (_np(x) for x in env.final_obs())
        assert env.final_obs_dropped() == 0
        exp = [(t, i) for t in range(k) for i in np.nonzero(run["te"][t] | run["tr"][t])[0]]
        got = list(zip(step.tolist(), who.tolist()))
        if tally.crypto:
            tally.bad[[i for _, i in set(exp) ^ set(got)]] = True
        else:
            assert got == exp, (scn.name, "delivered (step, env) pairs", len(got), len(exp))
        at = {p: j for j, p in enumerate(got)}
        both = [p for p in exp if p in at]
        assert both, (scn.name, "no terminal row to compare")
        ref = np.stack([run["fin"][t][i] for t, i in both])
        tally.rows(rows[[at[p] for p in both]], ref, "terminal rows", sel=np.array([i for _, i in both]))
    tally.close()
    env.close()
