"""Terminal observations of fused SAME_STEP rollouts (missing #1): every reference step() RETURNS the terminal observation
(snake_env.py:88-94,113-119; crypto_trading_env.py:384-398; environment.py:193-203; parking_env.py:150-159; env.py:105-116;
fleet_env.py:262-276; manufacturing_env.py:293-301; hospital_env.py:362-369).  `step()` delivers it as infos["final_obs"]; a fused
rollout writes the RESET observation to slot t of its trajectory and the terminal rows to the per-segment side output of
cge_<env>_rollout_final_obs.  For all eight env types: rollout(trajectory=True) + that output == k step() calls on a twin (whose
obs / final_obs are pinned against the oracle and the reference fixtures by the per-env test files)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


def _cases(cge):
    ri = lambda hi, shape: torch.randint(0, hi, shape, dtype=torch.int32, device="cuda")
    return {
        # name: (constructor, kwargs with a short time limit, actions(k, n) -> what rollout(actions=...) takes, action of step t)
        "snake": (cge.SnakeVectorEnv, dict(grid_size=10, max_steps=9), lambda k, n: ri(4, (k, n)), lambda a, t: a[t]),
        "snake15": (cge.SnakeVectorEnv, dict(grid_size=15, max_steps=40), lambda k, n: ri(4, (k, n)), lambda a, t: a[t]),
        # obs rows wider than 64 dwords (even G >= 18; 20 is the constructor's default): the terminal-row copy takes several passes
        "snake18": (cge.SnakeVectorEnv, dict(grid_size=18, max_steps=30), lambda k, n: ri(4, (k, n)), lambda a, t: a[t]),
        "snake20": (cge.SnakeVectorEnv, dict(grid_size=20, max_steps=30), lambda k, n: ri(4, (k, n)), lambda a, t: a[t]),
        "snake30": (cge.SnakeVectorEnv, dict(grid_size=30, max_steps=30), lambda k, n: ri(4, (k, n)), lambda a, t: a[t]),
        "crypto": (cge.CryptoVectorEnv, dict(action_type="discrete", max_steps=13), lambda k, n: ri(5, (k, n)), lambda a, t: a[t]),
        "traffic": (cge.TrafficVectorEnv, dict(max_steps=21), lambda k, n: ri(3, (k, n, 9)), lambda a, t: a[t]),
        "parking": (cge.ParkingVectorEnv, dict(max_steps=23), lambda k, n: ri(8, (k, n)), lambda a, t: a[t]),
        "climate": (cge.ClimateVectorEnv, dict(episode_minutes=17),
                    lambda k, n: (torch.rand((k, n), device="cuda") * 16 + 16, torch.randint(0, 2, (k, n, 4), dtype=torch.int8, device="cuda")),
                    lambda a, t: (a[0][t], a[1][t])),
        "fleet": (cge.FleetVectorEnv, dict(max_timesteps=29), lambda k, n: ri(8, (k, n, 3)), lambda a, t: a[t]),
        "manufacturing": (cge.ManufacturingVectorEnv, dict(max_steps=31), lambda k, n: ri(25, (k, n)), lambda a, t: a[t]),
        "hospital": (cge.HospitalVectorEnv, dict(max_episode_length=19), lambda k, n: ri(35, (k, n)), lambda a, t: a[t]),
    }


@pytest.mark.parametrize("name", ["snake", "snake15", "snake18", "snake20", "snake30", "crypto", "traffic", "parking", "climate", "fleet", "manufacturing", "hospital"])
def test_rollout_plus_final_rows_equals_k_step_calls(cge, name):
    Env, kw, make, at = _cases(cge)[name]
    n, k = 64 * 5 + 37, 70                                     # a ragged last segment; every env ends several episodes
    env = Env(n, autoreset_mode="SameStep", env_index0=3, **kw)
    twin = Env(n, autoreset_mode="SameStep", env_index0=3, **kw)
    env.reset(seed=5); twin.reset(seed=5)
    env.collect_final_obs(rows_per_env=k)                      # room for an episode end at every step
    acts = make(k, n)
    traj, rt, ft, rs, dc = env.rollout(k, actions=acts, trajectory=True, per_step=True)
    rows, step, who = env.final_obs()
    assert env.final_obs_dropped() == 0
    j = 0
    for t in range(k):
        ob, r, te, tr, info = twin.step(at(acts, t))
        done = te | tr
        assert torch.equal(ob, traj[t]), (name, t)
        assert torch.equal(done, ft[t] != 0), (name, t)
        d = torch.nonzero(done).flatten()
        m = d.numel()
        if m:
            assert torch.equal(step[j:j + m], torch.full((m,), t, device="cuda")) and torch.equal(who[j:j + m], d), (name, t)
            assert torch.equal(rows[j:j + m], info["final_obs"][d]), (name, t)
            j += m
    assert j == rows.shape[0] and j >= n, name                 # every env finished at least once
    # a second call reports ITS rows only; a segment that is too small drops the surplus and says so
    env.collect_final_obs(rows_per_env=1)
    traj, rt, ft, rs, dc = env.rollout(k, actions=acts, trajectory=True, per_step=True)
    rows, step, who = env.final_obs()
    total = int((ft != 0).sum())
    assert rows.shape[0] + env.final_obs_dropped() == total and env.final_obs_dropped() > 0
    # other autoreset modes deliver nothing (slot t of their trajectory is the terminal observation)
    nx = Env(n, autoreset_mode="NextStep", **kw)
    nx.reset(seed=5)
    nx.collect_final_obs(rows_per_env=4)
    nx.rollout(k, actions=acts, trajectory=True, per_step=True)
    assert nx.final_obs()[0].shape[0] == 0
    env.collect_final_obs(rows_per_env=0)
    for e in (env, twin, nx):
        e.close()


@pytest.mark.parametrize("name", ["snake", "crypto", "traffic", "parking", "climate", "fleet", "manufacturing", "hospital"])
def test_reading_rows_without_the_output_registered_is_a_clear_error(cge, name):
    """final_obs() / final_obs_dropped() before collect_final_obs(), and after collect_final_obs(0) turned the output off again."""
    Env, kw, make, at = _cases(cge)[name]
    n, k = 70, 5
    env = Env(n, autoreset_mode="SameStep", **kw)
    env.reset(seed=1)
    for read in (env.final_obs, env.final_obs_dropped):
        with pytest.raises(RuntimeError, match="collect_final_obs"):
            read()
    env.collect_final_obs(rows_per_env=2)
    env.rollout(k, actions=make(k, n))
    assert env.final_obs()[0].shape[0] + env.final_obs_dropped() >= 0
    env.collect_final_obs(rows_per_env=0)
    env.rollout(k, actions=make(k, n))
    for read in (env.final_obs, env.final_obs_dropped):
        with pytest.raises(RuntimeError, match="collect_final_obs"):
            read()
    env.close()
