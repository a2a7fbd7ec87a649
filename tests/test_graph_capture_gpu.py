"""step() and the fused rollout() are capturable in a HIP graph: with
`reuse_buffers=True` every launch goes to the capturing stream and nothing allocates, synchronises or touches the host in between.

step(): 32 calls are captured into one torch.cuda.CUDAGraph, replayed four times, and every step's outputs are compared with the CPU
oracle stepping the same actions, for every oracle-backed env type in both autoreset modes, with time limits short enough that
episodes end (and the in-kernel reset hand-over runs) inside the graph.  A replay repeats the captured kernel ARGUMENTS, so whatever a
kernel needs to know about the calls before it has to live on the device: after the replays one more eager step() and, for the types
with canonical records, a get_state() -> set_state() round trip into a fresh env followed by 60 eager steps check that the host's
view of the handle still agrees with the device's.

rollout(): four calls of rollout(7, trajectory=True, per_step=True) on hash actions in one graph, replayed three times, against the
oracle (bus and world builder: against an eager twin).  Fleet's rollout() is left out: it drives a side stream with events, which a
capture turns into a graph with parallel branches.

Small batches are host-bound per call (climate: kernel 9 us, ~19 us per eager call); a replay queues the launches at once."""
import numpy as np
import pytest
import torch

import _hash_actions
from test_edges_gpu import _rows_ok

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


def _np(t):
    return t.cpu().numpy()


# Steps per captured graph.  It must stay a number that is NOT 0 mod 50: crypto's 50-candle window is a ring, and only then does
# every replay start at another ring phase than the capture did (four replays of 32: phases 0, 32, 14, 46 relative to it).
K = 32
REPLAYS = 4
assert K % 50 != 0


def _cases(cge, oracle):
    """name -> (env(n, mode), oracle(n, code), actions [K, n, ...] on the device, device actions of a step, oracle arguments of a step,
    the name test_edges_gpu._rows_ok compares observation rows under).  The time limits are test_edges_gpu.SHORT's."""
    def ints(hi, *shape):
        return lambda n: torch.randint(0, hi, (K, n) + shape, dtype=torch.int32, device="cuda")

    def plain(a):
        return (_np(a),)
    return {
        "snake": (lambda n, mode: cge.SnakeVectorEnv(n, grid_size=10, autoreset_mode=mode, reuse_buffers=True), lambda n, code: oracle.SnakeOracle(n, 10, code),
                  ints(4), lambda a: a, plain, "Snake"),
        "parking": (lambda n, mode: cge.ParkingVectorEnv(n, autoreset_mode=mode, max_steps=17, reuse_buffers=True),
                    lambda n, code: oracle.ParkingOracle(n, code, max_steps=17), ints(8), lambda a: a, plain, "Parking"),
        "climate": (lambda n, mode: cge.ClimateVectorEnv(n, autoreset_mode=mode, episode_minutes=9, reuse_buffers=True),
                    lambda n, code: oracle.ClimateOracle(n, code, max_steps=9),
                    lambda n: torch.cat([torch.rand((K, n, 1), device="cuda") * 16 + 16, torch.randint(0, 2, (K, n, 4), device="cuda").float()], 2),
                    lambda a: (a[:, 0].contiguous(), a[:, 1:].to(torch.int8)), lambda a: (_np(a[:, :1]).astype(np.float32), _np(a[:, 1:]).astype(np.int8)), "Climate"),
        "fleet": (lambda n, mode: cge.FleetVectorEnv(n, autoreset_mode=mode, max_timesteps=40, reuse_buffers=True),
                  lambda n, code: oracle.FleetOracle(n, code, max_steps=40), ints(8, 3), lambda a: a, plain, "Fleet"),
        "traffic": (lambda n, mode: cge.TrafficVectorEnv(n, autoreset_mode=mode, max_steps=45, reuse_buffers=True),
                    lambda n, code: oracle.TrafficOracle(n, code, max_steps=45), ints(3, 9), lambda a: a, plain, "Traffic"),
        "crypto": (lambda n, mode: cge.CryptoVectorEnv(n, action_type="discrete", autoreset_mode=mode, max_steps=13, reuse_buffers=True),
                   lambda n, code: oracle.CryptoOracle(n, "discrete", code, max_steps=13), ints(5), lambda a: a, plain, "Crypto"),
        "crypto_continuous": (lambda n, mode: cge.CryptoVectorEnv(n, action_type="continuous", autoreset_mode=mode, max_steps=13, reuse_buffers=True),
                              lambda n, code: oracle.CryptoOracle(n, "continuous", code, max_steps=13),
                              lambda n: torch.rand((K, n, 2), device="cuda") * 1.999 - 0.9995, lambda a: a, plain, "Crypto"),
        "hospital": (lambda n, mode: cge.HospitalVectorEnv(n, autoreset_mode=mode, max_episode_length=12, reuse_buffers=True),
                     lambda n, code: oracle.HospitalOracle(n, code, max_steps=12), ints(35), lambda a: a, plain, "Hospital"),
        "manufacturing": (lambda n, mode: cge.ManufacturingVectorEnv(n, autoreset_mode=mode, max_steps=19, reuse_buffers=True),
                          lambda n, code: oracle.ManufacturingOracle(n, code, max_steps=19), ints(25), lambda a: a, plain, "Manufacturing"),
    }


class _Against:
    """One test's comparison with the oracle.  Bit-exact, except: climate against the C oracle (libm's last place,
    tests/test_climate_gpu.py) as before, and crypto within the project's stated tolerance (tests/test_edges_gpu.py) — observation rows
    through _rows_ok("Crypto", ...), rewards rtol 1e-6 / atol 1e-3 as in test_final_obs_oracle_gpu, flags exact for every env inside
    the tolerance, and at most ONE env outside it over the whole test (an env that left the CPU's float64 trajectory stays out)."""

    def __init__(self, name, rows_name, n):
        self.name, self.rows_name, self.out = name, rows_name, np.zeros(n, bool)

    def step(self, dev, ref, what):
        """dev / ref: (obs, reward, terminated, truncated) of one step as numpy arrays."""
        (od, rd, ted, trd), (oo, ro, teo, tro) = dev, ref
        teo, tro = teo.astype(bool), tro.astype(bool)
        if self.rows_name == "Crypto":
            self.out |= ~_rows_ok("Crypto", od, oo)
            assert int(self.out.sum()) <= 1, (self.name, what, "obs", np.argwhere(self.out)[:5].ravel())
            ok = ~self.out
            assert np.allclose(rd[ok], ro[ok], rtol=1e-6, atol=1e-3), (self.name, what, "reward")
            assert np.array_equal(ted[ok], teo[ok]) and np.array_equal(trd[ok], tro[ok]), (self.name, what, "flags")
            return
        if self.rows_name == "Climate":
            assert np.allclose(od.astype(np.float64), oo.astype(np.float64), rtol=1e-6, atol=1e-4), (self.name, what, "obs")
            assert np.allclose(rd.astype(np.float64), ro.astype(np.float64), rtol=1e-6, atol=1e-4), (self.name, what, "reward")
        else:
            assert _rows_ok(self.rows_name, od, oo).all(), (self.name, what, "obs")
            assert np.array_equal(rd, ro), (self.name, what, "reward")
        assert np.array_equal(ted, teo) and np.array_equal(trd, tro), (self.name, what, "flags")

    def report(self):
        if self.rows_name == "Crypto":
            print(f"{self.name}: {int(self.out.sum())}/{len(self.out)} envs outside the crypto tolerance over the whole test")


def _step_np(ret):
    return tuple(_np(x) for x in ret[:4])


ALL = ["climate", "parking", "snake", "fleet", "traffic", "crypto", "crypto_continuous", "hospital", "manufacturing"]
CANONICAL = ("snake", "crypto", "crypto_continuous", "traffic")          # the types with get_state() / set_state() records


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_captured_steps_replay_and_match_the_oracle(cge, oracle, name, mode):
    make, make_orc, make_acts, dev_act, orc_act, rows_name = _cases(cge, oracle)[name]
    code = {"NextStep": oracle.NEXT_STEP, "SameStep": oracle.SAME_STEP}[mode]
    n = 1000
    env, o = make(n, mode), make_orc(n, code)
    o.seed(np.arange(n, dtype=np.uint64) + np.uint64(9))
    env.reset(seed=9)
    o.reset()
    acts = make_acts(n)
    chk = _Against(name, rows_name, n)

    # warm-up on a side stream (the facade's persistent output buffers and the action conversion's temporaries get allocated)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w = env.step(dev_act(acts[0]))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    chk.step(_step_np(w), o.step(*orc_act(acts[0]))[:4], "warm-up")
    hist = {"obs": torch.empty((K,) + tuple(w[0].shape), dtype=w[0].dtype, device="cuda"), "rew": torch.empty((K, n), device="cuda"),
            "te": torch.empty((K, n), dtype=torch.bool, device="cuda"), "tr": torch.empty((K, n), dtype=torch.bool, device="cuda")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(K):
            ob, r, te, tr, _ = env.step(dev_act(acts[t]))
            hist["obs"][t].copy_(ob); hist["rew"][t].copy_(r); hist["te"][t].copy_(te); hist["tr"][t].copy_(tr)
    ndone = 0
    for rep in range(REPLAYS):                                 # the same graph again and again: the env state carries over, the actions repeat
        g.replay()
        torch.cuda.synchronize()
        h = {k: _np(v) for k, v in hist.items()}
        for t in range(K):
            chk.step((h["obs"][t], h["rew"][t], h["te"][t], h["tr"][t]), o.step(*orc_act(acts[t]))[:4], (rep, t))
        ndone += int((h["te"] | h["tr"]).sum())
    assert ndone > 0                                           # the short time limits end episodes inside the graph, for every type

    # (a) the host's view after the replays: one more eager step on the same env
    chk.step(_step_np(env.step(dev_act(acts[1]))), o.step(*orc_act(acts[1]))[:4], "eager step after the replays")

    # (b) ... and, where the type has canonical records, through get_state() / set_state(): a fresh env with the same arguments takes
    # the records over and must then step exactly as the replayed env does (bitwise), which must go on matching the oracle — for 60
    # steps, more than one length of crypto's ring
    if name in CANONICAL:
        twin = make(n, mode)
        twin.set_state(env.get_state())
        for t in range(60):
            a = acts[(t + 2) % K]
            re, rt = env.step(dev_act(a)), twin.step(dev_act(a))
            for what, x, y in zip(("obs", "reward", "terminated", "truncated"), re[:4], rt[:4]):
                assert torch.equal(x, y), (name, "twin", t, what)
            chk.step(_step_np(re), o.step(*orc_act(a))[:4], ("after get_state/set_state", t))
        twin.close()
    chk.report()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- fused rollout()
RK, RCALLS, RREPLAYS = 7, 4, 3            # 4 captured calls of rollout(7): 28 steps per replay, again not 0 mod 50 (crypto's ring)
assert (RK * RCALLS) % 50 != 0
RT0 = 1000                                # the calls' t0 are constants of the graph: call c hashes steps RT0 + 7 c .. at EVERY replay


def _rollout_cases(cge, oracle):
    """name -> (env(n, mode, reuse), oracle(n, code) or None (then an eager twin env is the reference), hash name, rows name)"""
    return {
        "snake": (lambda n, mode, reuse: cge.SnakeVectorEnv(n, grid_size=10, autoreset_mode=mode, max_steps=7, reuse_buffers=reuse),
                  lambda n, code: oracle.SnakeOracle(n, 10, code, max_steps=7), "snake", "Snake"),
        "crypto": (lambda n, mode, reuse: cge.CryptoVectorEnv(n, action_type="discrete", autoreset_mode=mode, max_steps=13, reuse_buffers=reuse),
                   lambda n, code: oracle.CryptoOracle(n, "discrete", code, max_steps=13), "crypto", "Crypto"),
        "traffic": (lambda n, mode, reuse: cge.TrafficVectorEnv(n, autoreset_mode=mode, max_steps=11, reuse_buffers=reuse),
                    lambda n, code: oracle.TrafficOracle(n, code, max_steps=11), "traffic", "Traffic"),
        "parking": (lambda n, mode, reuse: cge.ParkingVectorEnv(n, autoreset_mode=mode, max_steps=17, reuse_buffers=reuse),
                    lambda n, code: oracle.ParkingOracle(n, code, max_steps=17), "parking", "Parking"),
        "climate": (lambda n, mode, reuse: cge.ClimateVectorEnv(n, autoreset_mode=mode, episode_minutes=9, reuse_buffers=reuse),
                    lambda n, code: oracle.ClimateOracle(n, code, max_steps=9), "climate", "Climate"),
        "hospital": (lambda n, mode, reuse: cge.HospitalVectorEnv(n, autoreset_mode=mode, max_episode_length=12, reuse_buffers=reuse),
                     lambda n, code: oracle.HospitalOracle(n, code, max_steps=12), "hospital", "Hospital"),
        "manufacturing": (lambda n, mode, reuse: cge.ManufacturingVectorEnv(n, autoreset_mode=mode, max_steps=19, reuse_buffers=reuse),
                          lambda n, code: oracle.ManufacturingOracle(n, code, max_steps=19), "manufacturing", "Manufacturing"),
        "bus": (lambda n, mode, reuse: cge.BusVectorEnv(n, autoreset_mode=mode, max_timesteps=9, reuse_buffers=reuse), None, None, None),
        "world_builder": (lambda n, mode, reuse: cge.WorldBuilderVectorEnv(n, autoreset_mode=mode, grid_size=3, reuse_buffers=reuse), None, None, None),
        "world_builder_flat": (lambda n, mode, reuse: cge.WorldBuilderVectorEnv(n, autoreset_mode=mode, grid_size=3, flatten_obs=True, reuse_buffers=reuse),
                               None, None, None),
    }


def _flat(ret):
    """a rollout(per_step=True)'s five outputs as a flat list of tensors (a Dict observation: its tensors in key order, then the rest)"""
    obs = ret[0]
    return ([obs[k] for k in sorted(obs)] if isinstance(obs, dict) else [obs]) + list(ret[1:])


@pytest.mark.parametrize("name", ["snake", "crypto", "traffic", "parking", "climate", "hospital", "manufacturing", "bus", "world_builder",
                                  "world_builder_flat"])
@pytest.mark.parametrize("mode", ["SameStep", "NextStep"])
def test_captured_rollouts_replay_and_match_the_oracle(cge, oracle, name, mode):
    """Four rollout(7, action_seed=s, t0=const, trajectory=True, per_step=True) calls in one graph, replayed three times: every step's
    observation, reward and flags equal the oracle stepped with the actions the hash stands for (tests/_hash_actions.py) — the same
    actions at every replay, because t0 is an argument the graph repeats — and reward_sum / done_count equal the per-step outputs'."""
    make, make_orc, hash_name, rows_name = _rollout_cases(cge, oracle)[name]
    code = {"NextStep": oracle.NEXT_STEP, "SameStep": oracle.SAME_STEP}[mode]
    n, a_seed = 333, 77
    T = RK * RCALLS
    env = make(n, mode, True)
    env.reset(seed=6)
    if make_orc is not None:
        ref = make_orc(n, code)
        ref.seed(np.arange(n, dtype=np.uint64) + np.uint64(6))
        ref.reset()
        acts = _hash_actions.hash_actions(hash_name, a_seed, T, n, t0=RT0)
        chk = _Against(name, rows_name, n)
    else:
        ref = make(n, mode, False)                              # the eager twin: rollout() call by call, never captured
        ref.reset(seed=6)

    def call(e, c):
        return e.rollout(RK, action_seed=a_seed, t0=RT0 + c * RK, trajectory=True, per_step=True)

    def ref_calls():
        """The reference's next RCALLS calls.  Per call, the twin's [obs ..., reward [RK, n], flags [RK, n], reward_sum, done_count],
        or the oracle's RK steps as (obs, reward, terminated, truncated, reward in the precision reward_sum adds up)."""
        out = []
        for c in range(RCALLS):
            if make_orc is None:
                out.append([_np(x) for x in _flat(call(ref, c))])
                continue
            steps = []
            for t in range(RK):
                a = _hash_actions.at(acts, c * RK + t)
                res = ref.step(*a)[:4] if isinstance(a, tuple) else ref.step(a)[:4]
                steps.append(res + (res[1].copy() if name == "snake" else ref.last_reward64.copy(),))
            out.append(steps)
        return out

    # warm-up on a side stream: one call of the same shape allocates the persistent buffers (and is itself checked)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w = call(env, 0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [_np(x) for x in _flat(w)]
    hist = [[torch.empty_like(x) for x in _flat(w)] for _ in range(RCALLS)]

    def compare(got, want, what):
        """got: numpy [obs ..., reward, flags, reward_sum, done_count] of one call; want: ref_calls()[c]"""
        if make_orc is None:
            assert len(got) == len(want)
            for k, (x, y) in enumerate(zip(got, want)):
                assert x.dtype == y.dtype and np.array_equal(x, y), (name, what, "output", k)
            return int(got[-1].sum())
        ob, rt, ft, rs, dc = got
        done = np.zeros(n, np.int64)
        rsum = np.zeros(n, rs.dtype)                          # float64 (snake: float32), added up in step order as the kernels do
        for t, (oo, ro, teo, tro, rfull) in enumerate(want):
            if ft.dtype == np.bool_:                            # the types that never truncate report terminated only
                ted, trd = ft[t], np.zeros(n, bool)
            else:
                ted, trd = (ft[t] & 1).astype(bool), (ft[t] >> 1).astype(bool)
            chk.step((ob[t], rt[t], ted, trd), (oo, ro, teo, tro), (what, t))
            done += (teo | tro).astype(np.int64)
            rsum += rfull.astype(rs.dtype)
        inside = ~chk.out
        assert np.array_equal(dc[inside], done[inside]), (name, what, "done_count")
        if rows_name in ("Crypto", "Climate"):
            assert np.allclose(rs[inside], rsum[inside], rtol=1e-6, atol=1e-3), (name, what, "reward_sum")
        else:
            assert np.array_equal(rs, rsum), (name, what, "reward_sum")
        return int(done.sum())

    want = ref_calls()
    compare(first, want[0], "warm-up")
    for c in range(1, RCALLS):                                 # the reference finishes the warm-up's round of four calls ...
        r = call(env, c)                                       # ... and so does the env, eagerly
        compare([_np(x) for x in _flat(r)], want[c], ("eager", c))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in range(RCALLS):
            for dst, src in zip(hist[c], _flat(call(env, c))):
                dst.copy_(src)
    ndone = 0
    for rep in range(RREPLAYS):
        g.replay()
        torch.cuda.synchronize()
        want = ref_calls()
        for c in range(RCALLS):
            ndone += compare([_np(x) for x in hist[c]], want[c], (rep, c))
    assert ndone > 0 or name.startswith("world_builder")        # (the world builder has no time limit: no episode ends this early)
    if make_orc is not None:
        chk.report()
    else:
        ref.close()
    env.close()
