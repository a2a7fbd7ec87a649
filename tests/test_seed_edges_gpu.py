"""reset(seed=...) at the 32- and 64-bit boundaries, for all fifteen env types.

Env i's stream is the reference's generator seeded with s_i = seed + env_index0 + i, or seeds[i].  CPython's init_by_array key and
SeedSequence's entropy grow from one 32-bit word to two at s_i = 2**32, and the kernels decide that per lane; np.random.seed takes 32
bits and raises above them, as the five types that call it now do; from 2**64 on every generator takes a third limb, which is
refused.  Every case compares the reset observation, K hash-action steps (tests/_seed_edges.py: the K table, what is compared and how
both sides produce it) and, for the record-lane types, the info columns, with the CPU oracle (the comparison of
tests/test_edges_gpu.py::test_per_env_seed_lists: bit for bit, crypto within the tolerance stated there) or the type's Python model
(bit patterns, no row skipped).  tests/test_seed_edges_cpu.py shows that these references tell the edge seeds apart within K steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import _seed_edges as se
from _lane_kit import cge  # noqa: F401
from test_edges_gpu import _assert_match, _rows_ok

pytestmark = pytest.mark.gpu

N = 130                                                                   # two waves plus two lanes
CROSS1 = 2 ** 32 - 40                                                     # case 1: lanes 0-39 one-limb, 40-129 two-limb
ENV0, CROSS2 = 1000, 2 ** 32 - 1100                                       # case 2: the crossing at lane 100, inside the second wave
N32, LAST32 = 65, 2 ** 32 - 65                                            # case 4: the last lane gets 2**32 - 1
DIRTY_SEED, DIRTY_STEPS, DIRTY_ACTIONS = 977, 120, 3                      # case 5: emergency passes a generator twist within 120 steps
_REFERENCES = {}


def ref_of(oracle, name, seeds, env0=0):
    """the reference's data for these seeds at the type's K: computed once, shared by the tests that need it, never changed"""
    key = (name, tuple(int(s) for s in seeds), env0)
    if key not in _REFERENCES:
        _REFERENCES[key] = se.reference(name, seeds, se.K[name], env0=env0, oracle=oracle)
    return _REFERENCES[key]


def compare(name, dev, ref, what):
    if name not in se.ORACLE:
        se.assert_same(dev, ref, what)
        return
    assert list(dev) == list(ref) == ["reset", "final", "reward_sum", "done_count"]
    ok = _rows_ok(name, dev["reset"], ref["reset"])
    assert ok.all(), (what, "reset", np.argwhere(~ok)[:5])
    _assert_match(name, (dev["final"], dev["reward_sum"], dev["done_count"]), (ref["final"], ref["reward_sum"], ref["done_count"]), what)


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the crossing
@pytest.mark.parametrize("name", se.WIDE64)
def test_crossing_inside_the_first_wave(cge, oracle, name):
    env = se.make_env(cge, name, N)
    dev = se.device(env, name, CROSS1, se.K[name])
    compare(name, dev, ref_of(oracle, name, [CROSS1 + i for i in range(N)]), "crossing at lane 40")
    env.close()


@pytest.mark.parametrize("name", se.WIDE64)
def test_crossing_inside_the_second_wave_through_env_index0(cge, oracle, name):
    env = se.make_env(cge, name, N, env_index0=ENV0)
    dev = se.device(env, name, CROSS2, se.K[name])
    compare(name, dev, ref_of(oracle, name, [CROSS2 + ENV0 + i for i in range(N)], env0=ENV0), "crossing at lane 100")
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3: edge lists
@pytest.mark.parametrize("form", ["ints", "uint64"])
@pytest.mark.parametrize("name", se.TYPES)
def test_edge_seed_lists(cge, oracle, name, form):
    """the edge list of the type's width tiled over the batch (neighbouring lanes alternate one-limb and two-limb keys), as a list
    of Python ints and as a uint64 array; the 32-bit types take their members below 2**32, 2**32 - 1 among them"""
    seeds = se.edge_seeds(name, N)
    env = se.make_env(cge, name, N)
    dev = se.device(env, name, seeds if form == "ints" else np.array(seeds, dtype=np.uint64), se.K[name])
    compare(name, dev, ref_of(oracle, name, seeds), form)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4: the last valid seed
@pytest.mark.parametrize("name", se.LEGACY32)
def test_up_to_the_last_valid_seed_of_the_32_bit_types(cge, oracle, name):
    env, twin = se.make_env(cge, name, N32), se.make_env(cge, name, N32)
    seeds = [LAST32 + i for i in range(N32)]
    assert seeds[-1] == 2 ** 32 - 1
    compare(name, se.device(env, name, LAST32, se.K[name]), ref_of(oracle, name, seeds), "the last lane gets 2**32 - 1")
    se.device(twin, name, LAST32, se.K[name])
    with pytest.raises(ValueError, match=r"between 0 and 2\*\*32 - 1"):     # one more and the last lane would get the stream of seed 0
        env.reset(seed=LAST32 + 1)
    se.continue_equally(env, twin)
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 5: a dirty handle
@pytest.mark.parametrize("name", se.TYPES)
def test_reseeding_a_dirty_handle_equals_a_fresh_one(cge, oracle, name):
    """a handle that has run (cursors mid-generation, ready marks ahead of them, farm's cached Gaussian and second stream, the
    networks of airline and emergency drawn from the old seed) and is then given reset(seed=s) equals a fresh handle given the
    same, bit for bit, and the reference.  Crypto is the one type whose reference keeps state across a seeded reset: its
    MarketSimulator (regime, trend, psychology, the last close) is made once per env and reset by nothing (include/cge_amd.h,
    cge_crypto_seed), so a dirty crypto handle is not a fresh one in the reference either; it is compared with the oracle that has
    the same history (which the other seven oracle types are compared with too, beside the fresh reference)."""
    n, s = (N, CROSS1) if name in se.WIDE64 else (N32, LAST32)
    seeds = [s + i for i in range(n)]
    env, fresh = se.make_env(cge, name, n), se.make_env(cge, name, n)
    env.reset(seed=DIRTY_SEED)
    env.rollout(DIRTY_STEPS, action_seed=DIRTY_ACTIONS)
    dirty = se.device(env, name, s, se.K[name])
    if name in se.ORACLE:
        compare(name, dirty, se.reference(name, seeds, se.K[name], oracle=oracle, history=(DIRTY_SEED, DIRTY_STEPS, DIRTY_ACTIONS)), "dirty against the oracle with its history")
    if name != "Crypto":
        se.assert_same(dirty, se.device(fresh, name, s, se.K[name]), "dirty against fresh")
        compare(name, dirty, ref_of(oracle, name, seeds), "dirty against the reference")
        se.continue_equally(env, fresh)
    env.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 6: refusals
@pytest.mark.parametrize("name", se.TYPES)
def test_refused_seeds_leave_the_handle_as_it_was(cge, oracle, name):
    """every refusal is raised before anything native is called: it seeds nothing, resets nothing and leaves no last_error, so a
    twin that never saw the bad calls continues identically.  What is no integer array is a TypeError."""
    n, bits = N32, se.bits_of(name)
    last_base = 2 ** bits - ENV0 - n                                        # its last lane gets 2**bits - 1
    env, twin = se.make_env(cge, name, n, env_index0=ENV0), se.make_env(cge, name, n, env_index0=ENV0)
    dev = se.device(env, name, last_base, se.K[name])                       # accepted, and the reference's
    compare(name, dev, ref_of(oracle, name, [last_base + ENV0 + i for i in range(n)], env0=ENV0), "the last valid base")
    se.device(twin, name, last_base, se.K[name])
    good = list(range(n))
    words = r"between 0 and 2\*\*32 - 1" if bits == 32 else r"between 0 and 2\*\*64 - 1"

    def bad_list(value):
        out = list(good)
        out[n - 2] = value
        return out
    for seed in (last_base + 1, 2 ** bits, bad_list(2 ** bits), np.array(bad_list(2 ** 32), dtype=np.uint64) if bits == 32 else bad_list(2 ** 64 + 5)):
        with pytest.raises(ValueError, match=words):
            env.reset(seed=seed)
    for seed in (2 ** 64 - ENV0 - n + 1, 2 ** 64 + 5, bad_list(2 ** 64), -1, bad_list(-1), np.array(bad_list(-1), dtype=np.int64), good[:-1]):
        with pytest.raises(ValueError):
            env.reset(seed=seed)
    for seed in (np.array(good, dtype=np.float64), np.array(good, dtype=np.float32), np.array(good) % 2 == 0, bad_list(1.0), bad_list(True)):
        with pytest.raises(TypeError):
            env.reset(seed=seed)
    assert env._c_last_error(env._h) == twin._c_last_error(twin._h) == b""
    se.continue_equally(env, twin)
    env.reset(seed=good); twin.reset(seed=np.array(good, dtype=np.int32))  # and the handle takes the next valid seeds
    se.continue_equally(env, twin)
    env.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 7: shards
@pytest.mark.parametrize("name", ["Snake", "Climate", "Emergency"])
def test_shards_across_the_boundary(cge, oracle, name):
    """CPython, PCG64 and the lane kit: three shards of 200 envs, the crossing (env 100) inside shard 1"""
    n, seed = 200, 2 ** 32 - 100
    cls, kw = getattr(cge, se.ENV_CLASS[name]), se.env_kwargs(name)
    whole_env = se.make_env(cge, name, n)
    whole = se.device(whole_env, name, seed, se.K[name])
    compare(name, whole, ref_of(oracle, name, [seed + i for i in range(n)]), "the whole batch")
    parts = []
    for rank in range(3):
        p = cge.make_sharded(cls, n, rank=rank, world_size=3, local_rank=0, autoreset_mode="SameStep", **kw)
        parts.append(se.device(p, name, seed, se.K[name]))
        if rank == 1:
            assert p.shard[0] < 100 < p.shard[0] + p.shard[1] - 1
        p.close()
    se.assert_same(se.concat_envs(parts), whole, "shards against the whole")
    whole_env.close()


# ---------------------------------------------------------------------------------------------------------------- 8: the C ABI
@pytest.mark.parametrize("name", ["Snake", "Climate", "WorldBuilder", "Crypto", "Emergency", "Farm"])
def test_c_abi_refuses_a_base_seed_past_the_limit(cge, name):
    """cge_<env>_seed(h, NULL, base, stream) itself: init_by_array (snake), SeedSequence (climate), init_genrand through lane_seed
    (world builder), and beside the three families the hand-written legacy seeds (crypto, farm) and lane_seed at 64 bits (emergency)"""
    from custom_gymnasium_environments_amd import _native
    n, bits = N32, se.bits_of(name)
    last_base = 2 ** bits - ENV0 - n
    env, twin = se.make_env(cge, name, n, env_index0=ENV0), se.make_env(cge, name, n, env_index0=ENV0)
    se.device(env, name, 11, se.K[name]); se.device(twin, name, 11, se.K[name])
    seed_fn = getattr(cge.native_lib(), env._abi + "_seed")
    bad = [last_base + 1, 2 ** bits - 1] + ([2 ** 32, 2 ** 64 - 1] if bits == 32 else [])
    for base in bad:
        status = seed_fn(env._h, None, C.c_uint64(base), env._stream())
        assert status == -1 and _native.STATUS_NAMES[status] == "CGE_ERR_INVALID_ARG", base
        text = env._c_last_error(env._h).decode()
        assert env._abi + "_seed" in text and f"between 0 and 2**{bits} - 1" in text, text
    se.continue_equally(env, twin)                                          # nothing was seeded, nothing reset
    assert seed_fn(env._h, None, C.c_uint64(last_base), env._stream()) == 0
    obs, _ = env.reset()
    ref, _ = twin.reset(seed=last_base)
    assert all(torch.equal(obs[k], ref[k]) for k in ref) if isinstance(ref, dict) else torch.equal(obs, ref)
    se.continue_equally(env, twin)
    env.close(); twin.close()
