"""WHERE every entry point of every env type writes: nothing outside the outputs it was given, and no byte of them unwritten.

The rest of the suite compares values in the rows a kernel was handed.  Here every output of a call is a view of one arena
(tests/_guard_bands.py) with a wave-wide guard band of a fill byte round it; every case runs twice in lockstep, over the fills 0x7F and
0x80, with the same seeds and actions.  After every call: every byte outside the outputs still holds its fill, what the call returned IS
the planted memory (`data_ptr`), and the outputs agree between the two fills byte for byte, so every byte of them was written.

Batch sizes: 1 (a single lane), 63 (a wave one short of full), 65 (one lane into the second wave), 257 (one env past a 256-thread
block), and S - 1 and S + 1 for the types whose terminal-row segment S is not 64 (traffic and hospital step an env per quad: 16 envs per
wave).  Constructor arguments, short limits and action generators are those of tests the suite already has (test_edges_gpu.SHORT, the
SPECs of the four record-lane types, the hashed cases of test_slab_final_rows_gpu.py).  `env_index0` is 1000 throughout.

Order of the terminal rows within a segment: fleet is the one type whose kernel does not fix it.  Its step kernel serves work-list entries,
not contiguous envs, and takes a finishing env's slot with a returning atomicAdd on the segment's count (fleet.hip, "one returning atomic
per finishing env"), so the envs that end at one step share their slots in arbitration order.  Every other type keeps a segment's fill count
in a register of the one wave that steps the segment and hands its finishing lanes consecutive slots in lane order (`final_slot`,
cge_device.hpp).  The delivered rows are therefore compared through `final_obs()`, which sorts by (step, env) — for every type, since the
comparison holds either way.  WHICH slots are written is checked slot by slot all the same: slots below a segment's `count` are owned,
the others must keep the fill."""
import types

import numpy as np
import pytest
import torch

import farm_model as fm
from _action_streams import FINAL_OBS_CASES, FINAL_OBS_SEGMENT, edges_short_limit, edges_trajectory_block, final_obs_actions
from _guard_bands import (FILLS, ROLLOUT_KEYS, STEP_KEYS, Arena, final_rows_requests, output_requests, plane_byte_mask, plant, register_final_rows,
                          register_stats, request, stats_requests, written_everywhere)
from test_airline_gpu import SPEC as AIRLINE
from test_edges_gpu import SHORT, _dev
from test_emergency_gpu import SPEC as EMERGENCY
from test_slab_final_rows_gpu import A_SEED, ENV0, T0, WB_K, Hashed
from test_space_station_gpu import SPEC as STATION

pytestmark = pytest.mark.gpu

MODES3 = ["NextStep", "SameStep", "Disabled"]
SIZES = [1, 63, 65, 257]
OLD = ("Snake", "Snake-g15", "Crypto", "Crypto-continuous", "Traffic", "Parking", "Climate", "Fleet", "Manufacturing", "Hospital")


@pytest.fixture(scope="module")
def cge():
    import custom_gymnasium_environments_amd as m
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    m.native_lib()
    return m


# ---------------------------------------------------------------------------------------------------------------- the kinds
# kind -> cls, constructor arguments with a short limit, steps (limit + 3, or the type's own count), reset seed, steps(n, T) -> the host
# actions of T step() calls, block(k, n) -> the host actions of a rollout with given actions, pad (the smallest trajectory padding the
# header allows, in elements of the observation layout), t0 (the step counter at which the hash actions of the first rollout start)
KINDS = {}


def kind(name, cls, kw, steps, seed, step_actions, block, pad, t0=0):
    KINDS[name] = types.SimpleNamespace(name=name, cls=cls, kw=kw, steps=steps, seed=seed, step_actions=step_actions, block=block, pad=pad, t0=t0)


def _old(name, kw, limit, nact, ashape, label=None, continuous=False):
    if continuous:                                                        # the continuous twin of SHORT's crypto row, as test_final_obs_oracle_gpu.py runs it
        acts = lambda n, T: list(final_obs_actions("crypto", {"continuous": True}, T, n, np.random.default_rng(limit)))
        block = lambda k, n: final_obs_actions("crypto", {"continuous": True}, k, n, np.random.default_rng(7))
    else:
        acts = lambda n, T: list(edges_short_limit(name, limit, n, T, nact, ashape))
        block = lambda k, n: edges_trajectory_block(name, k, n, nact, ashape)
    # cge_amd.h states no stride multiple for these; a snake grid whose cells are a multiple of 4 takes strides that are multiples of 4
    kind(label or name, name + "VectorEnv", kw, limit + 3, 17, acts, block, 4)


for _name, _kw, _, _, _limit, _nact, _ashape in SHORT:
    _old(_name, _kw, _limit, _nact, _ashape)
    if _name == "Snake":
        _old(_name, dict(_kw, grid_size=15), _limit, _nact, _ashape, label="Snake-g15")
    if _name == "Crypto":
        _ckw = FINAL_OBS_CASES["crypto_continuous"][1]
        assert _ckw["max_steps"] == _limit
        _old(_name, dict(_kw, action_type=_ckw["action_type"]), _limit, _nact, _ashape, label="Crypto-continuous", continuous=True)


def _model(name, cls, model, kw, steps, seed, pad, t0=0):
    kind(name, cls, kw, steps, seed, lambda n, T: list(model.hash_actions(A_SEED, T, n, t0=t0, env0=ENV0)),
         lambda k, n: model.hash_actions(7, k, n, env0=ENV0), pad, t0)


for _h in (Hashed("bus"), Hashed("restaurant")):                          # limit 5: the hashed cases of test_slab_final_rows_gpu.py
    _model({"bus": "Bus", "restaurant": "Restaurant"}[_h.type], _h.spec.env, _h.spec.m, _h.kw, 5 + 3, 3, {"bus": 4, "restaurant": 1}[_h.type])
for _h in (Hashed("wb-3-dict"), Hashed("wb-3-flat")):                     # no time limit: the 24 steps from t0 = 5 in which every env ends
    _model("WorldBuilder-" + _h.kind.split("-")[2], _h.spec.env, _h.spec.m, _h.kw, WB_K, 3, 1 if _h.flat else 16, t0=T0)
for _s, _label in ((AIRLINE, "Airline"), (EMERGENCY, "Emergency"), (STATION, "SpaceStation")):
    _T, _seed, _limit, _ = _s.kernel                                      # the kit's kernel_equals_the_model: every env ends within T (airline: no limit keyword)
    _model(_label, _s.env, _s.m, {_s.limit: _limit} if _s.limit else {}, _T if _limit is None else _limit + 3, _seed, 4)
# test_farm_gpu.SPEC has no `kernel` entry (its own test of the kernel is written out): the limit keyword is SPEC.limit, the reset seed and
# the 360 steps of a year are those of test_farm_gpu.py::test_rollout_equals_steps_and_the_model, where day 360 ends every env's episode
for _label, _kw, _pad in (("Farm", {}, 4), ("Farm-compact", {"compact_obs": True}, 2)):
    _model(_label, "AgriculturalFarmVectorEnv", fm, dict(_kw, max_years=1), 360 + 3, 40, _pad)      # a year is 360 steps

assert len({k.cls for k in KINDS.values()}) == 15 and len(KINDS) == 19


def segment(name):
    return FINAL_OBS_SEGMENT.get(name.split("-")[0].lower(), 64)


def sizes(name, base=SIZES):
    s = segment(name)
    return sorted(set(base) | ({s - 1, s + 1} if s != 64 else set()))


CASES = [(name, n) for name in KINDS for n in sizes(name)]


def make(cge, K, n, mode, **extra):
    return getattr(cge, K.cls)(n, autoreset_mode=mode, env_index0=ENV0, reuse_buffers=True, **K.kw, **extra)


def tensor_of(env, obs):
    """the buffer behind what a call returned: the slab behind a dict"""
    return env.obs_slab(obs) if isinstance(obs, dict) else obs


def slab_mask(env, rows=None, steps=1, planes=None, num=None, nbytes=None):
    """bool per byte of `steps` observation buffers of env, on the device: the bytes that belong to a plane (of the envs `rows` only).
    planes, num, nbytes: another slab of the type's layout instead (the terminal rows: `num` slots in `nbytes` bytes)."""
    planes = getattr(env, "_planes", None) if planes is None else planes
    num = env.num_envs if num is None else num
    item = torch.empty((), dtype=env._obs_dtype).element_size()
    if planes is None:                                                    # plain rows: every byte belongs to a row
        m = torch.ones(num, int(np.prod(env._obs_shape[1:])) * item, dtype=torch.bool)
        if rows is not None:
            m &= torch.as_tensor(rows, dtype=torch.bool).cpu()[:, None]
        m = m.reshape(-1)
    else:
        m = plane_byte_mask(planes, num, env._slab * item if nbytes is None else nbytes, item, rows)
    return m.cuda().repeat(steps)


class Pair:
    """The same env twice, each with its outputs in an arena of its own fill; every call is made on both.  Before a call, every output
    the call is claimed to write is filled afresh (`refill`), so that agreement between the two fills afterwards is the work of THAT call
    and not of an earlier one.  `masks` holds what of an output counts as owned (the planes of a slab, the front of a longer buffer)."""

    def __init__(self, cge, K, n, mode, keys, k=None, stats=False, rows=False):
        self.K, self.n, self.envs, self.arenas, self.masks = K, n, [], [], {}
        for fill in FILLS:
            env = make(cge, K, n, mode, record_episode_statistics=stats)
            req = output_requests(env, keys, k)
            if rows:
                env.collect_final_obs(rows_per_env=4)
                assert env.final_obs_segment == segment(K.name)
            extra = (stats_requests(env) if stats else []) + (final_rows_requests(env) if rows else [])
            arena = Arena.sized_for(fill, "cuda", req + extra)
            plant(env, arena, req)
            if stats:
                register_stats(env, arena)
            if rows:
                register_final_rows(env, arena)
            self.envs.append(env); self.arenas.append(arena)
        env, views = self.envs[0], self.arenas[0].views
        for key in ("obs", "final_obs"):                                  # world builder: the padding between the planes is nobody's
            if key in views:
                self.masks[key] = slab_mask(env)
        if "traj" in views:
            self.masks["traj"] = slab_mask(env, steps=k)
        self.refill(self.masks)

    def refill(self, keys):
        """the outputs `keys` hold their arena's fill again and are owned as `masks` says"""
        for arena in self.arenas:
            for key in keys:
                arena.reset(key)
                if self.masks.get(key) is not None:
                    arena.restrict(key, self.masks[key])

    def call(self, fn, what, planted=(), written=(), partly=(), fresh=()):
        """fn(env) -> what it returned, on both; planted: (key, returned -> tensor); written: keys written whole; partly: (key, byte mask);
        fresh: further keys to refill before the call (`written` always are)"""
        self.refill(list(written) + list(fresh))
        outs = [fn(env) for env in self.envs]
        for env, arena, out in zip(self.envs, self.arenas, outs):
            arena.outside_untouched((self.K.name, self.n, what, hex(arena.fill)))
            for key, get in planted:
                arena.is_planted(key, tensor_of(env, get(out)), (self.K.name, what))
        a, b = self.arenas
        for key in written:
            assert written_everywhere(a, b, key, what=(self.K.name, self.n, what)) > 0
        for key, mask in partly:
            written_everywhere(a, b, key, mask=mask, what=(self.K.name, self.n, what))
        return outs

    def close(self):
        for env in self.envs:
            env.close()


# ---------------------------------------------------------------------------------------------------------------- reset() and step()
@pytest.mark.parametrize("mode", MODES3)
@pytest.mark.parametrize("name, n", CASES)
def test_reset_and_step(cge, name, n, mode):
    K = KINDS[name]
    p = Pair(cge, K, n, mode, STEP_KEYS, stats=True)
    env, views = p.envs[0], p.arenas[0].views
    flags = [key for key in ("terminated", "truncated", "done") if key in views]
    assert ("truncated" in views) == (env._flags != "terminated") and ("done" in views) == (env._flags == "both") and ("final_obs" in views) == (mode == "SameStep")
    p.call(lambda e: e.reset(seed=K.seed), "reset", planted=[("obs", lambda o: o[0])], written=["obs"])
    acts = K.step_actions(n, K.steps)
    ever = torch.zeros(n, dtype=torch.bool)
    for t in range(K.steps):
        a = _dev(acts[t])
        planted = [("obs", lambda o: o[0]), ("reward", lambda o: o[1]), ("terminated", lambda o: o[2])]
        if "truncated" in views:
            planted.append(("truncated", lambda o: o[3]))
        if "done" in views:
            planted.append(("done", lambda o: o[4]["_episode"]))
        if mode == "SameStep":
            planted.append(("final_obs", lambda o: o[4]["final_obs"]))
        outs = p.call(lambda e: e.step(a), ("step", t), planted=planted, written=["obs", "reward"] + flags, fresh=["final_obs"] if mode == "SameStep" else [])
        ended = outs[0][4]["_episode"].cpu()
        assert torch.equal(ended, outs[1][4]["_episode"].cpu())
        if ended.any():
            ever |= ended
            partly = [("ep_ret", slab_mask_rows(ended, 8)), ("ep_len", slab_mask_rows(ended, 4))]
            if mode == "SameStep":                                        # the rows of the envs that ended, whole; no claim about the others
                partly.append(("final_obs", slab_mask(env, rows=ended)))
            for key, mask in partly:
                written_everywhere(*p.arenas, key, mask=mask, what=(name, n, "step", t))
    assert n < 63 or ever.any(), "no env ended during the steps: the case would be vacuous"
    if mode == "Disabled":                                                # "returns every row"
        mask = (ever if ever.any() else ~ever).numpy().astype(np.uint8)
        p.call(lambda e: e.reset(options={"reset_mask": mask}), "masked reset", planted=[("obs", lambda o: o[0])], written=["obs"])
    p.close()


def slab_mask_rows(rows, item):
    return rows[:, None].expand(rows.numel(), item).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- rollout()
def restrict_final_rows(env, arena):
    """after a rollout: slots below a segment's count (plane by plane for a slab) are the call's; the others must keep the fill"""
    rows, index, count, cap = env._fin
    used = (torch.arange(cap)[None, :] < count.cpu().clamp(max=cap)[:, None]).reshape(-1)
    arena.restrict("index", slab_mask_rows(used, 8))
    arena.restrict("rows", slab_mask(env, rows=used, planes=getattr(env, "_fin_planes", None), num=used.numel(), nbytes=rows.numel() * rows.element_size()))
    return int(used.sum())


def same_rows(x, y):
    x, y = (v if isinstance(v, dict) else {"rows": v} for v in (x, y))
    return list(x) == list(y) and all(torch.equal(x[k].contiguous().view(torch.uint8), y[k].contiguous().view(torch.uint8)) for k in x)


@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("name, n", CASES)
def test_rollout(cge, name, n, mode):
    K = KINDS[name]
    rows = mode == "SameStep" and name != "Airline"                       # the airline has no terminal-row output (cge_amd.h declares none)
    p = Pair(cge, K, n, mode, ("obs",) + ROLLOUT_KEYS, k=K.steps, rows=rows)
    p.call(lambda e: e.reset(seed=K.seed), "reset", planted=[("obs", lambda o: o[0])], written=["obs"])
    traj_keys = ("traj", "reward_traj", "flags_traj")
    t0, delivered = K.t0, 0
    for k, given in ((K.steps, False), (K.steps, True), (5, False), (5, True)):      # the shorter ones after the longer: `_out` hands out the front
        acts = _dev(K.block(k, n)) if given else None
        if k < K.steps:                                                   # the planted bytes behind the shorter trajectory must not be written
            for key in traj_keys:
                view = p.arenas[0].views[key]
                front = torch.zeros(view.numel() * view.element_size(), dtype=torch.bool, device="cuda")
                front[:front.numel() // K.steps * k] = True
                p.masks[key] = front & slab_mask(p.envs[0], steps=K.steps) if key == "traj" else front
        planted = [(key, lambda o, j=j: o[j]) for j, key in enumerate(traj_keys + ("reward_sum", "done_count"))]
        what = ("rollout", k, "given" if given else "hash")
        if not rows:
            outs = p.call(lambda e: e.rollout(k, actions=acts, action_seed=A_SEED, t0=t0, trajectory=True, per_step=True), what, planted, [key for key, _ in planted])
        else:
            p.refill([key for key, _ in planted] + ["rows", "index", "count"])
            outs = [env.rollout(k, actions=acts, action_seed=A_SEED, t0=t0, trajectory=True, per_step=True) for env in p.envs]
            used = [restrict_final_rows(env, arena) for env, arena in zip(p.envs, p.arenas)]     # the counts are known only now
            assert used[0] == used[1]
            delivered += used[0] if k == K.steps else 0
            slots = ["rows", "index"] if used[0] and name != "Fleet" else []              # fleet: which env got which slot differs from run to run
            p.call(lambda e: None, what)
            for key in [key for key, _ in planted] + ["count"] + slots:
                assert written_everywhere(*p.arenas, key, what=(name, n, what)) > 0
            for env, arena, out in zip(p.envs, p.arenas, outs):
                for key, get in planted:
                    arena.is_planted(key, tensor_of(env, get(out)), what)
                assert env.final_obs_dropped() == 0, what
            (ra, sa, wa), (rb, sb, wb) = (env.final_obs() for env in p.envs)             # sorted by (step, env): fleet's slots are in no fixed order
            assert torch.equal(sa, sb) and torch.equal(wa, wb) and same_rows(ra, rb) and sa.numel() == used[0], what
        assert torch.equal(outs[0][2], outs[1][2])
        t0 += k
    assert not rows or delivered > 0, "no segment delivered a row: the case would be vacuous"
    for env in p.envs:                                                    # the calls below leave the trajectory buffers and the rows alone
        if rows:
            env.collect_final_obs(0)
    for key in traj_keys + (("rows", "index", "count") if rows else ()):
        view = p.arenas[0].views[key]
        p.masks[key] = torch.zeros(view.numel() * view.element_size(), dtype=torch.bool, device="cuda")
        p.refill([key])
    both = ["reward_sum", "done_count"]
    for k in (K.steps, 5):
        p.call(lambda e: e.rollout(k, action_seed=A_SEED, t0=t0), ("rollout", k, "last rows"),
               planted=[("obs", lambda o: o[0]), ("reward_sum", lambda o: o[1]), ("done_count", lambda o: o[2])], written=["obs"] + both)
        t0 += k
        outs = p.call(lambda e: e.rollout(k, action_seed=A_SEED, t0=t0, want_obs=False), ("rollout", k, "no obs"),
                      planted=[("reward_sum", lambda o: o[1]), ("done_count", lambda o: o[2])], written=both)
        assert outs[0][0] is None
        t0 += k
    p.close()


# ---------------------------------------------------------------------------------------------------------------- strided trajectories
def strided(cge, K, n, mode, pad):
    """`cge_<env>_rollout` with obs_step_stride = step_elems + pad, straight through the C ABI: the pad elements between the steps and
    behind the last keep the fill, every step's block equals the same step of an unpadded trajectory of an eager twin"""
    k = min(K.steps, 30)
    twin = make(cge, K, n, mode)
    twin.reset(seed=K.seed)
    ref = tensor_of(twin, twin.rollout(k, action_seed=A_SEED, t0=3, trajectory=True, per_step=True)[0]).reshape(k, -1).clone()
    twin.close()
    step = ref.shape[1]
    for fill in FILLS:
        env = make(cge, K, n, mode)
        item = torch.empty((), dtype=env._obs_dtype).element_size()
        assert step == env._obs_stride
        req = [request("traj", (k * (step + pad),), env._obs_dtype, row_bytes=step * item // n)] + output_requests(env, ROLLOUT_KEYS[1:], k)
        arena = Arena.sized_for(fill, "cuda", req)
        v = arena.take_all(req)
        own = torch.zeros(k, (step + pad) * item, dtype=torch.bool)
        own[:, :step * item] = slab_mask(env)[None, :]
        arena.restrict("traj", own)
        env.reset(seed=K.seed)
        status = env._c_rollout(env._h, k, *([None] * env._action_ptrs), A_SEED, 3, v["traj"].data_ptr(), step + pad, v["reward_traj"].data_ptr(),
                                v["flags_traj"].data_ptr(), v["reward_sum"].data_ptr(), v["done_count"].data_ptr(), env._stream())
        assert status == 0, (K.name, n, pad, env._c_last_error(env._h))
        arena.outside_untouched((K.name, n, "stride", step + pad, hex(fill)))
        got = v["traj"].view(k, step + pad)[:, :step]
        keep = slab_mask(env).cuda()
        assert torch.equal(got.contiguous().view(torch.uint8)[:, keep], ref.view(torch.uint8)[:, keep]), (K.name, n, pad, "a step's block differs from the unpadded trajectory")
        env.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("n", [63, 65])
@pytest.mark.parametrize("name", list(KINDS))
def test_strided_trajectory(cge, name, n, mode):
    strided(cge, KINDS[name], n, mode, KINDS[name].pad)


@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("n", [63, 65])
@pytest.mark.parametrize("name", [k for k in OLD if k != "Snake"])
def test_stride_of_one_more_element(cge, name, n, mode):
    """The eight older types and odd-grid snake state no stride multiple: a pad of ONE element puts every step's rows at 4-byte-aligned
    addresses (byte-aligned for snake at G = 15), where the 16-byte store forms of `store_own_row` and `stream_image` run."""
    strided(cge, KINDS[name], n, mode, 1)


# ---------------------------------------------------------------------------------------------------------------- small outputs
SMALL = [(name, n) for name in KINDS for n in (1, 63, 65)]
INVALID_ARG = -1                                                          # CGE_ERR_INVALID_ARG


@pytest.mark.parametrize("name, n", SMALL)
def test_info(cge, name, n):
    """every field, through cge_<env>_info into a view of the type's info dtype: written whole (with index 1 where the type takes one)"""
    K = KINDS[name]
    envs, arenas = [], []
    for fill in FILLS:
        env = make(cge, K, n, "SameStep")
        env.reset(seed=K.seed)
        env.rollout(5, action_seed=A_SEED)
        req = [request(f, (n,), env._info_dtype) for f in env.INFO_FIELDS] + [request(f, (n,), torch.float64) for f in env.INFO64_FIELDS]
        arena = Arena.sized_for(fill, "cuda", req)
        v = arena.take_all(req)
        for f, code in env.INFO_FIELDS.items():
            if env._info_indexed:
                status = env._c_info(env._h, code, 1, v[f].data_ptr(), env._stream())
                if status:                                                # only a field without items may refuse index 1, and only as a bad argument
                    assert status == INVALID_ARG and b"index" in env._c_last_error(env._h), (name, f, status)
                    arena.outside_untouched((name, n, "refused info", f))
                    status = env._c_info(env._h, code, 0, v[f].data_ptr(), env._stream())
            else:
                status = env._c_info(env._h, code, v[f].data_ptr(), env._stream())
            assert status == 0, (name, f)
            arena.outside_untouched((name, n, "info", f))
        for f, code in env.INFO64_FIELDS.items():
            assert getattr(env._lib, env._abi + "_info64")(env._h, code, v[f].data_ptr(), env._stream()) == 0
            arena.outside_untouched((name, n, "info64", f))
        envs.append(env); arenas.append(arena)
    assert len(arenas[0].views) > 0
    for f in arenas[0].views:
        assert written_everywhere(*arenas, f, what=(name, n, "info")) == n * arenas[0].views[f].element_size()
    for env in envs:
        env.close()


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("name", ["Snake", "Snake-g15"])
def test_render_rgb(cge, name, n):
    K = KINDS[name]
    arenas = []
    for fill in FILLS:
        env = make(cge, K, n, "SameStep")
        req = output_requests(env, ("rgb",))
        arena = Arena.sized_for(fill, "cuda", req)
        plant(env, arena, req)
        env.reset(seed=K.seed)
        env.rollout(5, action_seed=A_SEED)
        for _ in range(2):
            arena.is_planted("rgb", env.render_rgb(), name)
            arena.outside_untouched((name, n, "render_rgb"))
        arenas.append(arena)
        env.close()
    g = env.grid_size
    assert written_everywhere(*arenas, "rgb", what=(name, n)) == n * g * g * 3


@pytest.mark.parametrize("name, n", SMALL)
def test_action_sampler_out(cge, name, n):
    K = KINDS[name]
    arenas = []
    for fill in FILLS:
        env = make(cge, K, n, "SameStep")
        sampler = env.action_sampler(5)
        req = [request(str(key), lf.shape, lf.dtype) for key, lf in sampler._leaves.items()]
        arena = Arena.sized_for(fill, "cuda", req)
        v = arena.take_all(req)
        for _ in range(3):
            out = sampler.sample(out={key: v[str(key)] for key in sampler._leaves} if sampler._mapping else v["None"])
            for key in sampler._leaves:
                arena.is_planted(str(key), out[key] if sampler._mapping else out, name)
            arena.outside_untouched((name, n, "sample"))
        arenas.append(arena)
        sampler.close(); env.close()
    for key in arenas[0].views:
        assert written_everywhere(*arenas, key, what=(name, n, "sample")) > 0


@pytest.mark.parametrize("name, n", SMALL)
def test_state_records_on_the_host(cge, name, n):
    """get_state (the types with canonical records) or snapshot_get (the others) into host memory with guard bytes on both sides"""
    K = KINDS[name]
    G, got = 4096, []
    for fill in FILLS:
        env = make(cge, K, n, "SameStep")
        env.reset(seed=K.seed)
        env.rollout(5, action_seed=A_SEED)
        canonical = hasattr(env._lib, env._abi + "_get_state")
        nbytes = n * int(env._fn("state_bytes")(env._h)) if canonical else int(env._fn("snapshot_bytes")(env._h))
        buf = np.full(G + nbytes + G, fill, np.uint8)
        assert env._fn("get_state" if canonical else "snapshot_get")(env._h, buf.ctypes.data + G, env._stream()) == 0
        torch.cuda.synchronize()
        assert nbytes > 0 and (buf[:G] == fill).all() and (buf[G + nbytes:] == fill).all(), (name, n, "a guard byte round the host record was written")
        got.append(buf[G:G + nbytes].copy())
        env.close()
    diff = np.flatnonzero(got[0] != got[1])
    assert diff.size == 0, (name, n, "bytes of the record were not written", diff[:8], len(got[0]))
