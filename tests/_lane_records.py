"""Canonical per-env records of the four record-lane env types (cge_records_<env>_*): the layout as include/cge_amd.h states it, a
pure-Python reader, and the bodies of tests/test_lane_records_cpu.py and tests/test_lane_records_gpu.py, which hand a type's name in.

A record: int32[8] header | the type's body words, padded to 16 bytes | 624 uint32 words per stream."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import _guard_bands as gb
import _lane_kit as kit
from conftest import ROOT

STREAM_WORDS, HEADER_BYTES, TAG = 624, 32, 0x4C520100
ENTRY_POINTS = ("state_bytes", "get_state", "set_state", "pack", "unpack")
KERNELS = ("11pack_kernel", "12check_kernel", "13unpack_kernel")
SIZES = (1, 63, 64, 65, 130, 4097)                  # a single lane, a partial wave, one wave, one lane more, waves; one env into a second staging round


def _spec(kind):
    import test_airline_gpu, test_emergency_gpu, test_farm_gpu, test_space_station_gpu
    return {"airline": test_airline_gpu, "emergency": test_emergency_gpu, "space_station": test_space_station_gpu, "farm": test_farm_gpu}[kind].SPEC


# per type: its number in the tag, the kinds of its streams in the record's order ("py": CPython, "np": NumPy legacy) with the model's
# attribute of each, the body words of the cursors, the steps that cross a generation boundary and end episodes (with the step limit
# that ends them: the counts of _lane_kit's kernel_equals_the_model, farm's a year), and two pokes (body word, shift, width, value) that
# put an index field out of range
TYPES = {
    "airline": types.SimpleNamespace(number=1, streams=(("py", "rng"),), cursors=(243,), steps=80, limit=None,
                                     pokes=((0, 0, 4, 15), (264 + 3, 27, 5, 25))),           # aircraft 0's airport 15; flight 3's aircraft 25
    "emergency": types.SimpleNamespace(number=2, streams=(("py", "rng"),), cursors=(199, 200), steps=120, limit=50,
                                       pokes=((60 + 2, 11, 5, 20), (170 + 24, 0, 5, 21))),   # unit 2's incident slot 20; 21 incidents
    "space_station": types.SimpleNamespace(number=3, streams=(("np", "rng"),), cursors=(185, 186), steps=60, limit=25,
                                           pokes=((178 + 6, 0, 5, 18), (178 + 6, 5, 5, 18))),   # orbit phase 18; angle 18
    "farm": types.SimpleNamespace(number=4, streams=(("np", "rng"), ("py", "py")), cursors=(202, 203, 204, 205), steps=365, limit=1,
                                  pokes=((178 + 4, 4, 4, 8), (178 + 8, 0, 4, 6))),           # field 1's stage 8; field 2's crop 5 (stored + 1)
}
KINDS = tuple(TYPES)
FARM_FLAGS, FARM_GAUSS = 178 + 21, 150 + 24         # farm: has_gauss is bit 2 of integer word 21; the cached value is float64 word 24 of the rest


def header_macros():
    src = open(os.path.join(ROOT, "include", "cge_amd.h")).read()
    return {k.lower(): int(v) for k, v in re.findall(r"CGE_([A-Z_]+)_RECORD_BYTES = (\d+)", src)}


def layout(kind):
    """the header's layout rule, from its CGE_<ENV>_RECORD_BYTES: every section padded to a multiple of 16 bytes"""
    body = header_macros()[kind]
    padded = -(-body // 16) * 16
    streams = len(TYPES[kind].streams)
    return types.SimpleNamespace(words=body // 4, body=HEADER_BYTES, padding=(HEADER_BYTES + body, HEADER_BYTES + padded), streams=HEADER_BYTES + padded,
                                 n_streams=streams, state_bytes=HEADER_BYTES + padded + streams * STREAM_WORDS * 4)


def parse(record):
    """one record (uint8) -> (header int32[8], body words uint32[REC_WORDS], [(words uint32[624], index)] per stream)"""
    record = np.ascontiguousarray(record, dtype=np.uint8)
    header = record[:HEADER_BYTES].view(np.int32)
    words, streams = int(header[1]), int(header[2])
    padded = -(-words * 4 // 16) * 16
    assert record.size == HEADER_BYTES + padded + streams * STREAM_WORDS * 4, "the sections do not add up to the record"
    body = record[HEADER_BYTES:HEADER_BYTES + 4 * words].view(np.uint32)
    at = HEADER_BYTES + padded
    return header, body, [(record[at + s * STREAM_WORDS * 4:at + (s + 1) * STREAM_WORDS * 4].view(np.uint32), int(header[3 + s])) for s in range(streams)]


def poke(rec, env, byte_offset, shift, width, value):
    """the `width`-bit field at `shift` of the 32-bit word at `byte_offset` of record `env` <- value (rec: uint8 [n, state_bytes], torch)"""
    w = rec[env, byte_offset:byte_offset + 4].cpu().numpy().view(np.uint32)
    w[0] = (int(w[0]) & ~(((1 << width) - 1) << shift) | value << shift) & 0xFFFFFFFF
    rec[env, byte_offset:byte_offset + 4] = torch.from_numpy(w.view(np.uint8)).to(rec.device)


def make(cge, kind, n, **kw):
    return kit.make(cge, _spec(kind), n, TYPES[kind].limit, autoreset_mode="SameStep", **kw)


def actions(kind, seed, k, n):
    return kit.dev(_spec(kind).m.hash_actions(seed, k, n))


def advanced(cge, kind, n, steps, seed=11, **kw):
    env = make(cge, kind, n, **kw)
    env.reset(seed=seed)
    env.rollout(steps, action_seed=3)
    return env


def columns(env, kind):
    """the handle's record columns uint32 [words, n], read from its snapshot (32-byte header, then the arrays: the columns first)"""
    words = layout(kind).words
    return env.snapshot()[32:32 + 4 * words * env.num_envs].view(np.uint32).reshape(words, env.num_envs)


# ---------------------------------------------------------------------------------------------------------------------- CPU
def abi_is_declared_exported_and_bound(kind):
    from custom_gymnasium_environments_amd import _native, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cge_amd.h")).read(), flags=re.S)
    prefix = f"cge_records_{kind}_"
    protos = {name: (ret, args) for ret, name, args in re.findall(r"^\s*(size_t|int)\s*(" + prefix + r"[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)}
    assert set(protos) == {prefix + fn for fn in ENTRY_POINTS}
    handle = f"cge_{kind} *h"
    want = {"state_bytes": ("size_t", [f"const {handle}"]), "get_state": ("int", [handle, "void *host_buf", "void *stream"]),
            "set_state": ("int", [handle, "const void *host_buf", "void *stream"]),
            "pack": ("int", [handle, "int64_t first", "int64_t count", "void *dev_records", "void *stream"]),
            "unpack": ("int", [handle, "int64_t first", "int64_t count", "const void *dev_records", "void *stream"])}
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    bound = {"state_bytes": (ctypes.c_size_t, [vp]), "get_state": (ctypes.c_int, [vp, vp, vp]), "set_state": (ctypes.c_int, [vp, vp, vp]),
             "pack": (ctypes.c_int, [vp, i64, i64, vp, vp]), "unpack": (ctypes.c_int, [vp, i64, i64, vp, vp])}
    L = ctypes.CDLL(build.build_native())
    for fn in ENTRY_POINTS:
        ret, args = protos[prefix + fn]
        assert (ret, [" ".join(a.split()) for a in args.split(",")]) == want[fn], fn
        assert _native.SIGNATURES[prefix + fn] == bound[fn], fn
        assert hasattr(L, prefix + fn), fn


def record_sizes_follow_the_layout_rule():
    assert {k: layout(k).state_bytes for k in KINDS} == {"airline": 4192, "emergency": 3344, "space_station": 3280, "farm": 5856}
    assert all(layout(k).state_bytes % 16 == 0 and layout(k).streams % 16 == 0 for k in KINDS)
    for k in KINDS:                                                 # the cursor words are the last scalar words the type's header names
        assert all(0 <= c < layout(k).words for c in TYPES[k].cursors) and len(TYPES[k].cursors) in (len(TYPES[k].streams), 2 * len(TYPES[k].streams))


def kernel_notes(tmp_path):
    """{mangled name: (vgprs, sgprs, scratch bytes, LDS bytes)} of the records kernels, read as tests/test_kernel_occupancy.py reads them"""
    from custom_gymnasium_environments_amd import build
    lib = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(build.build_native(), lib)
    subprocess.run([os.path.join(kit.LLVM, "llvm-objdump"), "--offloading", lib], cwd=str(tmp_path), check=True, capture_output=True)
    found = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(kit.LLVM, "llvm-readelf"), "--notes", os.path.join(str(tmp_path), f)], capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "3cge7records" in name:
                found[name] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                                    for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    return found


def no_records_kernel_uses_scratch(tmp_path):
    found = kernel_notes(tmp_path)
    for k in KERNELS:                                               # one instance per type, under the type's number and not its name
        assert sorted(n for n in found if k in n) == sorted(f"_ZN3cge7records{k}ILi{t.number}EEEvNS0_4ArgsE" + ("Py" if "check" in k else "") for t in TYPES.values()), sorted(found)
    assert all(v[2] == 0 for v in found.values()), found
    assert all(v[3] <= 32 * 1024 for v in found.values()), found   # the tile and one generator block: several workgroups a CU
    return found


def ready_marks_stay_within_the_export(kind):
    """pack takes back at most MT_EXPORT_MAX_AHEAD = 227 words of the next generation (the un-twist of word k reads word k + 397 of
    the current one).  A kernel of these types leaves a mark at most at the end of the 32-word chunk that holds word cursor + READY - 1
    (mt_make_ready), the cursor at most 623: ahead <= roundup32(623 + READY - 624 + 1).  Airline keeps no mark at all."""
    src = open(os.path.join(ROOT, "custom_gymnasium_environments_amd", "csrc", kind + ".hip")).read()
    ready = [int(v) for v in re.findall(r"constexpr uint32_t READY = (\d+);", src)]
    needs = re.findall(r"mt_make_ready\(([^;]*)\);", src)
    if kind == "airline":
        assert not ready and not needs and "MtStream rng(p.mt + li * MT_STRIDE, e.mt_pos, 0u)" in src
        return
    assert len(ready) == 1 and needs and all("READY" in call.split(",")[3] and call.count(",") == 4 for call in needs), needs   # no slack argument
    assert -(-(623 + ready[0] - 624 + 1) // 32) * 32 <= 624 - 397


def parse_reads_a_hand_made_record():
    words, streams = 5, 2                                           # five body words: 20 bytes, padded to 32
    rec = np.zeros(32 + 32 + streams * 624 * 4, np.uint8)
    rec[:32].view(np.int32)[:5] = [TAG | 9, words, streams, 17, 624]
    rec[32:52].view(np.uint32)[:] = [1, 2, 3, 4, 0xFFFFFFFF]
    rec[64:64 + 2496].view(np.uint32)[:] = np.arange(624)
    rec[64 + 2496:].view(np.uint32)[:] = np.arange(624) + 1000
    header, body, (s0, s1) = parse(rec)
    assert header.tolist() == [TAG | 9, 5, 2, 17, 624, 0, 0, 0] and body.tolist() == [1, 2, 3, 4, 0xFFFFFFFF]
    assert s0[1] == 17 and s1[1] == 624 and s0[0][5] == 5 and s1[0][623] == 1623 and s0[0].size == s1[0].size == 624
    with pytest.raises(AssertionError):
        parse(rec[:-16])


# ---------------------------------------------------------------------------------------------------------------------- GPU
def streams_are_the_references(cge, kind):
    """after a rollout that crosses generation boundaries and ends episodes, every env's stream words and index are its model's
    generator's (random.Random.getstate() / RandomState.get_state()), the low 31 bits of word 0 apart, and the body is the device's own
    columns with the cursor words zeroed"""
    spec, ty, n = _spec(kind), TYPES[kind], 65
    env = make(cge, kind, n, env_index0=1000)
    m = kit.model(spec, 21 + 1000 + np.arange(n), kit.SAME_STEP, ty.limit)
    kit.same(env.reset(seed=21)[0], m.reset(), "reset")
    acts = spec.m.hash_actions(5, ty.steps, n, env0=1000)
    _, _, dc = env.rollout(ty.steps, action_seed=5)
    ends = 0
    for t in range(ty.steps):
        ends += int(m.step(acts[t])[2].sum())
    assert ends >= n and int(dc.sum()) == ends                      # every env's episode ended at least once on average, and the device agrees
    rec, cols = env.get_state(), columns(env, kind)
    lay = layout(kind)
    assert rec.shape == (n, lay.state_bytes) and rec.dtype == np.uint8
    off_by_one = 0
    for i, e in enumerate(m.envs):
        header, body, streams = parse(rec[i])
        assert header.tolist()[:3] == [TAG | ty.number, lay.words, lay.n_streams] and not header[3 + lay.n_streams:].any(), i
        want = cols[:, i].copy()
        want[list(ty.cursors)] = 0
        assert np.array_equal(body, want), (i, "body")
        assert not rec[i, lay.padding[0]:lay.padding[1]].any(), (i, "padding")
        for (words, index), (form, attr) in zip(streams, ty.streams):
            if form == "py":
                state = getattr(e, attr).getstate()[1]
                ref, ref_index = np.array(state[:624], np.uint32), int(state[624])
            else:
                _, ref, ref_index, has_gauss, cached = getattr(e, attr).get_state()
                ref_index = int(ref_index)
                if kind == "farm":
                    assert (int(body[FARM_FLAGS]) >> 2) & 1 == has_gauss, (i, "has_gauss")
                    mine = body[FARM_GAUSS:FARM_GAUSS + 2].view(np.float64)[0]      # the device's own record word (compared with the columns above)
                    if has_gauss:
                        ulps = abs(int(np.float64(cached).view(np.int64)) - int(mine.view(np.int64)))
                        assert ulps <= 1, (i, cached, mine)         # the stated `log` caveat (README): one unit in the last place
                        off_by_one += ulps
                    else:
                        assert mine == 0.0
                else:
                    assert has_gauss == 0                           # the space station keeps no cache: a reset's sixteen polar pairs leave none
            assert index == ref_index, (i, attr, index, ref_index)
            ref = ref.copy()
            ref[0] &= 0x80000000
            assert np.array_equal(words, ref), (i, attr, "words")
    print(f"{kind}: {off_by_one} cached Gaussians of {n} differ from the model's by one unit in the last place")
    # the record continues the stream in the reference's own generator
    words, index = parse(rec[0])[2][0]
    if ty.streams[0][0] == "py":
        r = random.Random()
        r.setstate((3, tuple(int(w) for w in words) + (index,), None))
        assert [r.getrandbits(32) for _ in range(700)] == [getattr(m.envs[0], ty.streams[0][1]).getrandbits(32) for _ in range(700)]
    else:
        r = np.random.RandomState()
        r.set_state(("MT19937", words, index, 0, 0.0))
        assert np.array_equal(r.randint(0, 2 ** 32, 700, dtype=np.uint64), getattr(m.envs[0], ty.streams[0][1]).randint(0, 2 ** 32, 700, dtype=np.uint64))
    env.close()


def records_are_canonical(cge, kind, n):
    """get_state of an env and of a fresh env that took those records are the same bytes; so they are again after both have stepped on,
    the one with chunks twisted ahead and the other from a whole generation ready; the device form is the host form"""
    steps = TYPES[kind].steps if n <= 130 else 24
    env = advanced(cge, kind, n, steps)
    rec = env.get_state()
    fresh = make(cge, kind, n, env_index0=31)
    fresh.set_state(rec)
    assert np.array_equal(fresh.get_state(), rec)
    acts = actions(kind, 8, 20, n)
    for lo, hi in ((0, 2), (2, 20)):
        a, b = (e.rollout(hi - lo, actions=acts[lo:hi], trajectory=True, per_step=True) for e in (env, fresh))
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        if kind != "airline" and n >= 63 and lo == 0:
            # two steps on, the ready marks differ (airline keeps none): a whole generation ready here, chunks ahead of the cursor
            # there.  They meet again when the cursors wrap, which the eighteen further steps see to.
            marks = list(TYPES[kind].cursors[1::2])
            assert (columns(env, kind)[marks] != columns(fresh, kind)[marks]).any()
        rec = env.get_state()
        assert np.array_equal(fresh.get_state(), rec)
    dev = env.get_state(out="device")
    assert dev.device == env.device and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), rec)
    into = torch.zeros_like(dev)
    assert env.get_state(out=into) is into and torch.equal(into, dev)
    fresh.set_state(dev)                                            # a CUDA tensor goes in as a host array does
    assert np.array_equal(fresh.get_state(), rec)
    env.close(); fresh.close()


def _outputs(env, acts):
    out = env.rollout(acts.shape[0], actions=acts, trajectory=True, per_step=True)
    return list(out) + [env.info(f) for f in env.INFO_FIELDS]


def records_move(cge, kind):
    """records of 130 envs, permuted and with duplicates, into a handle of 200 envs with another env_index0, and through first= into the
    middle of a 4,097-env handle: forty steps of given actions give the source's rows [perm], outputs and info fields"""
    n, m, k = 130, 200, 40
    src = advanced(cge, kind, n, TYPES[kind].steps)
    rec = src.get_state(out="device")
    perm = torch.from_numpy(np.random.RandomState(3).randint(0, n, m)).to(rec.device)
    assert len(set(perm.tolist())) < m
    acts = actions(kind, 9, k, n)
    want = _outputs(src, acts)                                      # [traj, reward, flags] are [k, n, ...]; sums, counts and info [n]
    moved = rec[perm].contiguous()

    def check(got, rows, what):
        for j, (x, y) in enumerate(zip(got, want)):
            x = x[:, rows] if j < 3 else x[rows]
            y = y[:, perm] if j < 3 else y[perm]
            assert torch.equal(x, y), (what, j)

    dst = make(cge, kind, m, env_index0=7777)
    dst.set_state(moved)
    assert torch.equal(dst.get_state(out="device"), moved)
    check(_outputs(dst, acts[:, perm].contiguous()), slice(None), "a handle of 200")
    dst.close()

    big, first = advanced(cge, kind, 4097, 10, seed=5), 2000
    before = big.get_state(out="device")
    big.set_state(moved, first=first)
    after = big.get_state(out="device")
    assert torch.equal(after[first:first + m], moved) and torch.equal(after[:first], before[:first]) and torch.equal(after[first + m:], before[first + m:])
    assert torch.equal(big.get_state(out="device", first=first)[:m], moved) and np.array_equal(big.get_state(first=4096), after[4096:].cpu().numpy())
    big_acts = actions(kind, 10, k, 4097)
    big_acts[:, first:first + m] = acts[:, perm]
    check(_outputs(big, big_acts), slice(first, first + m), "the middle of 4,097")
    big.close(); src.close()


def refusals(cge, kind):
    """a refused record anywhere — env 0, env 64, the last of 4,097 — is a ValueError that names the env, and every env is as it was.
    Refused inputs on a path that validates them: no bad record reaches a step kernel."""
    ty, lay, n = TYPES[kind], layout(kind), 4097
    env = advanced(cge, kind, n, 12)
    rec = env.get_state(out="device")
    body = lambda w: HEADER_BYTES + 4 * w
    cases = [("tag", 0, 0, 8, 9), ("index 625", 12, 0, 10, 625), ("a cursor word", body(ty.cursors[0]), 0, 10, 5), ("a reserved header word", 28, 0, 1, 1),
             ("the word count", 4, 0, 10, lay.words + 1), ("the stream count", 8, 0, 2, 3)]
    if lay.padding[1] > lay.padding[0]:
        cases.append(("a padding byte", lay.padding[1] - 4, 24, 8, 1))
    if kind == "farm":
        cases.append(("the second index", 16, 0, 10, 700))
    cases += [(f"index field {j}", body(w), shift, width, value) for j, (w, shift, width, value) in enumerate(ty.pokes)]
    for what, offset, shift, width, value in cases:
        for at in (0, 64, n - 1):
            bad = rec.clone()
            poke(bad, at, offset, shift, width, value)
            poke(bad, n - 1, offset, shift, width, value)           # the LOWEST refused env is named
            with pytest.raises(ValueError, match=rf"cge_records_{kind}_unpack: env {at}: "):
                env.set_state(bad)
        assert torch.equal(env.get_state(out="device"), rec), what
    host = rec.cpu().numpy()
    w, shift, width, value = ty.pokes[0]
    bad = torch.from_numpy(host.copy())
    poke(bad, n - 1, body(w), shift, width, value)                  # in the host form's second round: the first must not have been unpacked
    fresh = make(cge, kind, n)
    mine = fresh.get_state()
    with pytest.raises(ValueError, match=rf"cge_records_{kind}_set_state: env {n - 1}: "):
        fresh.set_state(bad.numpy())
    assert np.array_equal(fresh.get_state(), mine)
    # arguments: shape, dtype, device, contiguity, alignment and range are ValueErrors before any call
    for wrong in (rec[:, :-16], rec.to(torch.int8), rec.cpu()[:, :8], rec[:, ::2], rec.view(-1)[16 - rec.data_ptr() % 16 + 1:][:lay.state_bytes].view(1, -1)):
        with pytest.raises(ValueError):
            env.set_state(wrong)
    with pytest.raises(ValueError):
        env.set_state(rec[:10], first=n - 5)
    with pytest.raises(ValueError):
        env.get_state(out=torch.zeros((3, lay.state_bytes), dtype=torch.uint8))
    assert env._fn("pack")(env._h, 0, n + 1, rec.data_ptr(), None) == -1 and b"range" in env._c_last_error(env._h)
    assert env._fn("unpack")(env._h, -1, 1, rec.data_ptr(), None) == -1 and env._fn("pack")(env._h, 0, 1, None, None) == -1
    assert env._fn("pack")(env._h, 0, 1, rec.data_ptr() + 8, None) == -1 and b"aligned" in env._c_last_error(env._h)
    assert torch.equal(env.get_state(out="device"), rec)
    env.close(); fresh.close()


def bounds(cge, kind):
    """guard bands round the device tensor and the host buffer, over two fills: nothing outside written, every byte inside written"""
    n, lay = 130, layout(kind)
    env = advanced(cge, kind, n, 30)
    arenas = []
    for fill in gb.FILLS:
        arena = gb.Arena.sized_for(fill, "cuda", [gb.request("records", (n, lay.state_bytes), torch.uint8)])
        view = arena.take("records", (n, lay.state_bytes), torch.uint8)
        arena.is_planted("records", env.get_state(out=view), "get_state(out=)")
        arena.outside_untouched(f"{kind} pack")
        arenas.append(arena)
    gb.written_everywhere(arenas[0], arenas[1], "records", what=f"{kind} pack")
    hosts = []
    for fill in gb.FILLS:                                           # the host form, called as the façade calls it, into a planted buffer
        guard = gb.guard_bytes(lay.state_bytes)
        buf = np.full(2 * guard + n * lay.state_bytes, fill, np.uint8)
        inner = buf[guard:guard + n * lay.state_bytes]
        env._check(env._fn("get_state")(env._h, inner.ctypes.data, env._stream()), "get_state")
        assert (buf[:guard] == fill).all() and (buf[guard + n * lay.state_bytes:] == fill).all(), "written outside the host buffer"
        hosts.append(inner.copy())
    assert np.array_equal(hosts[0], hosts[1]) and np.array_equal(hosts[0].reshape(n, -1), arenas[0].views["records"].cpu().numpy())
    env.close()


def existing_entry_points_are_unchanged(cge, kind):
    n, lay = 200, layout(kind)
    env = advanced(cge, kind, n, 30)
    bytes_before = int(env._fn("device_bytes")(env._h))
    assert bytes_before == n * (lay.words * 4 + lay.n_streams * 640 * 4) + 8          # the columns, a block per stream, the error counter
    rec = env.get_state(out="device")
    env.set_state(rec[torch.arange(n - 1, -1, -1, device=rec.device)].contiguous())
    env.get_state()
    assert int(env._fn("device_bytes")(env._h)) == bytes_before
    snap = env.snapshot()
    assert snap.shape == (32 + bytes_before - 8,)
    fresh = make(cge, kind, n)
    fresh.restore(snap)
    assert np.array_equal(fresh.snapshot(), snap) and np.array_equal(fresh.get_state(), env.get_state())
    acts = actions(kind, 2, 10, n)
    assert all(torch.equal(x, y) for x, y in zip(_outputs(env, acts), _outputs(fresh, acts)))
    env.close(); fresh.close()
