"""Would the guard bands of tests/_guard_bands.py report a kernel that writes where it should not, or leaves a byte unwritten?  (No GPU.)

tests/test_output_bounds_gpu.py only ever sees the checks pass.  Here the arena lives in host memory and the "kernel" is a few lines of
torch: a clean write must pass; one byte in front of a view, one behind it, one in the guard between two views and one inside a
restricted region must each fail `outside_untouched` with a message that names the neighbouring output; one byte left unwritten must fail
`written_everywhere`; `take` must honour `align` and `skew`; and a façade that hands out another tensor than the planted one must fail
`is_planted`."""
import types

import pytest
import torch

from _guard_bands import FILLS, Arena, guard_bytes, output_requests, plant, plane_byte_mask, request, written_everywhere

N, W = 65, 9                                                              # a wave and one lane; rows of 36 bytes


def kernel(views, skip=None):
    """a clean "kernel": every element of every output written from a counter (deterministic, as the project's outputs are)"""
    for j, (name, v) in enumerate(views.items()):
        flat = v.view(-1)
        vals = (torch.arange(flat.numel()) * 7 + j) % 120 + 1
        vals = vals > 60 if v.dtype == torch.bool else vals.to(v.dtype)
        if skip is not None and skip[0] == name:
            keep = torch.ones(flat.numel(), dtype=torch.bool)
            keep[skip[1]] = False
            flat[keep] = vals[keep]
        else:
            flat.copy_(vals)


REQUESTS = [request("obs", (N, W), torch.float32), request("reward", (N,), torch.float32), request("terminated", (N,), torch.bool)]


def arenas(requests=REQUESTS):
    out = []
    for fill in FILLS:
        a = Arena.sized_for(fill, "cpu", requests)
        out.append((a, a.take_all(requests)))
    return out


def test_a_clean_write_passes():
    (a, va), (b, vb) = arenas()
    kernel(va); kernel(vb)
    a.outside_untouched(); b.outside_untouched()
    for name in va:
        assert written_everywhere(a, b, name) == va[name].numel() * va[name].element_size()
    assert written_everywhere(a, b, "obs", rows=[0, 64]) == 2 * W * 4


def test_guards_are_a_wave_wide_and_at_least_256_bytes():
    assert guard_bytes(1) == 256 and guard_bytes(4) == 256 and guard_bytes(36) == 2304 and guard_bytes(225) == 14592
    a, v = arenas()[0]
    assert a.guards == {"obs": 64 * 36, "reward": 256, "terminated": 256}
    (s0, e0), (s1, e1), (s2, e2) = (a.spans[k] for k in ("obs", "reward", "terminated"))
    assert s0 - a.base >= a.guards["obs"] and s1 - e0 >= a.guards["obs"] + a.guards["reward"] and s2 - e1 >= 512 and a.end - e2 == 256
    assert not a.owned[:s0].any() and a.owned[s0:e0].all() and not a.owned[e0:s1].any() and not a.owned[e2:].any()


@pytest.mark.parametrize("where, text", [("before", "1 byte(s) before obs"), ("after", "1 byte(s) behind obs"),
                                         ("between", "byte(s) before reward"), ("far", "byte(s) behind terminated")])
def test_one_byte_outside_a_view_fails(where, text):
    a, v = arenas()[0]
    kernel(v)
    s, e = a.spans["obs"]
    at = {"before": s - 1, "after": e, "between": a.spans["reward"][0] - 200, "far": a.spans["terminated"][1] + 255}[where]
    a.buf[at] = a.fill ^ 0xFF
    with pytest.raises(AssertionError, match="1 byte.s. outside the outputs were written") as err:
        a.outside_untouched(where)
    assert text in str(err.value) and f"offset {at - a.base}," in str(err.value)


def test_a_byte_that_happens_to_hold_the_fill_is_why_there_are_two_fills():
    (a, va), (b, vb) = arenas()
    a.buf[a.spans["obs"][1]], b.buf[b.spans["obs"][1]] = 0x7F, 0x7F                                      # the overrun writes 0x7F: invisible over the first fill only
    a.outside_untouched()
    with pytest.raises(AssertionError, match="behind obs"):
        b.outside_untouched()


def test_one_byte_in_a_restricted_region_fails():
    """world builder's padding between planes, the stride padding of a trajectory, slots at or above a segment's count"""
    planes = (("grid", (3, 3), torch.int8, 0), ("resources", (4,), torch.float32, 592))      # 65 * 9 = 585 bytes, then 7 of padding
    slab = 592 + N * 16
    req = [request("obs", (slab,), torch.uint8, row_bytes=25)]
    (a, va), (b, vb) = arenas(req)
    mask = plane_byte_mask(planes, N, slab, 1)
    assert int((~mask).sum()) == 7 and not mask[585:592].any()
    for ar, v in ((a, va), (b, vb)):
        ar.restrict("obs", mask)
        v["obs"][:585] = 1
        v["obs"][592:] = 2
        ar.outside_untouched()
    assert written_everywhere(a, b, "obs") == slab - 7
    assert written_everywhere(a, b, "obs", mask=plane_byte_mask(planes, N, slab, 1, rows=torch.arange(N) == 3)) == 25
    va["obs"][590] = 1
    with pytest.raises(AssertionError, match=r"inside obs at byte 590 \(restricted\)"):
        a.outside_untouched()


@pytest.mark.parametrize("name, element", [("obs", N * W - 1), ("obs", 0), ("reward", 63), ("terminated", 64)])
def test_one_unwritten_byte_fails(name, element):
    (a, va), (b, vb) = arenas()
    kernel(va, skip=(name, element)); kernel(vb, skip=(name, element))
    a.outside_untouched(); b.outside_untouched()                          # nothing out of bounds: only the second check sees it
    item = va[name].element_size()
    with pytest.raises(AssertionError, match=f"{item} byte.s. of {name} were not written") as err:
        written_everywhere(a, b, name)
    assert str(element * item) in str(err.value)
    for other in va:
        if other != name:
            written_everywhere(a, b, other)
    if name == "obs":                                                     # and the claim can be narrowed to rows
        row = element // W
        written_everywhere(a, b, "obs", rows=[r for r in range(N) if r != row])
        with pytest.raises(AssertionError):
            written_everywhere(a, b, "obs", rows=[row])


def test_take_honours_align_and_skew():
    a = Arena(0x7F, "cpu", 1 << 16)
    base = a.buf.data_ptr() + a.base
    assert base % 4096 == 0
    v = a.take("a", (63, 15, 15), torch.int8, align=16, skew=1)
    assert v.data_ptr() % 16 == 1 and tuple(v.shape) == (63, 15, 15) and v.dtype == torch.int8
    w = a.take("b", (7,), torch.float32, align=16, skew=4)
    assert w.data_ptr() % 16 == 4
    x = a.take("c", (5,), torch.float64, align=256)
    assert x.data_ptr() % 256 == 0
    y = a.take("d", (3,), torch.int32, align=4096, skew=8)
    assert y.data_ptr() % 4096 == 8
    with pytest.raises(AssertionError):
        a.take("e", (3,), torch.int32, skew=2)                            # an int at an odd half-word: no typed view exists
    with pytest.raises(AssertionError, match="too small"):
        a.take("f", (1 << 16,), torch.uint8)
    ptr = a.buf.data_ptr()
    assert a.buf.data_ptr() == ptr and int(a.owned.sum()) == 63 * 225 + 28 + 40 + 12     # no take reallocated


class Facade:
    """the part of DeviceVectorEnv that plant() and output_requests() read, with its `_out`"""
    _flags, _obs_dtype, _reward_sum_dtype, _ep_ret, _reuse = "both", torch.float32, torch.float64, None, True

    def __init__(self, honest):
        self.num_envs, self._obs_shape, self._bufs, self.honest = N, (N, W), {}, honest
        self.autoreset_mode = types.SimpleNamespace(name="SAME_STEP")

    def _out(self, key, shape, dtype):
        t = self._bufs.get(key)
        if self.honest and t is not None and tuple(t.shape) == tuple(shape) and t.dtype == dtype:
            return t
        return torch.empty(shape, dtype=dtype)                            # a later change that allocates afresh: the guards guard nothing


def test_a_planted_tensor_that_is_silently_replaced_fails():
    for honest in (True, False):
        env = Facade(honest)
        req = output_requests(env, ("obs", "reward", "terminated", "truncated", "final_obs", "done"))
        assert [r[0] for r in req] == ["obs", "reward", "terminated", "truncated", "final_obs", "done"]
        a = Arena.sized_for(0x7F, "cpu", req)
        views = plant(env, a, req)
        assert set(env._bufs) == set(views)
        got = env._out("obs", (N, W), torch.float32)
        if honest:
            a.is_planted("obs", got)
        else:
            with pytest.raises(AssertionError, match="did not return the planted obs"):
                a.is_planted("obs", got)
    with pytest.raises(AssertionError, match="did not return the planted reward"):
        a.is_planted("reward", views["obs"])                              # another planted tensor is not the one either


def test_requests_follow_the_type():
    env = Facade(True)
    env._flags, env.autoreset_mode = "terminated", types.SimpleNamespace(name="NEXT_STEP")
    assert [r[0] for r in output_requests(env, ("obs", "reward", "terminated", "truncated", "final_obs", "done"))] == ["obs", "reward", "terminated"]
    req = {r[0]: r for r in output_requests(env, ("traj", "reward_sum", "done_count", "reward_traj", "flags_traj"), k=5)}
    assert req["traj"][1] == (5, N, W) and req["traj"][5] == W * 4 and req["flags_traj"][2] == torch.bool and req["reward_sum"][2] == torch.float64


def test_a_refilled_output_shows_what_the_next_call_left_out():
    """what an earlier call wrote must not vouch for a later one: `reset` fills the view again (and owns it whole again), so a second
    "call" that skips a byte the first one wrote is found"""
    (a, va), (b, vb) = arenas()
    kernel(va); kernel(vb)
    kernel(va, skip=("obs", 5)); kernel(vb, skip=("obs", 5))             # without a refill the first call's byte hides the gap
    written_everywhere(a, b, "obs")
    for ar in (a, b):
        ar.restrict("obs", torch.zeros(N * W * 4, dtype=torch.bool))
        ar.reset("obs")
        assert bool((ar.bytes_of("obs") == ar.fill).all()) and bool(ar.owned_bytes("obs").all())
    kernel(va, skip=("obs", 5)); kernel(vb, skip=("obs", 5))
    with pytest.raises(AssertionError, match="4 byte.s. of obs were not written"):
        written_everywhere(a, b, "obs")
