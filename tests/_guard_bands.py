"""Guard bands round kernel outputs: WHERE a call wrote, next to the value comparisons of the rest of the suite.

All outputs of one call are carved from one allocation, the Arena, which is pre-filled with one byte value.  Every view has a guard band
of that fill in front of it and behind it; the arena knows which bytes it handed out (`owned`, narrowed by `restrict`).  Two checks:

  arena.outside_untouched()               every byte outside `owned` still holds the fill: nothing was written out of bounds
  written_everywhere(a, b, name, ...)     two arenas that hold the SAME calls over the fills 0x7F and 0x80 agree in the owned bytes of
                                          `name`: an unwritten byte would hold 0x7F in one and 0x80 in the other, so equality proves that
                                          the byte was written, with no tolerance and no knowledge of the value (the outputs are
                                          deterministic from the seeds, which the bit-exact suites establish)

A guard is as wide as what one wavefront writes to that output in one step (64 rows of it), rounded up to 256 bytes and never less:
every store pass of the project is at most wave-wide, so a pass that is off by up to a whole wave's share lands in memory the test owns.

Everything here works on CPU tensors as well as on the device (tests/test_guard_bands_cpu.py shows that the checks detect)."""
import numpy as np
import torch

FILLS = (0x7F, 0x80)
WAVE = 64


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _up(x, m):
    return -(-int(x) // m) * m


def guard_bytes(row_bytes):
    return max(256, _up(WAVE * int(row_bytes), 256))


def request(name, shape, dtype, align=16, skew=0, row_bytes=None):
    """What `take` takes, as a tuple: lists of these size an arena before it is allocated (`Arena.sized_for`)."""
    return (name, tuple(int(s) for s in shape), dtype, int(align), int(skew), row_bytes)


def _row_bytes(shape, dtype, row_bytes):
    if row_bytes is not None:
        return int(row_bytes)
    return int(np.prod(shape[1:], dtype=np.int64)) * _itemsize(dtype)             # a [N, ...] output: one env's share; a [N] one: an element


class Arena:
    """One uint8 tensor pre-filled with the byte `fill`, from which `take` carves typed views with guard bands round them.  It is
    allocated once, with `capacity` bytes (`Arena.sized_for` works the capacity out from the requests): no `take` reallocates."""

    def __init__(self, fill, device, capacity=1 << 20):
        self.fill, self.device = int(fill), torch.device(device)
        self.buf = torch.full((int(capacity) + 4096,), self.fill, dtype=torch.uint8, device=self.device)
        self.base = (-self.buf.data_ptr()) % 4096                                   # offsets are counted from a 4096-byte boundary
        self.owned = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.device)
        self.views, self.spans, self.guards = {}, {}, {}
        self.end = self.base                                                        # the first byte behind the last guard

    @classmethod
    def sized_for(cls, fill, device, requests):
        need = 0
        for name, shape, dtype, align, skew, row_bytes in requests:
            nbytes = int(np.prod(shape, dtype=np.int64)) * _itemsize(dtype)
            need += 2 * guard_bytes(_row_bytes(shape, dtype, row_bytes)) + nbytes + max(align, 16) + skew + 16
        return cls(fill, device, need)

    def take(self, name, shape, dtype, align=16, skew=0, row_bytes=None):
        """A view of `shape` and `dtype` whose first byte lies at a multiple of `align` plus `skew` bytes."""
        assert name not in self.views, name
        shape = tuple(int(s) for s in shape)
        item = _itemsize(dtype)
        assert skew % item == 0, "a typed view starts at a multiple of its element size"
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        g = guard_bytes(_row_bytes(shape, dtype, row_bytes))
        start = self.base + _up(self.end - self.base + g, max(int(align), item)) + int(skew)
        stop = start + nbytes
        assert stop + g <= self.buf.numel(), f"the arena is too small for {name}: size it with Arena.sized_for"
        view = self.buf[start:stop].view(dtype).view(shape)
        assert (view.data_ptr() - skew) % align == 0 and view.data_ptr() == self.buf.data_ptr() + start
        self.owned[start:stop] = True
        self.views[name], self.spans[name], self.guards[name] = view, (start, stop), g
        self.end = stop + g
        return view

    def take_all(self, requests):
        return {r[0]: self.take(*r) for r in requests}

    def restrict(self, name, byte_mask):
        """Narrow what counts as owned inside `name`: `byte_mask` is a bool per byte of the view (padding between planes or steps, unused
        slots).  Masks of several calls are ANDed."""
        start, stop = self.spans[name]
        m = torch.as_tensor(byte_mask, dtype=torch.bool).to(self.device).reshape(-1)
        assert m.numel() == stop - start, (name, m.numel(), stop - start)
        self.owned[start:stop] &= m

    def reset(self, name):
        """Before the next call: `name` holds the fill again and is owned whole again."""
        start, stop = self.spans[name]
        self.buf[start:stop] = self.fill
        self.owned[start:stop] = True

    def owned_bytes(self, name):
        start, stop = self.spans[name]
        return self.owned[start:stop]

    def bytes_of(self, name):
        start, stop = self.spans[name]
        return self.buf[start:stop]

    def _near(self, offset):
        best = min(self.spans, key=lambda k: min(abs(offset - self.spans[k][0]), abs(offset - (self.spans[k][1] - 1))))
        start, stop = self.spans[best]
        if offset < start:
            return f"{start - offset} byte(s) before {best}"
        if offset >= stop:
            return f"{offset - stop + 1} byte(s) behind {best}"
        return f"inside {best} at byte {offset - start} (restricted)"

    def outside_untouched(self, what=""):
        """Every byte outside `owned` still equals the fill.  One comparison on the device against the mask, one synchronisation."""
        bad = (self.buf != self.fill) & ~self.owned
        count = int(bad.sum())
        if count:
            offs = torch.nonzero(bad).flatten()[:8].tolist()
            raise AssertionError(f"{what}: {count} byte(s) outside the outputs were written (fill {self.fill:#x}): "
                                 + "; ".join(f"offset {o - self.base}, {self._near(o)}" for o in offs))

    def is_planted(self, name, tensor, what=""):
        """`tensor`, which a call returned, IS the arena's view `name` (or, for a shorter rollout, the front of it)."""
        view = self.views[name]
        assert isinstance(tensor, torch.Tensor) and tensor.data_ptr() == view.data_ptr() and tensor.dtype == view.dtype and tensor.numel() <= view.numel(), \
            f"{what}: the call did not return the planted {name}: the guards round it guard nothing"


def written_everywhere(arena_a, arena_b, name, rows=None, mask=None, what=""):
    """The owned bytes of `name` are equal in the two arenas (the same calls over two fills), so every one of them was written.  `rows`
    (bool or indices over the view's leading dimension) or `mask` (a bool per byte of the view) narrows the claim."""
    assert arena_a.fill != arena_b.fill
    oa, ob = arena_a.owned_bytes(name), arena_b.owned_bytes(name)
    assert torch.equal(oa, ob.to(oa.device)), f"{what}: the two runs own different bytes of {name}"
    sel = oa.clone()
    if mask is not None:
        sel &= torch.as_tensor(mask, dtype=torch.bool).to(sel.device).reshape(-1)
    if rows is not None:
        lead = arena_a.views[name].shape[0]
        r = torch.zeros(lead, dtype=torch.bool, device=sel.device)
        r[torch.as_tensor(rows).to(sel.device)] = True
        sel &= r[:, None].expand(lead, sel.numel() // lead).reshape(-1)
    a, b = arena_a.bytes_of(name), arena_b.bytes_of(name).to(arena_a.device)
    diff = (a != b) & sel
    count = int(diff.sum())
    if count:
        offs = torch.nonzero(diff).flatten()[:8].tolist()
        raise AssertionError(f"{what}: {count} byte(s) of {name} were not written (they differ between the fills): byte offsets {offs} "
                             f"of {a.numel()}, view shape {tuple(arena_a.views[name].shape)}")
    return int(sel.sum())


# ---------------------------------------------------------------------------------------------------------------- planting
STEP_KEYS = ("obs", "reward", "terminated", "truncated", "final_obs", "done")
ROLLOUT_KEYS = ("traj", "reward_sum", "done_count", "reward_traj", "flags_traj")


def output_requests(env, keys, k=None):
    """The requests for the outputs `keys` of `env` as DeviceVectorEnv asks `_out` for them (`k`: the steps of a rollout).  Keys the type
    does not write (`truncated` of a type that only terminates, `done` where the façade registers none, `final_obs` outside SameStep) are
    left out."""
    n, flags = env.num_envs, env._flags
    obs_item = _itemsize(env._obs_dtype)
    obs_row = int(np.prod(env._obs_shape, dtype=np.int64)) * obs_item // n          # one env's share of a step, for a slab too
    same = env.autoreset_mode.name == "SAME_STEP"
    out = []
    for key in keys:
        if key == "obs" or (key == "final_obs" and same):
            out.append(request(key, env._obs_shape, env._obs_dtype, row_bytes=obs_row))
        elif key == "traj":
            out.append(request(key, (k,) + tuple(env._obs_shape), env._obs_dtype, row_bytes=obs_row))
        elif key == "rgb":
            out.append(request(key, tuple(env._obs_shape) + (3,), torch.uint8))
        elif key == "reward":
            out.append(request(key, (n,), torch.float32))
        elif key == "terminated" or (key == "truncated" and flags != "terminated"):
            out.append(request(key, (n,), torch.bool))
        elif key == "done" and flags == "both" and (same or env._ep_ret is not None):
            out.append(request(key, (n,), torch.bool))
        elif key == "reward_sum":
            out.append(request(key, (n,), env._reward_sum_dtype))
        elif key == "done_count":
            out.append(request(key, (n,), torch.int32))
        elif key == "reward_traj":
            out.append(request(key, (k, n), torch.float32, row_bytes=4))
        elif key == "flags_traj":
            out.append(request(key, (k, n), torch.uint8 if flags == "both" else torch.bool, row_bytes=1))
        else:
            assert key in STEP_KEYS + ROLLOUT_KEYS, key
    return out


def plant(env, arena, requests):
    """Put arena views into `env._bufs` under the façade's keys (an env created with reuse_buffers=True: `_out` hands a planted tensor
    back when shape and dtype match).  -> {key: view}.  After every call the test asserts `arena.is_planted(key, returned)`."""
    assert env._reuse, "plant() needs reuse_buffers=True"
    views = {}
    for r in requests:
        views[r[0]] = env._bufs[r[0]] = arena.take(*r)
    return views


def stats_requests(env):
    return [request("ep_ret", (env.num_envs,), torch.float64), request("ep_len", (env.num_envs,), torch.int32)]


def register_stats(env, arena):
    """The episode-statistics pair of an env created with record_episode_statistics=True, re-registered on arena views."""
    assert env._ep_ret is not None
    torch.cuda.current_stream(env.device).synchronize()
    env._ep_ret, env._ep_len = (arena.take(*r) for r in stats_requests(env))
    assert env._fn("episode_stats")(env._h, env._ep_ret.data_ptr(), env._ep_len.data_ptr()) == 0
    return env._ep_ret, env._ep_len


def final_rows_requests(env):
    """rows / index / count of a `collect_final_obs` that has been called, as requests"""
    rows, index, count, cap = env._fin
    row = rows.numel() * rows.element_size() // index.numel()
    return [request("rows", rows.shape, rows.dtype, row_bytes=row), request("index", index.shape, index.dtype), request("count", count.shape, count.dtype)]


def register_final_rows(env, arena):
    """Re-register the terminal rows, their index and the counts of `collect_final_obs` on arena views (rows 16-byte aligned)."""
    _, _, _, cap = env._fin
    rows, index, count = (arena.take(*r) for r in final_rows_requests(env))
    assert env._fn("rollout_final_obs")(env._h, rows.data_ptr(), index.data_ptr(), cap, count.data_ptr()) == 0
    env._fin = (rows, index, count, cap)
    return rows, index, count


# the rows slab alone inside a plain allocation: tests/test_slab_final_rows_gpu.py::test_nothing_but_the_delivered_rows_is_written
GUARD = 64


def register_guarded(env, fill):
    """Re-register the rows slab inside a larger allocation filled with `fill` bytes: GUARD bytes in front, GUARD behind.  -> the allocation"""
    rows, index, count, cap = env._fin
    nbytes = rows.numel() * rows.element_size()
    big = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    inner = big[GUARD:GUARD + nbytes].view(rows.dtype)
    assert env._fn("rollout_final_obs")(env._h, inner.data_ptr(), index.data_ptr(), cap, count.data_ptr()) == 0
    env._fin = (inner, index, count, cap)
    return big


# ---------------------------------------------------------------------------------------------------------------- slabs
def plane_byte_mask(planes, num_envs, slab_bytes, slab_item, rows=None):
    """bool per byte of one observation slab (a _slab plane table: key, per-env shape, dtype, offset in slab elements): True inside the
    planes — of the envs `rows` only (bool [num_envs]) — and False in the padding between them."""
    mask = torch.zeros(int(slab_bytes), dtype=torch.bool)
    rows = None if rows is None else torch.as_tensor(rows, dtype=torch.bool).cpu()
    for key, shape, dtype, off in planes:
        rb = int(np.prod(shape, dtype=np.int64)) * _itemsize(dtype)
        a = off * slab_item
        plane = mask[a:a + num_envs * rb].view(num_envs, rb)
        if rows is None:
            plane[:] = True
        else:
            plane[rows] = True
    return mask
