"""The snapshot pack kernel and its slots through the C ABI (csrc/beat_snap.hip, include/beat_hip.h: beat_snap_*): frames bit for bit
against the NumPy slice ``a[lo_z:hi_z:s_z, lo_y:hi_y:s_y, lo_x:hi_x:s_x]`` of fields whose ghost planes hold NaN, the statistics
against NumPy's over the tissue nodes of the box, the order of the two streams, the slots and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL, EBUSY = -1, -5
SHAPES = [(2,), (65,), (130,), (63, 5), (65, 2), (64, 3, 2), (65, 7, 5), (130, 9, 4)]
STRIDES = [1, 2, 3, "mixed"]
MIXED = (3, 1, 2)


def _pad(v, fill):
    return list(v) + [fill] * (3 - len(v))


def _i64x3(v):
    return (C.c_int64 * 3)(*v)


class Snap:
    """One beat_snap: geometry per used axis, x first."""

    def __init__(self, ctx, shape, lo=None, hi=None, stride=1, dtype=np.float64, nfields=1, depth=1, mask=None, fill=float("nan"),
                 flags=1):
        from beat import _hip

        dim = len(shape)
        self.ctx, self.lib, self.nfields = ctx, ctx.lib, nfields
        self.lo = list(lo) if lo is not None else [0] * dim
        self.hi = list(hi) if hi is not None else list(shape)
        self.stride = [stride] * dim if np.ndim(stride) == 0 else list(stride)
        self.dtype = np.dtype(dtype)
        self.mask = None if mask is None else ctx.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8).ravel())
        self.handle = C.c_void_p()
        _hip.check(self.lib.beat_snap_create(ctx.handle, _i64x3(_pad(shape, 1)), _i64x3(_pad(self.lo, 0)), _i64x3(_pad(self.hi, 1)),
                                             _i64x3(_pad(self.stride, 1)), 1 if self.dtype == np.float32 else 0, nfields, depth,
                                             None if self.mask is None else self.mask.data_ptr(), fill, flags, C.byref(self.handle)))
        info = (C.c_int64 * 6)()
        _hip.check(self.lib.beat_snap_info(self.handle, info))
        self.frame_shape = (info[2], info[1], info[0])
        self.field_bytes = info[3]
        assert self.field_bytes == info[0] * info[1] * info[2] * self.dtype.itemsize

    def slices(self):
        s = [slice(a, b, c) for a, b, c in zip(_pad(self.lo, 0), _pad(self.hi, 1), _pad(self.stride, 1))]
        return tuple(reversed(s))

    def box(self):
        return tuple(reversed([slice(a, b) for a, b in zip(_pad(self.lo, 0), _pad(self.hi, 1))]))

    def enqueue(self, fields):
        ptrs = (C.c_void_p * len(fields))(*[f.ptr.value for f in fields])
        slot = C.c_int(-7)
        rc = self.lib.beat_snap_enqueue(self.handle, ptrs, C.byref(slot))
        return rc, slot.value

    def wait(self, slot):
        """(frames (nfields, nz_s, ny_s, nx_s) copied out of the slot, stats (nfields, 3))"""
        from beat import _hip

        host, stats = C.c_void_p(), (C.c_double * (3 * self.nfields))()
        _hip.check(self.lib.beat_snap_wait(self.handle, slot, C.byref(host), stats))
        raw = np.ctypeslib.as_array((C.c_ubyte * (self.nfields * self.field_bytes)).from_address(host.value))
        return raw.view(self.dtype).reshape((self.nfields,) + self.frame_shape).copy(), np.array(stats).reshape(self.nfields, 3)

    def release(self, slot):
        return self.lib.beat_snap_release(self.handle, slot)

    def take(self, fields):
        from beat import _hip

        rc, slot = self.enqueue(fields)
        _hip.check(rc)
        out = self.wait(slot)
        _hip.check(self.release(slot))
        return out

    def destroy(self):
        from beat import _hip

        _hip.check(self.lib.beat_snap_destroy(self.handle))


@functools.lru_cache(maxsize=None)
def _values(shape, seed=0):
    """Arbitrary finite values, (nz, ny, nx); on grids of some size also what fp32 rounds at a tie, overflows, holds as a subnormal
    and flushes to zero."""
    rng = np.random.default_rng(1000 * len(shape) + shape[0] + seed)
    n3 = tuple(reversed(_pad(shape, 1)))
    a = rng.standard_normal(n3) * 10.0 ** rng.integers(-3, 4, n3)
    flat = a.reshape(-1)
    if flat.size >= 64:
        where = rng.choice(flat.size, 5, replace=False)
        flat[where] = [1.0 + 2.0 ** -24, 1.0e39, -1.0e39, 1.0e-40, 1.0e-46]
    a.setflags(write=False)
    return a


def _as(a, dtype):
    with np.errstate(over="ignore", under="ignore"):
        return a.astype(dtype)


def _field(ctx, shape, values):
    """A field as the PDE lays it out: an xy plane of ghosts on either side, here NaN."""
    n3 = _pad(shape, 1)
    f = ctx.field(n3[0] * n3[1] * n3[2], n3[0] * n3[1])
    f.buf.fill_(float("nan"))
    f.set(np.asarray(values).ravel())
    return f


def _boxes(shape):
    whole = ([0] * len(shape), list(shape))
    interior = ([min(1, n - 1) for n in shape], [max(n - 1, min(1, n - 1) + 1) for n in shape])
    single = ([n // 2 for n in shape], [n // 2 + 1 for n in shape])
    return {"whole": whole, "interior": interior, "single": single}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frames_equal_the_numpy_slice(hip_ctx, shape, dtype):
    """Strides 1, 2, 3 and mixed, the whole grid, an interior box and a single node: frames bit-equal (fp32: to .astype(float32)),
    min and max bit-equal to NumPy's over the box, nothing non-finite although every ghost plane is NaN."""
    a = _values(shape)
    f = _field(hip_ctx, shape, a)
    for stride in STRIDES:
        st = MIXED[: len(shape)] if stride == "mixed" else stride
        for name, (lo, hi) in _boxes(shape).items():
            snap = Snap(hip_ctx, shape, lo, hi, st, dtype)
            frames, stats = snap.take([f])
            snap.destroy()
            want = _as(a[snap.slices()], dtype)
            assert _same_bits(frames[0], want), (shape, stride, name)
            box = a[snap.box()]
            assert stats[0, 0] == box.min() and stats[0, 1] == box.max() and stats[0, 2] == 0, (shape, stride, name, stats)


@pytest.mark.parametrize("shape", [(130,), (63, 5), (65, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_mask_fill_and_statistics(hip_ctx, shape):
    """With a mask: masked samples equal ``fill`` (NaN as NaN, and a number), min / max are NumPy's over the tissue nodes of the box --
    all of them, not the sampled ones --, nonfinite counts NaN and both infinities at tissue nodes, and a NaN at a masked node
    changes nothing."""
    a = _values(shape, seed=1).copy()
    rng = np.random.default_rng(5)
    mask = rng.random(a.shape) < 0.7
    lo, hi = _boxes(shape)["interior"]
    for fill, stride in ((float("nan"), 2), (-1234.5, MIXED[: len(shape)])):
        snap = Snap(hip_ctx, shape, lo, hi, stride, np.float64, mask=mask, fill=fill)
        box, mbox = a[snap.box()], mask[snap.box()]
        assert mbox.any() and not mbox.all()
        frames, stats = snap.take([_field(hip_ctx, shape, a)])
        want = np.where(mask[snap.slices()], a[snap.slices()], fill)
        assert _same_bits(frames[0], want)
        assert stats[0, 0] == box[mbox].min() and stats[0, 1] == box[mbox].max() and stats[0, 2] == 0
        # the extremes sit at nodes off the lattice: the statistics cover the box, not the frame
        b = a.copy()
        inside = np.argwhere(mbox) + np.array([s.start for s in snap.box()])
        off = [tuple(p) for p in inside if any((p[k] - snap.box()[k].start) % _pad(snap.stride, 1)[2 - k] for k in range(3))]
        if off:
            b[off[0]] = 1.0e300
            _, s2 = snap.take([_field(hip_ctx, shape, b)])
            assert s2[0, 1] == 1.0e300 and s2[0, 0] == stats[0, 0]
        # NaN and the infinities at tissue nodes are counted; the infinities are the extremes, NaN is none
        tissue = [tuple(p) for p in inside]
        c = a.copy()
        special = [np.nan, np.inf, -np.inf, np.nan][: len(tissue)]
        for p, v in zip(tissue, special):
            c[p] = v
        frames3, s3 = snap.take([_field(hip_ctx, shape, c)])
        assert s3[0, 2] == len(special)
        sel = c[snap.box()][mbox]
        assert np.isnan(sel).any()
        if len(special) >= 3:
            assert s3[0, 0] == -np.inf and s3[0, 1] == np.inf
        assert _same_bits(frames3[0], np.where(mask[snap.slices()], c[snap.slices()], fill))
        # a NaN at a masked node of the box changes neither the frame nor the statistics
        d = a.copy()
        d[tuple((np.argwhere(~mbox) + np.array([s.start for s in snap.box()]))[0])] = np.nan
        frames4, s4 = snap.take([_field(hip_ctx, shape, d)])
        assert _same_bits(frames4[0], frames[0]) and np.array_equal(s4, stats)
        snap.destroy()


def test_no_tissue_in_the_box_has_no_extremes(hip_ctx):
    shape = (65, 2)
    a = _values(shape)
    snap = Snap(hip_ctx, shape, mask=np.zeros(a.shape, dtype=bool), fill=7.0)
    frames, stats = snap.take([_field(hip_ctx, shape, a)])
    snap.destroy()
    assert (frames == 7.0).all() and np.isnan(stats[0, 0]) and np.isnan(stats[0, 1]) and stats[0, 2] == 0


def test_eight_fields_in_one_launch(hip_ctx):
    """Eight fields that start at eight different offsets from a 512-byte boundary, one launch, fp32."""
    from beat._device import Field

    shape = (65, 7, 5)
    n, plane = 65 * 7 * 5, 65 * 7
    ld = n + 2 * plane + 3  # (odd: every field another alignment)
    buf = hip_ctx.zeros(8 * ld)
    buf.fill_(float("nan"))
    fields, values = [], []
    for k in range(8):
        f = Field(hip_ctx, n, plane, buf=buf, offset=plane + k * ld)
        a = _values(shape, seed=10 + k)
        f.set(a.ravel())
        fields.append(f)
        values.append(a)
    assert len({(f.ptr.value // 8) % 64 for f in fields}) == 8
    snap = Snap(hip_ctx, shape, (1, 0, 1), (64, 7, 4), (2, 3, 1), np.float32, nfields=8)
    frames, stats = snap.take(fields)
    snap.destroy()
    for k, a in enumerate(values):
        assert _same_bits(frames[k], _as(a[snap.slices()], np.float32)), k
        box = a[snap.box()]
        assert stats[k, 0] == box.min() and stats[k, 1] == box.max() and stats[k, 2] == 0


def test_frame_holds_what_the_field_held_at_enqueue(hip_ctx):
    """Enqueue, overwrite the field on the compute stream, then wait: the frame is the old field."""
    shape = (130, 9, 4)
    a = _values(shape)
    f = _field(hip_ctx, shape, a)
    snap = Snap(hip_ctx, shape, stride=2)
    rc, slot = snap.enqueue([f])
    assert rc == 0
    f.fill(4321.0)
    frames, _ = snap.wait(slot)
    assert snap.release(slot) == 0
    assert _same_bits(frames[0], a[snap.slices()])
    frames, stats = snap.take([f])
    snap.destroy()
    assert (frames == 4321.0).all() and stats[0, 0] == 4321.0 == stats[0, 1]


def test_depth_one_is_busy_until_released(hip_ctx):
    shape = (65, 7, 5)
    a, b = _values(shape), _values(shape, seed=3)
    fa, fb = _field(hip_ctx, shape, a), _field(hip_ctx, shape, b)
    snap = Snap(hip_ctx, shape, stride=(1, 2, 1), depth=1)
    rc, slot = snap.enqueue([fa])
    assert (rc, slot) == (0, 0)
    assert snap.enqueue([fb])[0] == EBUSY  # (returns at once: nothing waits in there)
    assert b"in flight" in snap.lib.beat_last_error()
    first, _ = snap.wait(slot)
    assert snap.enqueue([fb])[0] == EBUSY  # waited for, not released
    assert snap.release(slot) == 0
    rc, slot = snap.enqueue([fb])
    assert (rc, slot) == (0, 0)
    second, _ = snap.wait(slot)
    assert snap.release(slot) == 0
    snap.destroy()
    assert _same_bits(first[0], a[snap.slices()]) and _same_bits(second[0], b[snap.slices()])


def test_two_slots_take_turns(hip_ctx):
    shape = (63, 5)
    vals = [_values(shape, seed=s) for s in range(3)]
    snap = Snap(hip_ctx, shape, depth=2)
    slots = []
    for v in vals[:2]:
        rc, slot = snap.enqueue([_field(hip_ctx, shape, v)])
        assert rc == 0
        slots.append(slot)
    assert slots == [0, 1] and snap.enqueue([_field(hip_ctx, shape, vals[2])])[0] == EBUSY
    got0, _ = snap.wait(0)
    assert snap.release(0) == 0
    rc, slot = snap.enqueue([_field(hip_ctx, shape, vals[2])])
    assert (rc, slot) == (0, 0)
    got1, _ = snap.wait(1)
    got2, _ = snap.wait(0)
    assert snap.release(1) == 0 and snap.release(0) == 0
    snap.destroy()
    for got, v in zip((got0, got1, got2), vals):
        assert _same_bits(got[0], v[snap.slices()])


@pytest.mark.parametrize("shape", [(130,), (65, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_without_statistics_the_frames_are_unchanged(hip_ctx, shape):
    a = _values(shape)
    f = _field(hip_ctx, shape, a)
    for flags in (0, 2, 3):  # no statistics; non-temporal loads without and with them
        snap = Snap(hip_ctx, shape, stride=MIXED[: len(shape)], dtype=np.float32, flags=flags)
        frames, stats = snap.take([f])
        snap.destroy()
        assert _same_bits(frames[0], _as(a[snap.slices()], np.float32))
        if flags & 1:
            assert stats[0, 0] == a.min() and stats[0, 1] == a.max() and stats[0, 2] == 0
        else:
            assert np.isnan(stats[0, 0]) and np.isnan(stats[0, 1]) and stats[0, 2] == -1


def test_node_indices_past_two_to_the_31(hip_ctx):
    """A grid of 2048 x 1024 x 1025 nodes: the last plane's node indices do not fit 32 bits.  Only the box is ever read."""
    import torch

    from beat._device import Field

    shape = (2048, 1024, 1025)
    n, plane = shape[0] * shape[1] * shape[2], shape[0] * shape[1]
    assert n - plane >= 2 ** 31
    buf = torch.empty(n, dtype=torch.float64, device=hip_ctx.device)
    rng = np.random.default_rng(31)
    tail = rng.standard_normal((2, shape[1], shape[0]))
    buf[n - 2 * plane:].copy_(torch.from_numpy(tail.ravel()))
    f = Field(hip_ctx, n, 0, buf=buf, offset=0)
    snap = Snap(hip_ctx, shape, (2000, 1000, 1023), (2048, 1024, 1025), (3, 2, 1))
    frames, stats = snap.take([f])
    snap.destroy()
    del f, buf
    torch.cuda.empty_cache()  # (17 GB go back to the driver, not into the allocator's cache)
    want = tail[:, 1000:1024:2, 2000:2048:3]
    assert _same_bits(frames[0], want)
    box = tail[:, 1000:1024, 2000:2048]
    assert stats[0, 0] == box.min() and stats[0, 1] == box.max() and stats[0, 2] == 0


def test_refusals(hip_ctx):
    """BEAT_EINVAL with nothing made or enqueued."""
    lib = hip_ctx.lib
    good = dict(n=(65, 7, 5), lo=(0, 0, 0), hi=(65, 7, 5), stride=(1, 1, 1), dtype=0, nfields=1, depth=1)

    def create(**kw):
        a = {**good, **kw}
        handle = C.c_void_p()
        arr = lambda v: None if v is None else _i64x3(v)  # noqa: E731
        rc = lib.beat_snap_create(None if a.get("ctx", 1) is None else hip_ctx.handle, arr(a["n"]), arr(a["lo"]), arr(a["hi"]),
                                  arr(a["stride"]), a["dtype"], a["nfields"], a["depth"], None, 0.0, a.get("flags", 1),
                                  None if a.get("out", 1) is None else C.byref(handle))
        return rc, handle

    for bad in (dict(stride=(1, 0, 1)), dict(stride=(-1, 1, 1)), dict(lo=(3, 0, 0), hi=(3, 7, 5)), dict(lo=(4, 0, 0), hi=(3, 7, 5)),
                dict(hi=(66, 7, 5)), dict(hi=(65, 7, 6)), dict(lo=(-1, 0, 0)), dict(n=None), dict(lo=None), dict(hi=None), dict(stride=None),
                dict(ctx=None), dict(out=None), dict(nfields=0), dict(nfields=9), dict(depth=0), dict(dtype=2), dict(dtype=-1),
                dict(flags=4), dict(n=(0, 7, 5))):
        rc, handle = create(**bad)
        assert rc == EINVAL and handle.value is None, bad
        assert lib.beat_last_error()
    rc, handle = create()
    assert rc == 0 and handle.value
    f = _field(hip_ctx, good["n"], _values(good["n"]))
    slot = C.c_int(-7)
    ptrs = (C.c_void_p * 1)(f.ptr.value)
    assert lib.beat_snap_enqueue(None, ptrs, C.byref(slot)) == EINVAL
    assert lib.beat_snap_enqueue(handle, None, C.byref(slot)) == EINVAL
    assert lib.beat_snap_enqueue(handle, ptrs, None) == EINVAL
    assert lib.beat_snap_enqueue(handle, (C.c_void_p * 1)(None), C.byref(slot)) == EINVAL
    assert lib.beat_snap_enqueue(handle, (C.c_void_p * 1)(f.ptr.value + 4), C.byref(slot)) == EINVAL
    assert slot.value == -7
    host = C.c_void_p()
    for s in (0, -1, 1):  # not in flight (nothing above was enqueued), out of range
        assert lib.beat_snap_wait(handle, s, C.byref(host), None) == EINVAL
        assert lib.beat_snap_release(handle, s) == EINVAL
    assert lib.beat_snap_wait(None, 0, C.byref(host), None) == EINVAL and lib.beat_snap_release(None, 0) == EINVAL
    assert lib.beat_snap_info(handle, None) == EINVAL
    assert lib.beat_snap_enqueue(handle, ptrs, C.byref(slot)) == 0 and slot.value == 0  # the only slot was free all along
    assert lib.beat_snap_wait(handle, 0, C.byref(host), None) == 0 and host.value
    assert lib.beat_snap_release(handle, 0) == 0
    assert lib.beat_snap_release(handle, 0) == EINVAL
    assert lib.beat_snap_destroy(handle) == 0
    assert lib.beat_snap_destroy(None) == 0
