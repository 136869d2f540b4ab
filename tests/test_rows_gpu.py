"""beat_rows_plan_* / beat_rows_to_fields / beat_fields_to_rows through the C ABI on synthetic arrays: every layout, class pattern and
field count against the NumPy statement of tests/_rows_cases.py.  All values are copies: every comparison is exact.  The outputs are
interior pointers into sentinel-filled buffers with a guard plane on either side, so a store outside [0, n) of an output shows."""
import ctypes as C

import numpy as np
import pytest

import _rows_cases as cases
from beat import _hip
from beat import _rows_layout as rl

pytestmark = pytest.mark.gpu

SHAPES = {120: (6, 5, 4), 441: (9, 7, 7)}  # under two waves with a tail; two blocks of 256 with a tail
GUARD = 64
SENTINEL = -777.25


def _layout(n, pattern, kind):
    cls = cases.cls_full(cases.markers(SHAPES[n], pattern))
    if kind == "grid":  # pos NULL, one array, ld larger than n
        return cases.shared_problem(rl.grid_layout(cls, 3, 9), S=9)
    if kind == "compact":  # pos given, one array with padding entries
        return cases.shared_problem(rl.compact_layout(n, *cases.compact_arrays(cls, 3), 3, 9), S=9)
    return cases.separate_problem(rl.marker_layout(n, cases.index_lists(cls, 3), (8, 10, 9)), S=(8, 10, 9))  # base / ld / rows per class


class _Device:
    """The problem's arrays on the device and a plan over them."""

    def __init__(self, ctx, pb):
        self.ctx, self.pb = ctx, pb
        self.arena_host = np.random.default_rng(5).standard_normal(pb.arena)
        self.arena = ctx.from_numpy(self.arena_host)
        self.cls = ctx.from_numpy(pb.cls)
        self.pos = None if pb.pos is None else ctx.from_numpy(pb.pos.astype(np.int32))
        self.plan = C.c_void_p()
        _hip.check(self.create(self.plan))

    def create(self, out, n=None, cls=True, pos=True, k=None, base=None, ld=None, cn=None, rows=None):
        pb = self.pb
        k = pb.k if k is None else k
        m = max(k, 1)
        base = [self.arena.data_ptr() + 8 * b for b in pb.base] if base is None else base
        arr = lambda t, v: (t * m)(*(list(v) + [v[-1]] * (m - len(v)))[:m])  # noqa: E731
        return self.ctx.lib.beat_rows_plan_create(
            self.ctx.handle, pb.n if n is None else n, self.cls.data_ptr() if cls is True else cls,
            (None if self.pos is None else self.pos.data_ptr()) if pos is True else pos, k, arr(C.c_void_p, base),
            arr(C.c_int64, pb.ld if ld is None else ld), arr(C.c_int64, pb.cn if cn is None else cn),
            arr(C.c_int, pb.rows if rows is None else rows), C.byref(out))

    def buffers(self, nf, values=None):
        """nf sentinel-filled buffers; the fields are the n doubles GUARD in.  ``values``: what the fields hold."""
        host = np.full((nf, self.pb.n + 2 * GUARD), SENTINEL)
        if values is not None:
            host[:, GUARD:-GUARD] = values
        dev = self.ctx.from_numpy(host)
        ptrs = (C.c_void_p * max(nf, 1))(*[dev.data_ptr() + 8 * (f * host.shape[1] + GUARD) for f in range(nf)])
        return host, dev, ptrs

    def rows_arg(self, rows):
        flat = [r for rows_f in rows for r in rows_f]
        return (C.c_int * max(len(flat), 1))(*flat)

    def close(self):
        _hip.check(self.ctx.lib.beat_rows_plan_destroy(self.plan))


CASES = [(n, pattern, kind) for n in SHAPES for pattern in ("checker", "thirds", "runs") for kind in ("grid", "compact", "markers")]


@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("n,pattern,kind", CASES, ids=lambda v: str(v))
def test_expand_and_collapse(hip_ctx, n, pattern, kind, max_blocks):
    pb = _layout(n, pattern, kind)
    dev = _Device(hip_ctx, pb)
    lib = hip_ctx.lib
    try:
        assert (pb.cls < 3).any() and (pattern != "runs" or (pb.cls == 255).any())
        for nf in (1, 3, 8):
            rows = cases.pick_rows(pb, nf, seed=nf)
            prior = np.random.default_rng(nf).standard_normal((nf, n))
            # KEEP: nodes without a source and everything outside [0, n) stay
            host, buf, ptrs = dev.buffers(nf, prior)
            _hip.check(lib.beat_rows_to_fields(dev.plan, nf, dev.rows_arg(rows), ptrs, _hip.ROWS_KEEP, 3.5, max_blocks))
            want = host.copy()
            want[:, GUARD:-GUARD] = cases.expand_ref(pb, dev.arena_host, rows, prior)
            assert buf.cpu().numpy().tobytes() == want.tobytes()
            # FILL, with plain and with non-temporal loads
            for mode in (_hip.ROWS_FILL, _hip.ROWS_FILL | _hip.ROWS_NT_LOADS):
                host, buf, ptrs = dev.buffers(nf, prior)
                _hip.check(lib.beat_rows_to_fields(dev.plan, nf, dev.rows_arg(rows), ptrs, mode, -2.5, max_blocks))
                want = host.copy()
                want[:, GUARD:-GUARD] = cases.expand_ref(pb, dev.arena_host, rows, prior, fill=-2.5)
                assert buf.cpu().numpy().tobytes() == want.tobytes()
            # collapse new values, then expand them again: the identity on marked nodes; padding entries, unmarked columns and the
            # rows that were not named stay as they were
            fields = np.random.default_rng(100 + nf).standard_normal((nf, n))
            _, buf, ptrs = dev.buffers(nf, fields)
            before = dev.arena.cpu().numpy()
            _hip.check(lib.beat_fields_to_rows(dev.plan, nf, dev.rows_arg(rows), ptrs, max_blocks))
            after = dev.arena.cpu().numpy()
            assert after.tobytes() == cases.collapse_ref(pb, before, rows, fields).tobytes()
            assert (after != before).sum() == nf * (pb.cls < 3).sum()
            host, buf2, ptrs2 = dev.buffers(nf)
            _hip.check(lib.beat_rows_to_fields(dev.plan, nf, dev.rows_arg(rows), ptrs2, _hip.ROWS_KEEP, 0.0, max_blocks))
            back = buf2.cpu().numpy()[:, GUARD:-GUARD]
            marked = pb.cls < 3
            np.testing.assert_array_equal(back[:, marked], fields[:, marked])
            np.testing.assert_array_equal(back[:, ~marked], SENTINEL)
            assert buf.cpu().numpy()[:, GUARD:-GUARD].tobytes() == fields.tobytes()  # (collapse does not write the fields)
            dev.arena.copy_(hip_ctx.from_numpy(dev.arena_host))
    finally:
        dev.close()


def test_bad_arguments_launch_nothing(hip_ctx):
    pb = _layout(120, "thirds", "markers")
    dev = _Device(hip_ctx, pb)
    lib, EINVAL = hip_ctx.lib, -1
    try:
        rows = cases.pick_rows(pb, 3, seed=3)
        host, buf, ptrs = dev.buffers(3, 1.0)
        arena0 = dev.arena.cpu().numpy()

        def refused(rc):
            assert rc == EINVAL and lib.beat_last_error() != b""
            hip_ctx.synchronize()
            assert buf.cpu().numpy().tobytes() == host.tobytes() and dev.arena.cpu().numpy().tobytes() == arena0.tobytes()

        flat = dev.rows_arg(rows)
        # nfields of 0 and 9
        _, _, nine_ptrs = dev.buffers(9, 1.0)
        for nf, p in ((0, ptrs), (9, nine_ptrs)):
            refused(lib.beat_rows_to_fields(dev.plan, nf, dev.rows_arg([[0, 0, 0]] * 9), p, _hip.ROWS_KEEP, 0.0, 0))
            refused(lib.beat_fields_to_rows(dev.plan, nf, dev.rows_arg([[0, 0, 0]] * 9), p, 0))
        # null plan, null or misaligned pointers
        refused(lib.beat_rows_to_fields(None, 3, flat, ptrs, _hip.ROWS_KEEP, 0.0, 0))
        refused(lib.beat_rows_to_fields(dev.plan, 3, None, ptrs, _hip.ROWS_KEEP, 0.0, 0))
        refused(lib.beat_rows_to_fields(dev.plan, 3, flat, None, _hip.ROWS_KEEP, 0.0, 0))
        for bad in (None, ptrs[1] + 4):
            p = (C.c_void_p * 3)(ptrs[0], bad, ptrs[2])
            refused(lib.beat_rows_to_fields(dev.plan, 3, flat, p, _hip.ROWS_FILL, 0.0, 0))
            refused(lib.beat_fields_to_rows(dev.plan, 3, flat, p, 0))
        # a row outside [0, class_rows[c]); unknown mode bits; collapse onto one row twice
        for bad in (-1, pb.rows[2]):
            r = [list(x) for x in rows]
            r[1][2] = bad
            refused(lib.beat_rows_to_fields(dev.plan, 3, dev.rows_arg(r), ptrs, _hip.ROWS_KEEP, 0.0, 0))
            refused(lib.beat_fields_to_rows(dev.plan, 3, dev.rows_arg(r), ptrs, 0))
        refused(lib.beat_rows_to_fields(dev.plan, 3, flat, ptrs, 2, 0.0, 0))
        r = [list(x) for x in rows]
        r[2][1] = r[0][1]
        refused(lib.beat_fields_to_rows(dev.plan, 3, dev.rows_arg(r), ptrs, 0))
        # the plan: num_classes of 0 and 33, null and misaligned pointers, n or a class_n at 2^31
        out = C.c_void_p()
        good_base = [dev.arena.data_ptr() + 8 * b for b in pb.base]
        for kw in (dict(k=0), dict(k=33), dict(cls=None), dict(pos=dev.pos.data_ptr() + 2), dict(base=[good_base[0], None, good_base[2]]),
                   dict(base=[good_base[0], good_base[1] + 4, good_base[2]]), dict(n=2**31), dict(cn=[pb.cn[0], 2**31, pb.cn[2]],
                                                                                               ld=[pb.ld[0], 2**31 + 8, pb.ld[2]]),
                   dict(ld=[pb.cn[0] - 1, pb.ld[1], pb.ld[2]]), dict(rows=[pb.rows[0], 0, pb.rows[2]])):
            refused(dev.create(out, **kw))
            assert out.value is None
        assert lib.beat_rows_plan_create(hip_ctx.handle, pb.n, dev.cls.data_ptr(), None, 3, None, None, None, None, C.byref(out)) == EINVAL
        assert lib.beat_rows_plan_destroy(None) == 0
    finally:
        dev.close()


def test_a_position_outside_its_class_is_never_addressed(hip_ctx):
    """The kernel's own guard: a plan whose positions point past a class's array (the Python layer refuses to build one) moves
    nothing for those nodes."""
    pb = _layout(120, "thirds", "markers")
    short = cases.Problem(pb.n, pb.cls, pb.pos, pb.base, pb.ld, [m - 5 for m in pb.cn], pb.rows, pb.arena)
    dev = _Device(hip_ctx, short)
    try:
        rows = cases.pick_rows(short, 2, seed=4)
        prior = np.zeros((2, pb.n))
        host, buf, ptrs = dev.buffers(2, prior)
        _hip.check(hip_ctx.lib.beat_rows_to_fields(dev.plan, 2, dev.rows_arg(rows), ptrs, _hip.ROWS_FILL, 9.0, 0))
        want = cases.expand_ref(short, dev.arena_host, rows, prior, fill=9.0)
        assert (np.array(want) == 9.0).sum() == 2 * 15
        assert buf.cpu().numpy()[:, GUARD:-GUARD].tobytes() == np.array(want).tobytes()
        _, buf, ptrs = dev.buffers(2, 4.0)
        _hip.check(hip_ctx.lib.beat_fields_to_rows(dev.plan, 2, dev.rows_arg(rows), ptrs, 0))
        assert dev.arena.cpu().numpy().tobytes() == cases.collapse_ref(short, dev.arena_host, rows, np.full((2, pb.n), 4.0)).tobytes()
    finally:
        dev.close()
