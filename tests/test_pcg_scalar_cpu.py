"""CPU: the scalar steps of the PCG (csrc/beat_pcg_scalar.h: the start of a solve, the roll, the predicted stop, the single-reduction
step, and the one stopping test under all of them), built with g++ into tests/pcg_scalar_harness.cpp -- once plain, once with the
address and undefined-behaviour sanitizers -- and driven line by line.  Begin and roll are held to the independent Python
implementation of tests/_oracle_ops.py with ==; whole Jacobi-PCG solves on the cases of tests/_pcg_ref.py run with NumPy vectors and
every scalar decision taken by the header."""
import shutil

import numpy as np
import pytest

import _oracle_ops as oo
import _pcg_ref as ref
from _pcg_scalar import BUILDS, Harness, build, same_bits
from beat import _hip

NAMES = ["BB", "RZ", "RR", "PQ", "RZN", "RRN", "TOL2", "BETA", "STOP", "ITERS", "REASON", "RTOL", "ATOL", "MAXIT", "NUPD"]
BB, RZ, RR, PQ, RZN, RRN, TOL2, BETA, STOP, ITERS, REASON, RTOL, ATOL, MAXIT, NUPD = (getattr(oo, "ST_" + n) for n in NAMES)
RR0, ALPHA, PQS, RQ, QQ = 15, 16, 17, 18, 19  # (test_layout holds these, and the names above, to the header)
RING = 6
NAN = float("nan")


@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    out = tmp_path_factory.mktemp("pcg_scalar_harness")
    return {name: build(out, name) for name in BUILDS}


@pytest.fixture(params=list(BUILDS))
def harness(executables, request):
    h = Harness(executables[request.param])
    h.build = request.param
    yield h
    h.close()


def test_layout(harness):
    lay = harness.layout()
    for name in NAMES:
        assert lay[name] == getattr(oo, "ST_" + name), name
    for name in ("BB", "RZ", "RR", "PQ", "RZN", "RRN", "TOL2", "BETA", "STOP", "ITERS", "REASON", "NUPD"):
        assert lay[name] == getattr(_hip, "ST_" + name), name
    assert [lay[n] for n in ("RR0", "ALPHA", "PQS", "RQ", "QQ")] == [RR0, ALPHA, PQS, RQ, QQ]
    assert lay["DOUBLES"] >= 20 and lay["DOUBLES"] > max(lay[n] for n in NAMES + ["RR0", "ALPHA", "PQS", "RQ", "QQ"])
    # the host reads the first 16 slots: everything a solve's record is made of lies there, the device-only sums behind it
    assert _hip.ST_SIZE == 16 and all(lay[n] < 16 for n in NAMES + ["RR0"]) and all(lay[n] >= 16 for n in ("ALPHA", "PQS", "RQ", "QQ"))
    assert [lay[k] for k in ("NONE", "ROLL", "BEGIN", "PREDICT", "MERGED")] == [0, 1, 2, 3, 4]


# ---- begin and roll against tests/_oracle_ops.py ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle():
    ops = oo.OracleOps((2, 2, 2), True, True, *ref.tables(3))
    ops.set_timestep(ref.C_M, ref.THETA, ref.DT)
    return ops


def _oracle_begin(ops, st, rtol, atol, max_it):
    ops.st[:] = oo.torch.from_numpy(np.array(st[:16]))
    ops.cg_begin(rtol, atol, max_it)
    return ops.st.numpy().copy()


def _oracle_roll(ops, st):
    ops.st[:] = oo.torch.from_numpy(np.array(st[:16]))
    ops.r.data.zero_()  # (cg_next also forms p = D^-1 r + beta p: keep it finite)
    ops.p.data.zero_()
    ops.cg_next()
    return ops.st.numpy().copy()


def _check_begin(h, ops, state, rtol, atol, max_it):
    h.set(state)
    got, _ = h.begin(rtol, atol, max_it)
    want = _oracle_begin(ops, state, rtol, atol, max_it)
    assert np.array_equal(got[:15], want[:15], equal_nan=True), (state[:15], rtol, atol, max_it, got[:15], want[:15])
    assert same_bits(got[RR0], state[RR]) and same_bits(got[16:], state[16:])  # r.r of the guess is kept; nothing else is touched
    return got


def _check_roll(h, ops, state):
    h.set(state)
    got, _ = h.roll()
    want = _oracle_roll(ops, state)
    assert np.array_equal(got[:15], want[:15], equal_nan=True), (state[:15], got[:15], want[:15])
    assert same_bits(got[15:], state[15:])
    return got


def _random_state(rng):
    st = np.zeros(32)
    scale = 10.0 ** rng.uniform(-12, 6)
    st[BB] = scale * 10.0 ** rng.uniform(-2, 8)
    st[[RZ, RR, RZN, RRN]] = scale * 10.0 ** rng.uniform(-14, 2, 4)
    st[[PQ, BETA, ALPHA]] = rng.standard_normal(3)
    st[ITERS], st[NUPD] = rng.integers(0, 8), rng.integers(0, 8)
    st[16:] = rng.standard_normal(16)
    return st


def test_begin_and_roll_equal_the_python_implementation(harness, oracle):
    rng = np.random.default_rng(20260)
    latched = {0.0: 0, 2.0: 0, 3.0: 0, -3.0: 0}
    for _ in range(300):
        st = _random_state(rng)
        rtol = float(rng.choice([0.0, 1e-12, 1e-9, 1e-6, 1e-3, 10.0 ** rng.uniform(-14, 0)]))
        atol = float(rng.choice([0.0, 0.0, 10.0 ** rng.uniform(-12, 3)]))
        begun = _check_begin(harness, oracle, st, rtol, atol, int(rng.integers(0, 12)))
        latched[begun[REASON]] += 1
        begun[STOP] = begun[REASON] = 0.0  # (a latched state does not roll: see test_latched_steps_are_no_ops)
        begun[ITERS] = st[ITERS]
        latched[_check_roll(harness, oracle, begun)[REASON]] += 1
    assert all(v >= 10 for v in latched.values()), latched  # every outcome was met many times


def test_begin_and_roll_branch_by_branch(harness, oracle):
    def state(bb, rr, rrn=0.0, iters=0.0, rtol=0.0, atol=0.0, max_it=0.0, rz=2.0, rzn=1.0):
        st = np.zeros(32)
        st[[BB, RZ, RR, RZN, RRN, ITERS, RTOL, ATOL, MAXIT]] = bb, rz, rr, rzn, rrn, iters, rtol, atol, max_it
        return st

    def begun(bb, rr, rtol, atol, max_it):
        got = _check_begin(harness, oracle, state(bb, rr), rtol, atol, max_it)
        return got[STOP], got[REASON], got[TOL2]

    assert begun(4.0, 1.0, 0.5, 0.0, 5) == (1.0, 2.0, 1.0)            # rr == tol2 exactly, the threshold rtol's
    assert begun(4.0, np.nextafter(1.0, 2.0), 0.5, 0.0, 5) == (0.0, 0.0, 1.0)
    assert begun(4.0, 1.0, 0.5, 2.0, 5) == (1.0, 2.0, 4.0)            # atol's threshold, met by rtol's too: reason 2
    assert begun(4.0, 4.0, 0.5, 2.0, 5) == (1.0, 3.0, 4.0)            # rr == tol2 exactly, by atol only: reason 3
    assert begun(4.0, 3.0, 0.5, 0.0, 0) == (0.0, 0.0, 1.0)            # max_it = 0: begin does not latch
    assert begun(4.0, 1e-30, 1e-9, 0.0, 5)[:2] == (1.0, 2.0)          # a right-hand side the guess already solves
    assert begun(0.0, 0.0, 1e-9, 0.0, 5) == (1.0, 2.0, 0.0)           # b = 0, r = 0

    def rolled(st):
        got = _check_roll(harness, oracle, st)
        return got[STOP], got[REASON], got[ITERS]

    th = dict(rtol=0.5, max_it=5.0)

    def with_tol(st, atol=0.0):
        st[TOL2] = max(0.25 * st[BB], atol * atol)
        return st

    assert rolled(with_tol(state(4.0, 9.0, rrn=1.0, **th))) == (1.0, 2.0, 1.0)                       # rr == tol2 exactly
    assert rolled(with_tol(state(4.0, 9.0, rrn=np.nextafter(1.0, 2.0), **th))) == (0.0, 0.0, 1.0)
    assert rolled(with_tol(state(4.0, 9.0, rrn=4.0, atol=2.0, **th), 2.0)) == (1.0, 3.0, 1.0)        # atol-dominated threshold
    assert rolled(with_tol(state(4.0, 9.0, rrn=0.5, atol=2.0, **th), 2.0)) == (1.0, 2.0, 1.0)
    assert rolled(with_tol(state(4.0, 9.0, rrn=3.0, iters=3.0, **th))) == (0.0, 0.0, 4.0)
    assert rolled(with_tol(state(4.0, 9.0, rrn=3.0, iters=4.0, **th))) == (1.0, -3.0, 5.0)           # iters == max_it - 1: cut
    assert rolled(with_tol(state(4.0, 9.0, rrn=1.0, iters=4.0, **th))) == (1.0, 2.0, 5.0)            # convergence first, then max_it
    assert rolled(with_tol(state(4.0, 9.0, rrn=3.0, rtol=0.5, max_it=0.0))) == (1.0, -3.0, 1.0)      # max_it = 0: the first roll cuts

    # NaN in RRN: never converged, cut at max_it, and nothing but the roll's own slots changes
    st = with_tol(state(4.0, 9.0, rrn=NAN, **th))
    for k in range(1, 6):
        st = _check_roll(harness, oracle, st)
        assert (st[STOP], st[REASON], st[ITERS]) == ((1.0, -3.0, 5.0) if k == 5 else (0.0, 0.0, float(k)))
        assert np.isnan(st[RR]) and st[BETA] == (0.5 if k == 1 else 1.0) and st[RZ] == 1.0 and st[TOL2] == 1.0 and st[NUPD] == 0.0


def test_latched_steps_are_no_ops(harness):
    rng = np.random.default_rng(7)
    for stop in (1.0, -1.0, 2.0, NAN):  # (st[STOP] != 0: a NaN counts)
        st = _random_state(rng)
        st[STOP], st[REASON] = stop, 2.0
        st[[RTOL, ATOL, MAXIT, TOL2]] = 1e-6, 0.0, 50.0, 1e-12 * st[BB]
        alphas = rng.standard_normal(12)
        harness.set(st)
        harness.alpha(alphas)
        for step in (harness.roll, lambda: harness.predict(3, 1e-13), lambda: harness.merged(4)):
            got, al = step()
            assert same_bits(got, st) and same_bits(al, alphas)
        got, al = harness.begin(1e-6, 0.0, 50)  # the start of the next solve resets the latch
        assert same_bits(al, alphas) and got[ITERS] == 0.0 and got[NUPD] == 0.0 and got[STOP] == (1.0 if st[RR] <= got[TOL2] else 0.0)


# ---- whole solves through the header ----------------------------------------------------------------------------------------------

_systems: dict = {}


def system(shape):
    """(A, b, x0, 1 / diag A) of the shape's case in float64: the float64 run of _pcg_ref.reference starts from the same roundings."""
    if shape not in _systems:
        p, v = ref.problem(shape), ref.field(shape)
        _systems[shape] = (p.A, ref.rhs_longdouble(p, v).astype(np.float64), v.copy(), 1.0 / p.A.diagonal())
    return _systems[shape]


def apply(A, x):
    return ref.matvec(A, x, np.float64)


def predict_bound(n):
    """c = 4 (2 D + 8) 2^-53 (beat_rr_predict_bound's form) with D = n + 16: no sum of n terms on the host is deeper."""
    return 4.0 * (2.0 * (n + 16) + 8.0) * 2.0**-53


def inline_solve(shape, rtol):
    """Jacobi-PCG with the stopping test written out here: (iterations, reason, [x_1 ..])."""
    A, b, x, dinv = system(shape)
    r = b - apply(A, x)
    z = dinv * r
    bb, rz, rr = b @ b, r @ z, r @ r
    tr = rtol * rtol * bb
    tol2 = max(tr, 0.0)
    p, xs, iters = z, [], 0
    if rr <= tol2:
        return 0, 2 if rr <= tr else 3, xs
    while True:
        q = apply(A, p)
        alpha = rz / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        xs.append(x)
        rzn, rr = r @ (dinv * r), r @ r
        beta, rz, iters = rzn / rz, rzn, iters + 1
        if rr <= tol2:
            return iters, 2 if rr <= tr else 3, xs
        if iters >= ref.KMAX:
            return iters, -3, xs
        p = dinv * r + beta * p


_classic: dict = {}


def classic_solve(h, shape, rtol):
    """The same loop with every scalar decision taken by the header, the sums fed in as a reduction would write them; before each
    residual update the predicted stop is tried on a copy of the state and held to what the explicit update and roll then decide.
    -> (iterations, reason, [x_1 ..], settled: the prediction latched the solve)"""
    key = (h.build, shape, rtol)
    if key in _classic:
        return _classic[key]
    A, b, x, dinv = system(shape)
    c = predict_bound(len(b))
    r = b - apply(A, x)
    h.set(np.zeros(32))
    h.set([b @ b, r @ (dinv * r), r @ r])
    st, _ = h.begin(rtol, 0.0, ref.KMAX)
    p, xs, settled, i = dinv * r, [], False, 0
    while st[STOP] == 0.0:
        q = apply(A, p)
        slot = i % RING
        before, alphas = h.dump()
        sums = [p @ q, r @ q, q @ q]
        for bad in range(3):  # a NaN in any of the three sums: no latch
            h.set([NAN if k == bad else s for k, s in enumerate(sums)], first=PQS)
            got, _ = h.predict(slot, c)
            assert got[STOP] == 0.0 and got[ITERS] == before[ITERS] and got[NUPD] == before[NUPD]
            h.set(before)
            h.alpha(alphas)
        h.set(sums, first=PQS)
        pred, pred_alphas = h.predict(slot, c)
        h.set(before)  # the explicit update and roll work on the untouched state
        h.alpha(alphas)
        alpha = st[RZ] / sums[0]
        x = x + alpha * p
        r = r - alpha * q
        xs.append(x)
        h.set([sums[0], r @ (dinv * r), r @ r], first=PQ)
        h.set([st[NUPD] + 1.0], first=NUPD)
        st, _ = h.roll()
        if pred[STOP] != 0.0:
            m = np.sqrt(before[RR]) + abs(alpha) * np.sqrt(sums[2])
            assert st[STOP] == 1.0 and st[REASON] == pred[REASON] and st[ITERS] == pred[ITERS] and st[NUPD] == pred[NUPD], (shape, rtol, i)
            assert same_bits(pred_alphas[slot], alpha) and abs(pred[RR] - st[RR]) <= c * m * m, (shape, rtol, pred[RR], st[RR])
            settled = True
        else:
            assert same_bits(pred[[RZ, RR, ITERS, NUPD, STOP, REASON]], before[[RZ, RR, ITERS, NUPD, STOP, REASON]]) and pred[PQ] == sums[0]
            assert same_bits(pred_alphas, alphas)
        p = dinv * r + st[BETA] * p
        i += 1
    _classic[key] = (int(st[ITERS]), int(st[REASON]), xs, settled)
    return _classic[key]


CASES = [(shape, rtol) for shape in ref.SHAPES for rtol in ref.RTOLS]


def test_whole_solves_decide_as_the_inline_test_does(harness):
    for shape, rtol in CASES:
        iters, reason, xs, _ = classic_solve(harness, shape, rtol)
        want_iters, want_reason, want_xs = inline_solve(shape, rtol)
        assert (iters, reason) == (want_iters, want_reason) and reason == 2, (shape, rtol)
        assert all(np.array_equal(a, b) for a, b in zip(xs, want_xs))
        assert abs(iters - ref.plain_reference(shape).stop(rtol)) <= 1, (shape, rtol, iters)


def test_predicted_stop_never_decides_differently(harness):
    """(The agreement itself is asserted in classic_solve, at every iteration of every case.)  Against a vacuous pass: a NumPy mirror
    of the arithmetic on exactly these inputs settled 28 of the 30 cases; the two left over are (2, 2, 2), where CG ends at n = 8 and
    the accuracy condition E <= 2^-20 rho rightly refuses."""
    settled = [case for case in CASES if classic_solve(harness, *case)[3]]
    assert len(settled) >= 26, sorted(set(CASES) - set(settled))


def test_single_reduction_step(harness):
    """Chronopoulos & Gear's loop with every scalar through merged_next, against the classic run of the same case."""
    for shape, rtol in CASES:
        k_classic, _, xs_classic, _ = classic_solve(harness, shape, rtol)
        A, b, x, dinv = system(shape)
        r = b - apply(A, x)
        harness.set(np.zeros(32))
        harness.set([b @ b, r @ (dinv * r), r @ r])
        st, _ = harness.begin(rtol, 0.0, ref.KMAX)
        _, alphas = harness.alpha(np.full(12, -7.0))
        p, xs, passes = np.zeros_like(r), [], 0
        while st[STOP] == 0.0:
            u = dinv * r
            harness.set([u @ apply(A, u), r @ u, r @ r], first=PQ)
            slot, before = passes % RING, st
            st, now = harness.merged(slot)
            passes += 1
            if st[STOP] != 0.0:  # no update follows: neither counted nor given a step length
                assert st[NUPD] == before[NUPD] and st[ITERS] == before[ITERS] and same_bits(now, alphas)
                break
            assert st[NUPD] == before[NUPD] + 1.0 and st[ITERS] == before[ITERS] + 1.0 and same_bits(now[slot], st[ALPHA])
            assert same_bits(np.delete(now, slot), np.delete(alphas, slot))
            alphas = now
            p = u + st[BETA] * p
            r = r - st[ALPHA] * apply(A, p)
            x = x + st[ALPHA] * p
            xs.append(x)
        k = int(st[ITERS])
        assert st[REASON] == 2.0 and k == len(xs) == passes - 1 and abs(passes - (k_classic + 1)) <= 1, (shape, rtol, passes, k_classic)
        kk = min(k, k_classic)
        err = np.abs(xs[kk - 1] - xs_classic[kk - 1]).max()
        assert err <= ref.plain_reference(shape).x_bound(kk), (shape, rtol, kk, err)
