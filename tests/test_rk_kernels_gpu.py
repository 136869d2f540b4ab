"""Kernel-level tests of the Runge-Kutta stage kernels (csrc/beat_pde_rk.hip) through the C ABI, over grid shapes that reach
what the model-level tests (tests/test_rk_gpu.py) do not: a second pass of the x lane loop (nx > 64), the row grid-stride
(ny * nz > 8192 rows), 1-D grids (all y / z rows collapsed), axes of 2 nodes and off-diagonal conductivity.

The shifted apply is checked against the assembled S = a Mass + (b + i c) K, the COCG solve against its host restatement
(tests/_rk_oracle.py: jacobi_cocg, in extended precision) iteration by iteration, the stage right-hand side and the final
update against extended-precision sums; then the chunked enqueue of the iterations, degenerate right-hand sides and the
arguments the ABI refuses."""

import ctypes as C

import numpy as np
import pytest

from _rk_oracle import jacobi_cocg

pytestmark = pytest.mark.gpu

BEAT_EINVAL = -1
H = 0.125  # mesh spacing of every axis: dyadic, so that the oracle's node coordinates and their differences are exact
BIG = 50_000  # nodes up to which the host reference works in extended precision (complex256); complex128 above


def _conductivity(kind, dim):
    if dim == 1:
        return 1.0
    if kind == "aniso2":
        return np.array([[2.0, 0.3], [0.3, 1.0]])
    if kind == "aniso3":
        f0 = np.array([np.cos(np.pi / 6), np.sin(np.pi / 6), 0.0])
        return 9.5e-4 * np.outer(f0, f0) + 1.25e-4 * (np.eye(3) - np.outer(f0, f0))
    return np.diag([1.0, 0.6, 0.3][:dim]) if dim == 3 else np.diag([1.0, 0.5])


def _shapes():
    """(nodes per axis, conductivity): off-diagonal tensors on every other 2-D / 3-D grid."""
    fixed = [(2,), (64,), (65,), (130,), (100_001,),
             (65, 2), (63, 40), (129, 33), (2, 301), (65, 8201),
             (3, 3, 3), (2, 2, 41), (64, 3, 2), (65, 15, 33), (70, 95, 95)]
    rng = np.random.default_rng(20261016)
    for k in range(8):  # in the style of test_gpu_kernels._sweep_shapes: up to ~50 k nodes
        if k % 3 == 2:
            fixed.append((int(rng.integers(2, 330)), int(rng.integers(2, 150))))
        else:
            fixed.append((int(rng.integers(2, 330)), int(rng.integers(2, 20)), int(rng.integers(2, 8))))
    out, m = [], 0
    for s in fixed:
        if len(s) == 1:
            out.append((s, "diag"))
        else:
            out.append((s, ("aniso2" if len(s) == 2 else "aniso3") if m % 2 == 0 else "diag"))
            m += 1
    return out


class _System:
    """The operator handle of a grid of `nodes` and its assembled Mass and K (oracle/fem.py)."""

    def __init__(self, ctx, nodes, cond):
        from beat import _stencil
        from beat.irksome_model import _RkOps
        from oracle import fem

        dim = len(nodes)
        cells = tuple(v - 1 for v in nodes)
        Mt = _conductivity(cond, dim)
        om = fem.BoxMesh(cells, tuple(H * c for c in cells))
        self.Mm = fem.assemble_mass(om).tocsr()
        self.K = fem.assemble_stiffness(om, Mt).tocsr()
        mt, kt = _stencil.stencil_tables(dim, (H,) * dim, Mt)
        self.ops = _RkOps(ctx, tuple(nodes) + (1,) * (3 - dim), mt, kt)
        self.lib, self.handle, self.n, self.nodes = self.ops.lib, self.ops.handle, om.num_nodes, nodes
        # b / a of the stage operators in units of h^2 / lambda_max(M): the same conditioning on every grid
        self.h2 = H * H / float(np.max(np.linalg.eigvalsh(np.atleast_2d(Mt))))
        self.cdt = np.clongdouble if self.n <= BIG else np.complex128
        self.rdt = np.longdouble if self.n <= BIG else np.float64

    def S(self, a, b, c=0.0):
        return (a * self.Mm + complex(b, c) * self.K) if c != 0.0 else (a * self.Mm + b * self.K)

    def field(self, key, values=None, poison=True):
        f = self.ops.field(key)
        if values is not None:
            f.set(values)
        if poison:  # the RK kernels gather inside the box only: the ghost planes must never be read
            f.ghost_lo.fill_(float("nan"))
            f.ghost_hi.fill_(float("nan"))
        return f

    def solve(self, a, b, c, rhs, rtol, atol, max_it, cplx=True, x0=None):
        """Device solve of (a Mass + (b + i c) K) x = rhs; complex instantiation when `cplx`: returns (x, KspResult)."""
        br = self.field("br", np.real(rhs))
        bi = self.field("bi", np.imag(rhs)) if cplx else None
        xr = self.field("xr", x0)
        xi = self.field("xi", x0) if cplx else None
        res = self.ops.solve(a, complex(b, c) if cplx else b, br, bi, xr, xi, rtol, atol, max_it)
        x = xr.numpy() + 1j * xi.numpy() if cplx else xr.numpy()
        return x, res


def _host_at(S, b, its, dtype):
    """The host iterate after exactly `its` iterations (no stopping test)."""
    return jacobi_cocg(S, b, 0.0, 0.0, max(its, 1), dtype)[0] if its > 0 else np.zeros(b.shape, dtype=dtype)


def _check_solve(sysm, a, b, c, rhs, rtol, atol, reason, cplx=True, what=""):
    """Device COCG (or real PCG) against the host restatement: iteration count, iterate, reported norms, true residual,
    stopping reason.  Returns the device x."""
    dt = sysm.cdt if cplx else sysm.rdt
    S = sysm.S(a, b, c)
    xd, res = sysm.solve(a, b, c, rhs, rtol, atol, 500, cplx=cplx)
    xh, its, rh, rn, bn, hist = jacobi_cocg(S, rhs, rtol, atol, 500, dt)
    tag = f"{what} rtol={rtol} atol={atol}: device {res.iterations} its, host {its} its"
    print(f"{sysm.nodes} {tag}")
    assert rh == reason, tag
    if res.iterations != its:
        # only a stop decided within 1 % of the threshold may land on the neighbouring iteration
        assert abs(res.iterations - its) == 1, tag
        k = its - 1 if res.iterations > its else its - 2
        assert abs(hist[k] - 1.0) <= 0.01, (tag, hist[k])
        xh, _, _, rn, _, _ = jacobi_cocg(S, rhs, 0.0, 0.0, res.iterations, dt)  # the host's iterate at the device's count
    assert res.converged_reason == reason, tag
    xh = np.asarray(xh, dtype=np.complex128 if cplx else np.float64)
    assert np.abs(xd - xh).max() <= 1e-9 * np.abs(xh).max(), (tag, np.abs(xd - xh).max() / np.abs(xh).max())
    assert abs(res.rhs_norm - bn) <= 1e-10 * bn, tag
    assert abs(res.residual_norm - rn) <= 1e-10 * rn + 1e-13 * bn, (tag, res.residual_norm, rn)
    r_true = np.asarray(rhs, dtype=dt) - S.astype(dt) @ np.asarray(xd, dtype=dt)
    assert float(np.linalg.norm(r_true)) <= max(rtol * bn, atol) * (1 + 1e-6), tag
    return xd, res


@pytest.mark.parametrize("nodes, cond", _shapes(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_stage_kernels_over_grid_shapes(hip_ctx, nodes, cond):
    """zapply, zsolve (complex and real instantiation), rk_rhs and rk_update on one grid against host references."""
    from beat import _hip

    sysm = _System(hip_ctx, nodes, cond)
    n, h2, lib, hd = sysm.n, sysm.h2, sysm.lib, sysm.handle
    rng = np.random.default_rng(n)

    # 1. q = S p, the shifted apply: mixed, real-shift and strongly stiffness-dominated operators
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xr, xi = sysm.field("ar", x.real), sysm.field("ai", x.imag)
    yr, yi = sysm.field("yr"), sysm.field("yi")
    for a, b, c in ((1.0, 0.5 * h2, 0.3 * h2), (1.0, 0.7 * h2, 0.0), (1e-3, 50.0 * h2, 20.0 * h2)):
        _hip.check(lib.beat_pde_zapply(hd, a, b, c, xr.ptr, xi.ptr, yr.ptr, yi.ptr))
        y = yr.numpy() + 1j * yi.numpy()
        ref = np.asarray(sysm.S(a, b, c).astype(sysm.cdt) @ x.astype(sysm.cdt), dtype=np.complex128)
        assert np.abs(y - ref).max() <= 1e-13 * np.abs(ref).max(), (a, b, c)

    # 2. complex COCG, rtol and atol deciding
    a, b, c = 1.0, 0.5 * h2, 0.3 * h2
    rhs = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    for rtol in (1e-6, 1e-10):
        _check_solve(sysm, a, b, c, rhs, rtol, 0.0, 2, what="complex")
    bn = float(np.linalg.norm(rhs))
    if n > 8:  # (a system of a few nodes is solved exactly in n iterations: no atol can decide)
        _check_solve(sysm, a, b, c, rhs, 1e-10, 1e-6 * bn, 3, what="complex atol")

    # 3. the real instantiation (c = 0, no imaginary fields), and the complex one on the same real system
    rhs_r = rng.standard_normal(n)
    for rtol in (1e-6, 1e-10):
        xreal, _ = _check_solve(sysm, a, b, 0.0, rhs_r, rtol, 0.0, 2, cplx=False, what="real")
        xc, resc = sysm.solve(a, b, 0.0, rhs_r + 0j, rtol, 0.0, 500, cplx=True)
        assert np.abs(xc.real - xreal).max() <= 1e-12 * np.abs(xreal).max()
        assert np.all(xc.imag == 0.0)
    if n > 8:
        _check_solve(sysm, a, b, 0.0, rhs_r, 1e-10, 1e-6 * float(np.linalg.norm(rhs_r)), 3, cplx=False, what="real atol")

    # 4. stage right-hand sides r = sum_m gamma_m w_m - K sum_j s_j y_j
    W = [sysm.field(("w", m), rng.standard_normal(n)) for m in range(8)]
    Y = [sysm.field(("y", j), rng.standard_normal(n)) for j in range(8)]
    Wh = [f.numpy().astype(sysm.rdt) for f in W]
    Yh = [f.numpy().astype(sysm.rdt) for f in Y]
    Kd = sysm.K.astype(sysm.rdt)
    absK = abs(sysm.K)
    rr_, ri_ = sysm.field("rr"), sysm.field("ri")
    combos = ((0, 0), (1, 0), (0, 1), (1, 3), (3, 1), (3, 8), (8, 3), (8, 8)) if n <= BIG else ((0, 1), (3, 8), (8, 8))
    for nw, ny in combos:
        g = rng.standard_normal(nw) + 1j * rng.standard_normal(nw)
        s = rng.standard_normal(ny) + 1j * rng.standard_normal(ny)
        rr_.fill(np.nan)
        ri_.fill(np.nan)
        sysm.ops.rhs(W[:nw], g, Y[:ny], s, rr_, ri_)
        got = rr_.numpy() + 1j * ri_.numpy()
        ref = np.zeros(n, dtype=sysm.cdt)
        scale = np.zeros(n)
        for m in range(nw):
            ref += sysm.cdt(g[m]) * Wh[m]
            scale += abs(g[m]) * np.abs(W[m].numpy())
        if ny:
            ysum = sum(sysm.cdt(s[j]) * Yh[j] for j in range(ny))
            ref -= Kd @ ysum
            scale += absK @ sum(abs(s[j]) * np.abs(Y[j].numpy()) for j in range(ny))
        ref = np.asarray(ref, dtype=np.complex128)
        assert np.abs(got - ref).max() <= 1e-13 * max(scale.max(), 1e-300), (nw, ny)
    # the real-only call: r_im = NULL, real coefficients
    g, s = rng.standard_normal(3), rng.standard_normal(3)
    rr_.fill(np.nan)
    sysm.ops.rhs(W[:3], g, Y[:3], s, rr_, None)
    ref = sum(g[m] * Wh[m] for m in range(3)) - Kd @ sum(s[j] * Yh[j] for j in range(3))
    scale = sum(abs(g[m]) * np.abs(W[m].numpy()) for m in range(3)) + absK @ sum(abs(s[j]) * np.abs(Y[j].numpy()) for j in range(3))
    assert np.abs(rr_.numpy() - np.asarray(ref, dtype=np.float64)).max() <= 1e-13 * scale.max()

    # 5. the final update v += sum_i Re(d_i u_i)
    _check_update(sysm, rng)


def _check_update(sysm, rng):
    """Random data: |v| < 0.9 with max|v| in [0.5, 0.9), so every partial sum stays in the binade of max|v| and each fma
    rounds by at most half an ulp of it: bound n_fma / 2 ulp (4 ulp up to 8 terms).  Dyadic data, whose every partial
    sum is exact in binary64: bit-equal to the exact update."""
    n, lib, hd = sysm.n, sysm.lib, sysm.handle
    vf = sysm.field("v")
    U_re = [sysm.field(("ure", k)) for k in range(8)]
    U_im = [sysm.field(("uim", k)) for k in range(8)]
    layouts = {0: [], 1: [True], 3: [True, False, True], 8: [True, False, False, True, True, False, True, False]}
    for dyadic in (False, True):
        for nu, cplx in layouts.items():
            if dyadic:
                v = rng.integers(-2**30, 2**30, n) * 2.0**-20
                ure = [rng.integers(-2**20, 2**20, n) * 2.0**-20 for _ in range(nu)]
                uim = [rng.integers(-2**20, 2**20, n) * 2.0**-20 for _ in range(nu)]
                d = rng.integers(-8, 8, nu) * 0.25 + 1j * rng.integers(-8, 8, nu) * 0.25
            else:
                v = rng.uniform(-0.9, 0.9, n)
                v[rng.integers(n)] = 0.89
                ure = [1e-3 * rng.standard_normal(n) for _ in range(nu)]
                uim = [1e-3 * rng.standard_normal(n) for _ in range(nu)]
                d = rng.uniform(-1, 1, nu) + 1j * rng.uniform(-1, 1, nu)
            vf.set(v)
            for k in range(nu):
                U_re[k].set(ure[k])
                U_im[k].set(uim[k])
            sysm.ops.update(vf, U_re[:nu], [U_im[k] if cplx[k] else None for k in range(nu)], d)
            got = vf.numpy()
            if nu == 0:
                assert np.array_equal(got.view(np.int64), v.view(np.int64))
                continue
            ref = v.astype(np.longdouble)
            for k in range(nu):
                ref += np.longdouble(d[k].real) * ure[k]
                if cplx[k]:
                    ref -= np.longdouble(d[k].imag) * uim[k]
            err = np.abs(got - np.asarray(ref, dtype=np.float64))
            if dyadic:
                assert err.max() == 0.0, nu
            else:
                n_fma = nu + sum(cplx)
                assert err.max() <= max(4.0, n_fma / 2) * np.spacing(np.abs(v).max()), (nu, err.max() / np.spacing(np.abs(v).max()))
    # a NULL array of imaginary fields
    vf.set(v)
    _hip_update(lib, hd, vf, U_re[:2], None, [0.5, -0.25], [3.0, 3.0])
    ref = v + 0.5 * U_re[0].numpy() - 0.25 * U_re[1].numpy()
    assert np.abs(vf.numpy() - ref).max() <= 4 * np.spacing(np.abs(v).max())


def _hip_update(lib, hd, v, ure, uim, dre, dim):
    from beat import _hip

    k = len(ure)
    up = (C.c_void_p * k)(*[f.ptr for f in ure])
    ui = None if uim is None else (C.c_void_p * k)(*[None if f is None else f.ptr for f in uim])
    _hip.check(lib.beat_pde_rk_update(hd, v.ptr, up, ui, (C.c_double * k)(*dre), (C.c_double * k)(*dim), k))


def _rtol_for(rel, target):
    """(rtol, its): the first iteration count `its` >= target whose rr / bb (rel[k] after iteration k + 1) is a new low
    by a margin of 20 % -- COCG's residual is not monotone -- and an rtol whose stopping test is met first there, rtol^2
    half-way (geometrically) between that rr / bb and the smallest before it."""
    for its in range(max(target, 2), len(rel) + 1):
        lo, hi = rel[its - 1], min(rel[: its - 1])
        if hi > 1.2 * lo:
            return float(np.sqrt(np.sqrt(lo * hi))), its
    raise AssertionError(f"no clear new low of the residual from iteration {target} on")


def test_chunked_enqueue_over_a_sequence_of_solves(hip_ctx):
    """One handle, solves of varying difficulty in a row (~60 iterations, 3, a zero right-hand side, ~60): every count is
    the host's, whatever chunk the previous solve left (z_last_iters); max_it equal to the count changes nothing (the
    latched surplus launches are empty); a solve cut short at max_it in {1, 4, 16, 17} stops at exactly that iterate."""
    sysm = _System(hip_ctx, (41, 23, 9), "aniso3")
    n, h2 = sysm.n, sysm.h2
    a, b, c = 1.0, 20.0 * h2, 8.0 * h2
    S = sysm.S(a, b, c)
    rng = np.random.default_rng(5)
    rhs = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    # relative residuals of the host iteration with no stopping test
    full = jacobi_cocg(S, rhs, 1e-30, 0.0, 200, sysm.cdt)
    rel = [hk * 1e-60 for hk in full[5]]  # rr / bb (history = rr / tol^2, tol^2 = 1e-60 bb)
    (r60, n60), (r3, n3) = _rtol_for(rel, 60), _rtol_for(rel, 3)
    assert 60 <= n60 < 80 and n3 == 3, (n60, n3)
    seq = [(rhs, r60, n60), (rhs, r3, 3), (np.zeros(n, complex), 1e-8, 0), (1j * rhs, r60, n60), (rhs, r3, 3), (rhs, r60, n60)]
    for k, (f, rtol, its) in enumerate(seq):
        x, res = sysm.solve(a, b, c, f, rtol, 0.0, 500)
        assert res.iterations == its and res.converged_reason == 2, (k, res)
        xh = jacobi_cocg(S, f, rtol, 0.0, 500, sysm.cdt)
        assert xh[1] == its
        if its:
            xh = np.asarray(xh[0], dtype=complex)
            assert np.abs(x - xh).max() <= 1e-9 * np.abs(xh).max(), k
        else:
            assert np.all(x == 0.0)
    # max_it = the solve's own count: bit-identical x, same reason
    x1, res1 = sysm.solve(a, b, c, rhs, r60, 0.0, 500)
    x2, res2 = sysm.solve(a, b, c, rhs, r60, 0.0, res1.iterations)
    assert res2.iterations == res1.iterations == n60 and res2.converged_reason == res1.converged_reason == 2
    assert np.array_equal(x1.view(np.float64), x2.view(np.float64))
    # cut short: reason -3 at exactly max_it iterations, the host's iterate
    for mi in (1, 4, 16, 17):
        for prev in (3, 60):  # after a short and after a long solve (the first chunk differs)
            sysm.solve(a, b, c, rhs, r3 if prev == 3 else r60, 0.0, 500)
            x, res = sysm.solve(a, b, c, rhs, r60, 0.0, mi)
            assert res.converged_reason == -3 and res.iterations == mi, (mi, prev, res)
            xh = np.asarray(_host_at(S, rhs, mi, sysm.cdt), dtype=complex)
            assert np.abs(x - xh).max() <= 1e-9 * np.abs(xh).max(), (mi, prev)


def test_degenerate_right_hand_sides(hip_ctx):
    """Zero and 1e-300 right-hand sides (a sum of squares that is 0) return x = 0 at once; a purely imaginary one is i times
    the real one's; scalings by 1e-150 and 1e100 (sums of squares near the ends of the exponent range, finite) scale x."""
    sysm = _System(hip_ctx, (70, 33, 5), "aniso3")
    n, h2 = sysm.n, sysm.h2
    a, b, c = 1.0, 3.0 * h2, 1.5 * h2
    rng = np.random.default_rng(11)
    unit = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    seven = np.full(n, 7.0)
    for cplx in (True, False):
        c_ = c if cplx else 0.0
        f0 = unit if cplx else unit.real
        for z in (np.zeros(n), 1e-300 * f0):
            x, res = sysm.solve(a, b, c_, z, 1e-8, 0.0, 100, cplx=cplx, x0=seven)
            assert res.iterations == 0 and res.converged_reason > 0, (cplx, res)
            assert np.all(x == 0.0)
        x1, r1 = sysm.solve(a, b, c_, f0, 1e-6, 0.0, 200, cplx=cplx)
        xh = jacobi_cocg(sysm.S(a, b, c_), f0, 1e-6, 0.0, 200, sysm.cdt if cplx else sysm.rdt)
        assert r1.converged_reason == 2 and r1.iterations == xh[1] > 0
        for scale in (1e-150, 1e100):
            xs, rs = sysm.solve(a, b, c_, scale * f0, 1e-6, 0.0, 200, cplx=cplx)
            assert rs.converged_reason == 2 and rs.iterations == r1.iterations, (scale, cplx, rs)
            assert np.isfinite(xs).all()
            assert np.abs(xs - scale * x1).max() <= 1e-9 * scale * np.abs(x1).max(), (scale, cplx)
            assert abs(rs.rhs_norm - scale * r1.rhs_norm) <= 1e-10 * scale * r1.rhs_norm
    # purely imaginary right-hand side: x = i x(real right-hand side)
    xr_, rr_ = sysm.solve(a, b, c, unit.real + 0j, 1e-8, 0.0, 200)
    xi_, ri_ = sysm.solve(a, b, c, 1j * unit.real, 1e-8, 0.0, 200)
    assert ri_.iterations == rr_.iterations and ri_.converged_reason == 2
    assert np.abs(xi_ - 1j * xr_).max() <= 1e-12 * np.abs(xr_).max()
    _check_solve(sysm, a, b, c, 1j * unit.real, 1e-8, 0.0, 2, what="imaginary")


def test_refused_arguments_leave_outputs_untouched(hip_ctx):
    """Every argument the stage kernels refuse returns BEAT_EINVAL before anything is enqueued."""
    from beat import _hip, _stencil
    from beat._engine import HipOps

    sysm = _System(hip_ctx, (9, 7, 5), "aniso3")
    n, lib, hd = sysm.n, sysm.lib, sysm.handle
    rng = np.random.default_rng(2)
    fs = {k: sysm.field(k, rng.standard_normal(n), poison=False) for k in ("p", "q", "s", "t")}
    snap = {k: f.numpy().copy() for k, f in fs.items()}
    work = C.c_void_p(sysm.ops.work.data_ptr())
    P = lambda k: fs[k].ptr  # noqa: E731

    def untouched():
        hip_ctx.synchronize()
        for k, f in fs.items():
            assert np.array_equal(f.numpy(), snap[k]), k

    def info():
        i = _hip.KspInfo()
        i.iterations, i.converged_reason, i.residual_norm, i.rhs_norm = 12345, 777, -1.0, -2.0
        return i

    def info_untouched(i):
        assert (i.iterations, i.converged_reason, i.residual_norm, i.rhs_norm) == (12345, 777, -1.0, -2.0)

    # the four aliasings of the apply
    for xre, xim, yre, yim in (("p", "q", "p", "s"), ("p", "q", "s", "q"), ("p", "q", "s", "p"), ("p", "q", "q", "s")):
        assert lib.beat_pde_zapply(hd, 1.0, 0.1, 0.1, P(xre), P(xim), P(yre), P(yim)) == BEAT_EINVAL, (xre, xim, yre, yim)
        untouched()

    def zsolve(handle, c, rim, xim, max_it):
        i = info()
        rc = lib.beat_pde_zsolve(handle, 1.0, 0.1, c, P("p"), rim, P("s"), xim, work, 1e-8, 0.0, max_it, C.byref(i))
        info_untouched(i)
        untouched()
        return rc

    assert zsolve(hd, 0.1, None, None, 10) == BEAT_EINVAL  # c != 0 without x_im
    assert zsolve(hd, 0.0, P("q"), None, 10) == BEAT_EINVAL  # an imaginary right-hand side without x_im
    assert zsolve(hd, 0.1, None, P("t"), 10) == BEAT_EINVAL  # x_im without rhs_im
    assert zsolve(hd, 0.1, P("q"), P("t"), 0) == BEAT_EINVAL  # max_it = 0

    # 9 fields; a complex coefficient with r_im = NULL
    ptr9 = (C.c_void_p * 9)(*([P("p").value] * 9))
    one9 = (C.c_double * 9)(*([1.0] * 9))
    zero9 = (C.c_double * 9)(*([0.0] * 9))
    assert lib.beat_pde_rk_rhs(hd, ptr9, one9, zero9, 9, ptr9, one9, zero9, 0, P("s"), P("t")) == BEAT_EINVAL
    assert lib.beat_pde_rk_rhs(hd, ptr9, one9, zero9, 0, ptr9, one9, zero9, 9, P("s"), P("t")) == BEAT_EINVAL
    assert lib.beat_pde_rk_update(hd, P("s"), ptr9, ptr9, one9, zero9, 9) == BEAT_EINVAL
    untouched()
    im = (C.c_double * 9)(*([0.0] * 7 + [0.5, 0.0]))
    im0 = (C.c_double * 9)(*([0.5] + [0.0] * 8))
    assert lib.beat_pde_rk_rhs(hd, ptr9, one9, im0, 1, ptr9, one9, zero9, 0, P("s"), None) == BEAT_EINVAL
    assert lib.beat_pde_rk_rhs(hd, ptr9, one9, zero9, 0, ptr9, one9, im0, 1, P("s"), None) == BEAT_EINVAL
    assert lib.beat_pde_rk_rhs(hd, ptr9, one9, im, 8, ptr9, one9, zero9, 1, P("s"), None) == BEAT_EINVAL
    untouched()

    # handles the stage kernels do not take: per-node rows, a slab without its low physical face, an open theta-rule solve
    nn = (9, 7, 5)
    cells = tuple(v - 1 for v in nn)
    M = np.diag([1.0, 0.5, 0.25])
    per_node = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_fields(3, cells, (H,) * 3, M), per_node=True)
    mt, kt = _stencil.stencil_tables(3, (H,) * 3, M)
    slab = C.c_void_p()
    _hip.check(lib.beat_pde_create(hip_ctx.handle, (C.c_int64 * 3)(*nn), 0, 1, np.ascontiguousarray(mt).ctypes.data_as(C.c_void_p),
                                   np.ascontiguousarray(kt).ctypes.data_as(C.c_void_p), C.byref(slab)))
    theta = HipOps(hip_ctx, nn, True, True, mt, kt)
    theta.set_small(False)  # (the one-launch path of small grids does not open a solve)
    theta.set_timestep(0.01, 0.5, 0.05)
    assert theta.can_open()
    v = theta.new_field()
    v.set(rng.standard_normal(n))
    x = theta.new_field()
    theta.solve_begin(v, [], [], x, 1e-8, 0.0, 100)
    try:
        for handle in (per_node.handle, slab, theta.handle):
            assert lib.beat_pde_zapply(handle, 1.0, 0.1, 0.1, P("p"), P("q"), P("s"), P("t")) == BEAT_EINVAL
            untouched()
            assert zsolve(handle, 0.1, P("q"), P("t"), 10) == BEAT_EINVAL
            assert lib.beat_pde_rk_rhs(handle, ptr9, one9, zero9, 1, ptr9, one9, zero9, 1, P("s"), P("t")) == BEAT_EINVAL
            assert lib.beat_pde_rk_update(handle, P("s"), ptr9, None, one9, zero9, 1) == BEAT_EINVAL
            untouched()
    finally:
        res = theta.solve_finish()
        _hip.check(lib.beat_pde_destroy(slab))
    assert res.converged_reason > 0
    # the closed handle takes the stage kernels again
    _hip.check(lib.beat_pde_zapply(theta.handle, 1.0, 0.1, 0.1, P("p"), P("q"), P("s"), P("t")))
