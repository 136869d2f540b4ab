"""GPU: the ionic kernels' math layer on the device (beat_math_probe: csrc/beat_math_probe.h evaluated by one thread per column, with
FastMath staged and pinned as ode_step_kernel does) against mpmath (50 digits) and long double -- exp, log, the reciprocal
estimates beat_rcp / beat_rsqrt and the batched rcp2/3/4 of TP06 and ToR-ORd, the GRL1 polynomials and the gate / GRL1 updates --
and against the host build of the same source (tests/math_host_harness.cpp), bit for bit.  The host-form bounds are in
tests/_device_math.py; the docstrings give the maxima measured on an MI355X."""
import numpy as np
import pytest

from beat import _hip

import _device_math as dm

pytestmark = pytest.mark.gpu

N_DENSE = 4_000_000
N_MP = 20_000


@pytest.fixture(scope="module")
def dev(hip_ctx):
    import ctypes as C

    import torch

    ctx = hip_ctx

    def run(fn, rows):
        rows = [np.ascontiguousarray(r, dtype=np.float64) for r in rows]
        n = len(rows[0])
        assert len(rows) == _hip.MATH_IN[fn] and all(len(r) == n for r in rows) and n > 0
        ld = n + (-n) % 32
        a = np.zeros((len(rows), ld))
        for k, r in enumerate(rows):
            a[k, :n] = r
        din = torch.from_numpy(a).cuda()
        dout = torch.full((_hip.MATH_OUT[fn], ld), 12345.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _hip.check(ctx.lib.beat_math_probe(ctx.handle, fn, C.c_void_p(din.data_ptr()), ld, C.c_void_p(dout.data_ptr()), n))
        ctx.synchronize()
        out = dout.cpu().numpy()
        assert (out[:, n:] == 12345.0).all()  # nothing written past column n
        return list(out[:, :n].copy())

    return run


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return dm.build_host(tmp_path_factory.mktemp("math_host_gpu"))  # None without g++: the bit-identity test skips


def test_probe_rejects_bad_arguments(hip_ctx):
    import ctypes as C

    import torch

    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert hip_ctx.lib.beat_math_probe(hip_ctx.handle, 22, p, 8, p, 8) != 0
    assert hip_ctx.lib.beat_math_probe(hip_ctx.handle, -1, p, 8, p, 8) != 0
    assert hip_ctx.lib.beat_math_probe(hip_ctx.handle, 0, p, 4, p, 8) != 0  # ld < n
    assert hip_ctx.lib.beat_math_probe(hip_ctx.handle, 0, None, 8, p, 8) != 0


@pytest.mark.parametrize("fn", [_hip.MATH_EXP, _hip.MATH_EXP_INT])
def test_exp_within_1p5_ulp(dev, fn):
    """exp: <= 1.5 ulp (normal results), <= 1.5 * 2^-1074 (subnormal results, ldexp flavour); FastMathT<true> only over its
    normal range [-708, 709].  MI355X: 1.311 ulp (4 M points), 1.08 * 2^-1074; FastMathT<true> 1.325 ulp."""
    lo, hi = (-708.0, 709.0) if fn == _hip.MATH_EXP_INT else (dm.EXP_LAST, dm.EXP_OVF)
    x = dm.exp_edges()
    ulp, sub, at = dm.check_exp(dev, fn, x[(x >= lo) & (x <= hi)], mp=True)
    assert ulp <= dm.EXP_ULP and sub <= dm.EXP_SUB, (ulp, sub, at)
    ulp, sub, at = dm.check_exp(dev, fn, dm.exp_random(N_MP, 1, max(lo, dm.EXP_NORMAL_LO), hi), mp=True)
    assert ulp <= dm.EXP_ULP, (ulp, at)
    if dm.LONG_OK:
        ulp, sub, at = dm.check_exp(dev, fn, dm.exp_random(N_DENSE, 2, max(lo, dm.EXP_NORMAL_LO), hi))
        assert ulp <= dm.EXP_ULP, (ulp, at)
        if fn == _hip.MATH_EXP:
            ulp, sub, at = dm.check_exp(dev, fn, dm.exp_random(N_DENSE // 8, 3, dm.EXP_LAST, dm.EXP_NORMAL_LO))
            assert ulp <= dm.EXP_ULP and sub <= dm.EXP_SUB, (ulp, sub, at)


@pytest.mark.parametrize("fn", [_hip.MATH_LOG, _hip.MATH_LOG_INT])
def test_log_absolute_error(dev, fn):
    """log: |error| <= 2 * 2^-53 max(|log x|, 1), positive normal and subnormal x (the host form reaches 1.58 at x = 3.4, 0.96
    ulp of the result: the final rounding of a result in [1, 2) alone is up to one such unit).  MI355X: 1.58, the host's bits."""
    for x, mp in ((dm.log_edges(), True), (dm.log_random(N_MP, 4), True)) + (((dm.log_random(N_DENSE, 5), False),) if dm.LONG_OK else ()):
        e, at = dm.check_log(dev, fn, x, mp=mp)
        assert e <= dm.LOG_UNIT, (e, at)


@pytest.mark.parametrize("fn", [_hip.MATH_LOG, _hip.MATH_LOG_INT])
def test_log_special_values(dev, fn):
    """libm's semantics outside (0, inf): -inf at +-0, +inf at +inf, NaN for x < 0, -inf and NaN."""
    x = np.array([0.0, -0.0, np.inf, np.nan, -2.0, -1e-310, -np.inf, -dm.DBL_MAX, -dm.TINY, 1e-310, dm.TINY])
    got = dev(fn, [x])[0]
    assert np.array_equal(got[:3], [-np.inf, -np.inf, np.inf]), got
    assert np.isnan(got[3:9]).all(), got
    assert abs(got[9] - np.log(1e-310)) < 1e-13 and abs(got[10] - np.log(dm.TINY)) < 1e-13, got


def _specials():
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 1022, 2.0 ** 1023, dm.DBL_MAX, dm.TINY, dm.DBL_MIN / 2, -2.0])


def test_special_values_stay_non_finite(dev):
    """exp, beat_rcp and beat_rsqrt at +-0, +-inf, NaN and beyond their range: never a finite number where libm's is not,
    and the device's values there pinned."""
    x = _specials()
    pinned = {}
    with np.errstate(all="ignore"):
        for fn, name, lib in ((_hip.MATH_EXP, "exp", np.exp), (_hip.MATH_RCP, "rcp", lambda v: 1.0 / v),
                              (_hip.MATH_RSQRT, "rsqrt", lambda v: 1.0 / np.sqrt(v))):
            got = dev(fn, [x])[0]
            ref = lib(x)
            bad = ~np.isfinite(ref) & np.isfinite(got)
            assert not bad.any(), (name, x[bad], got[bad])
            pinned[name] = got
    # what the device returns (MI355X): NaN from the correction step's 0 * inf wherever v_rcp_f64 / v_rsq_f64 give 0 or inf --
    # rcp(+-0), rcp(+-inf), rcp of a subnormal (whose reciprocal overflows), rsqrt(+-0), rsqrt(+inf); exp(+-inf) and exp(NaN)
    # are NaN from the range reduction (inf - inf), and so is exp of a finite x beyond its 32-bit k range (callers clamp)
    nan = np.nan
    np.testing.assert_array_equal(pinned["rcp"][[0, 1, 2, 3, 4, 8]], [nan] * 6)
    np.testing.assert_array_equal(pinned["rsqrt"][[0, 1, 2, 3, 4, 10]], [nan] * 6)
    np.testing.assert_array_equal(pinned["exp"][[0, 1, 2, 3, 4]], [1.0, 1.0, nan, nan, nan])


def _rcp_inputs(n, seed):
    rng = np.random.default_rng(seed)
    pw = 2.0 ** np.arange(-1021, 1022, dtype=np.float64)
    edges = np.concatenate([pw, -pw, dm.around([1.0, -1.0, 3.0, 0.1, 1e300, 1e-300], 2)])
    rnd = np.exp2(rng.uniform(-1021, 1021, n)) * rng.choice([-1.0, 1.0], n)
    return edges, rnd


def _rel_ulp(got, ref_mp):
    return dm.err_mp(got, ref_mp)


def test_rcp_and_rsqrt_within_1_ulp(dev):
    """beat_rcp (v_rcp_f64 + one third-order step) and beat_rsqrt: <= 1 ulp where x and the result are normal.  MI355X: 0.5 ulp
    (correctly rounded on 4 M points) and 0.99 ulp."""
    edges, rnd = _rcp_inputs(N_MP, 9)
    for x in (edges, rnd):
        got = dev(_hip.MATH_RCP, [x])[0]
        e = _rel_ulp(got, [1 / mp for mp in (dm.mpmath.mpf(float(v)) for v in x)])
        assert e.max() <= dm.RCP_ULP, (e.max(), x[np.argmax(e)])
        xp = np.abs(x)
        got = dev(_hip.MATH_RSQRT, [xp])[0]
        e = _rel_ulp(got, [1 / dm.mpmath.sqrt(mp) for mp in (dm.mpmath.mpf(float(v)) for v in xp)])
        assert e.max() <= dm.RCP_ULP, (e.max(), xp[np.argmax(e)])
    if dm.LONG_OK:
        x = np.exp2(np.random.default_rng(10).uniform(-1021, 1021, N_DENSE))
        got = dev(_hip.MATH_RCP, [x])[0]
        e = dm.err_ld(got, 1 / x.astype(np.longdouble))
        assert e.max() <= dm.RCP_ULP, (e.max(), x[np.argmax(e)])
        got = dev(_hip.MATH_RSQRT, [x])[0]
        e = dm.err_ld(got, 1 / np.sqrt(x.astype(np.longdouble)))
        assert e.max() <= dm.RCP_ULP, (e.max(), x[np.argmax(e)])


def test_rcp_at_the_edge_of_the_range(dev):
    """1/x next to 2^+-1022 (subnormal or overflowing results) and at subnormal x: within 1 ulp (2^-1074 where the result is
    subnormal), or non-finite where the true reciprocal overflows."""
    x = np.concatenate([dm.around([2.0 ** 1022, -2.0 ** 1022, 2.0 ** 1023, 2.0 ** -1022, 2.0 ** -1023], 2), [dm.TINY, 1e-310, 1e-320]])
    got = dev(_hip.MATH_RCP, [x])[0]
    ref = [1 / dm.mpmath.mpf(float(v)) for v in x]
    ovf = np.array([abs(r) > dm.DBL_MAX for r in ref])
    e = dm.err_mp(np.where(ovf, 0.0, got), [0 if o else r for o, r in zip(ovf, ref)])
    assert (~np.isfinite(got[ovf])).all(), got[ovf]
    assert e[~ovf].max() <= dm.RCP_ULP, (e[~ovf].max(), x[~ovf][np.argmax(e[~ovf])])


@pytest.mark.parametrize("fn,k", [(_hip.MATH_TP06_RCP2, 2), (_hip.MATH_TP06_RCP3, 3), (_hip.MATH_TP06_RCP4, 4),
                                  (_hip.MATH_TORORD_RCP2, 2), (_hip.MATH_TORORD_RCP3, 3), (_hip.MATH_TORORD_RCP4, 4)])
def test_batched_reciprocals_within_2p5_ulp(dev, fn, k):
    """rcp2 / rcp3 / rcp4 (one v_rcp_f64 for two to four reciprocals) for factors of either sign up to 1e60 whose product stays
    normal -- their documented domain: <= 2.5 / 3.5 / 4 ulp per output.  (2.5 for all three does not hold even with a correctly
    rounded reciprocal: the host form, 1/x in place of the estimate, reaches 1.85 / 2.99 / 3.02 ulp -- every output carries the
    roundings of the product and of two more multiplications, 2.5 / 3.0 / 3.5 ulp to first order with the reciprocal's 1 ulp.)  MI355X: 1.90 / 3.15 / 3.15 ulp (1 M points)."""
    rng = np.random.default_rng(11 + k)
    n = N_MP
    rows = [np.exp(rng.uniform(np.log(1e-3), np.log(1e60), n)) * rng.choice([-1.0, 1.0], n) for _ in range(k)]
    rows[0][:8] = [1.0, 1.0, 1e60, 1e-3, 2.0, 0.5, 3.0, 7.0]
    got = dev(fn, rows)
    for j in range(k):
        e = dm.err_mp(got[j], [1 / dm.mpmath.mpf(float(v)) for v in rows[j]])
        assert e.max() <= dm.RCPN_ULP[k], (j, e.max(), rows[j][np.argmax(e)])


@pytest.mark.parametrize("fn,w", [(_hip.MATH_TP06_PHI_SMALL, 1 / 16), (_hip.MATH_TP06_PHI7, 1 / 32),
                                  (_hip.MATH_TORORD_PHI_SMALL, 1 / 16), (_hip.MATH_TORORD_PHI7, 1 / 32)])
def test_phi_polynomials_within_1_ulp(dev, fn, w):
    """(exp(z) - 1) / z by its Taylor polynomial over the kernels' windows, both ends and 0 included: <= 1 ulp.  MI355X: 0.551
    ulp (degree 8, |z| <= 1/16), 0.529 ulp (degree 7, |z| <= 1/32), TP06's and ToR-ORd's copies alike."""
    edges, rnd = dm.phi_inputs(w, N_MP, 6)
    for z in (edges, rnd):
        e, at = dm.check_phi(dev, fn, z, mp=True)
        assert e <= dm.PHI_ULP, (e, at)
    if dm.LONG_OK:
        e, at = dm.check_phi(dev, fn, np.random.default_rng(7).uniform(-w, w, N_DENSE))
        assert e <= dm.PHI_ULP, (e, at)


COMPOSITES = [(_hip.MATH_TP06_GRL1, "grl1"), (_hip.MATH_TP06_ADVANCE, "grl1"), (_hip.MATH_TP06_GATE, "gate"),
              (_hip.MATH_TORORD_ADVANCE, "grl1"), (_hip.MATH_TORORD_GATE, "gate"), (_hip.MATH_TORORD_GATE_B, "gate_b")]


@pytest.mark.parametrize("fn,kind", COMPOSITES)
def test_composite_updates_against_the_literal_scheme(dev, fn, kind):
    """The device's gate / GRL1 updates against mpmath's value of the scheme's literal expression, with the error budget of
    tests/test_device_math_host.py (4 ulp of the increment + 1 ulp of the result + exp's error through exp(z) - 1), J dt from
    -800 to 800 (+-inf where exp(J dt) overflows), |J dt| = 1/16 +- ulp, |J| = 1e-8 +- ulp."""
    k = "gate" if kind.startswith("gate") else "grl1"
    y, f, J, dt = dm.composite_inputs(k, 8)
    if kind == "gate_b":
        keep = J * dt <= 1 / 32
        y, f, J, dt = y[keep], f[keep], J[keep], dt[keep]
    got = dev(fn, [y, f, J, dt])[0]
    ref, inc, cexp, cswitch = dm.composite_reference(k, y, f, J, dt)
    e = dm.composite_errors(got, ref, inc, cexp, cswitch)
    i = int(np.argmax(e))
    assert e.max() <= 1.0, (float(e[i]), y[i], f[i], J[i], dt[i], got[i], ref[i])


BIT_IDENTICAL = [_hip.MATH_EXP, _hip.MATH_EXP_INT, _hip.MATH_LOG, _hip.MATH_LOG_INT, _hip.MATH_TP06_PHI_SMALL, _hip.MATH_TP06_PHI7,
                 _hip.MATH_TORORD_PHI_SMALL, _hip.MATH_TORORD_PHI7]


@pytest.mark.parametrize("fn", BIT_IDENTICAL)
def test_host_and_device_agree_bit_for_bit(dev, host, fn):
    """exp, log and the phi polynomials: the device's results are the host build's, bit for bit (NaN where NaN), on the same
    inputs -- what the CPU suite verifies of these sources is what the GPU runs.  FastMathT<true>::exp over [-708, 709] (its
    integer-add scaling is the ldexp scaling there)."""
    if host is None:
        pytest.skip("no g++ on this machine")
    rng = np.random.default_rng(12)
    if fn in (_hip.MATH_EXP, _hip.MATH_EXP_INT):
        lo, hi = (-708.0, 709.0) if fn == _hip.MATH_EXP_INT else (-800.0, 800.0)
        x = np.concatenate([dm.exp_edges(), rng.uniform(lo, hi, 1_000_000)])
        x = x[(x >= lo) & (x <= hi)]
        if fn == _hip.MATH_EXP:
            x = np.concatenate([x, [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e5, -1e5]])
    elif fn in (_hip.MATH_LOG, _hip.MATH_LOG_INT):
        x = np.concatenate([dm.log_edges(), dm.log_random(1_000_000, 13), [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, 1e-310, -1e-310]])
    else:
        w = 1 / 16 if fn in (_hip.MATH_TP06_PHI_SMALL, _hip.MATH_TORORD_PHI_SMALL) else 1 / 32
        edges, rnd = dm.phi_inputs(w, 1_000_000, 14)
        x = np.concatenate([edges, rnd])
    d, h = dev(fn, [x])[0], host(fn, [x])[0]
    same = (d.view(np.int64) == h.view(np.int64)) | (np.isnan(d) & np.isnan(h))
    assert same.all(), (int((~same).sum()), x[~same][:5], d[~same][:5], h[~same][:5])


def test_generated_model_fexp_against_mpmath(tmp_path):
    """The exp wrapper generated models call (beat/models/_ode_cxx.py: fexp = FastMath::exp of the clamped argument, NaN kept):
    forward Euler on dx/dt = 0, dy/dt = exp(x) from y = 0 with dt = 1 gives y' = fexp(x) exactly.  x over [-1e6, 1e3] and the
    exp edge points: <= 1.5 ulp (1.5 * 2^-1074 subnormal), 0 below -745.13, inf above 709.78, NaN for NaN."""
    from beat.models import from_ode

    f = tmp_path / "fexp.ode"
    f.write_text('parameters("P", a = 1.0)\nstates("S", x = 0.0, y = 0.0)\nexpressions("S")\ndx_dt = 0*a\ndy_dt = exp(x)\n')
    model = from_ode(f, name="fexp_probe", scheme="forward_euler", v_name="x")
    rng = np.random.default_rng(15)
    x = np.concatenate([dm.exp_edges(), rng.uniform(dm.EXP_LAST, dm.EXP_OVF, N_MP), rng.uniform(-1e6, 1e3, 2000),
                        dm.around([-1e6, 1e3, -745.2, 709.79, 710.0]), [np.nan, np.inf, -np.inf]])
    S = np.vstack([x, np.zeros_like(x)])
    got = model(states=S, t=0.0, parameters=model.init_parameter_values(), dt=1.0)[1]
    fin = np.isfinite(x)
    with np.errstate(over="ignore"):
        libm = np.exp(x)
    assert np.isnan(got[np.isnan(x)]).all()
    assert np.array_equal(got[fin & np.isinf(libm)], libm[fin & np.isinf(libm)])
    assert (got[fin & (x < dm.EXP_LAST - 1)] == 0.0).all()
    m = fin & (x >= dm.EXP_LAST) & (x <= dm.EXP_OVF)
    refs = dm.mp_map(dm.mpmath.exp, x[m])
    e = dm.err_mp(got[m], refs)
    r = np.array([float(v) for v in refs])
    sub = r < dm.DBL_MIN
    assert e[~sub].max() <= dm.EXP_ULP and (e[sub].max() if sub.any() else 0) <= dm.EXP_SUB, (e.max(), x[m][np.argmax(e)])
