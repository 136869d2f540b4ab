"""CPU: the ionic kernels' math layer -- FastMath's exp and log, the GRL1 polynomials phi_small / phi7 of TP06 and ToR-ORd, and the
gate / GRL1 updates built from them -- as the host build of the very source the device compiles (csrc/beat_math_probe.h through
tests/math_host_harness.cpp, g++ -ffp-contract=off) against mpmath (50 digits) and long double, with the bounds and special
values tests/test_device_math_gpu.py holds the device to.  The reciprocal estimates are 1/x on the host: their rows are GPU-only."""
import numpy as np
import pytest

from beat import _hip

import _device_math as dm

N_DENSE = 4_000_000
N_MP = 20_000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    run = dm.build_host(tmp_path_factory.mktemp("math_host"))
    if run is None:
        pytest.skip("no g++ on this machine")
    return run


@pytest.mark.parametrize("fn", [_hip.MATH_EXP, _hip.MATH_EXP_INT])
def test_exp_within_1p5_ulp(host, fn):
    """exp: <= 1.5 ulp over the normal range, <= 1.5 * 2^-1074 where the result is subnormal (host form, both flavours: the
    integer-add scaling is device-only).  Measured: 1.31 ulp (4 M points), 1.08 * 2^-1074."""
    ulp, sub, at = dm.check_exp(host, fn, dm.exp_edges(), mp=True)
    assert ulp <= dm.EXP_ULP and sub <= dm.EXP_SUB, (ulp, sub, at)
    ulp, sub, at = dm.check_exp(host, fn, dm.exp_random(N_MP, 1), mp=True)
    assert ulp <= dm.EXP_ULP, (ulp, at)
    if dm.LONG_OK:
        ulp, sub, at = dm.check_exp(host, fn, dm.exp_random(N_DENSE, 2))
        assert ulp <= dm.EXP_ULP, (ulp, at)
        ulp, sub, at = dm.check_exp(host, fn, dm.exp_random(N_DENSE // 8, 3, dm.EXP_LAST, dm.EXP_NORMAL_LO))
        assert ulp <= dm.EXP_ULP and sub <= dm.EXP_SUB, (ulp, sub, at)


def test_exp_special_values(host):
    """exp never makes a non-finite argument finite: +-inf and NaN give NaN (r = inf - inf in the reduction); the ldexp form
    overflows to inf above ln(DBL_MAX) and underflows to 0 below -745.13, as libm does."""
    x = np.array([np.inf, -np.inf, np.nan, dm.nxt(dm.EXP_OVF), 710.0, 1000.0, -746.0, -1e5, 0.0, -0.0])
    got = host(_hip.MATH_EXP, [x])[0]
    assert np.isnan(got[:3]).all(), got
    assert np.array_equal(got[3:], [np.inf, np.inf, np.inf, 0.0, 0.0, 1.0, 1.0]), got


@pytest.mark.parametrize("fn", [_hip.MATH_LOG, _hip.MATH_LOG_INT])
def test_log_absolute_error(host, fn):
    """log: |error| <= 2 * 2^-53 max(|log x|, 1) over positive normal and subnormal x (the table does not centre on 1: the
    relative error next to 1 is larger, the absolute one is not).  Measured: 1.58 at x = 3.4, i.e. 0.96 ulp of the result --
    one unit of 2^-53 max(|log x|, 1) is half an ulp where |log x| is in [1, 2), which only a correctly rounded log keeps."""
    e, at = dm.check_log(host, fn, dm.log_edges(), mp=True)
    assert e <= dm.LOG_UNIT, (e, at)
    e, at = dm.check_log(host, fn, dm.log_random(N_MP, 4), mp=True)
    assert e <= dm.LOG_UNIT, (e, at)
    if dm.LONG_OK:
        e, at = dm.check_log(host, fn, dm.log_random(N_DENSE, 5))
        assert e <= dm.LOG_UNIT, (e, at)


def test_log_special_values(host):
    """log has libm's semantics outside (0, inf): -inf at +-0, +inf at +inf, NaN for negative x, -inf and NaN -- a diverged
    concentration stays visibly diverged.  Subnormal x are normalised (log(1e-310) = -713.80, not -709.09)."""
    x = np.array([0.0, -0.0, np.inf, np.nan, -2.0, -1e-310, -np.inf, -dm.DBL_MAX, -dm.TINY, 1e-310, dm.TINY])
    got = host(_hip.MATH_LOG, [x])[0]
    assert np.array_equal(got[:3], [-np.inf, -np.inf, np.inf]), got
    assert np.isnan(got[3:9]).all(), got
    assert abs(got[9] - np.log(1e-310)) < 1e-13 and abs(got[10] - np.log(dm.TINY)) < 1e-13, got


@pytest.mark.parametrize("fn,w", [(_hip.MATH_TP06_PHI_SMALL, 1 / 16), (_hip.MATH_TP06_PHI7, 1 / 32),
                                  (_hip.MATH_TORORD_PHI_SMALL, 1 / 16), (_hip.MATH_TORORD_PHI7, 1 / 32)])
def test_phi_polynomials_within_1_ulp(host, fn, w):
    """phi(z) = (exp(z) - 1) / z by its Taylor polynomial over the window the kernels use it in (|z| <= 1/16 for the degree-8
    phi_small, 1/32 for the degree-7 phi7), both ends and 0 included.  Measured: 0.551 / 0.529 ulp."""
    edges, rnd = dm.phi_inputs(w, N_MP, 6)
    for z in (edges, rnd):
        e, at = dm.check_phi(host, fn, z, mp=True)
        assert e <= dm.PHI_ULP, (e, at)
    if dm.LONG_OK:
        e, at = dm.check_phi(host, fn, np.random.default_rng(7).uniform(-w, w, N_DENSE))
        assert e <= dm.PHI_ULP, (e, at)


COMPOSITES = [(_hip.MATH_TP06_GRL1, "grl1"), (_hip.MATH_TP06_ADVANCE, "grl1"), (_hip.MATH_TP06_GATE, "gate"),
              (_hip.MATH_TORORD_ADVANCE, "grl1"), (_hip.MATH_TORORD_GATE, "gate"), (_hip.MATH_TORORD_GATE_B, "gate_b")]


@pytest.mark.parametrize("fn,kind", COMPOSITES)
def test_composite_updates_against_the_literal_scheme(host, fn, kind):
    """The gate and GRL1 updates against mpmath's value of the scheme's literal y + f (exp(J dt) - 1) / J (f dt where |J| <=
    1e-8; gates y + (inf - y)(1 - exp(-dt rate))), at |J dt| = 1/16 +- ulp, |J| = 1e-8 +- ulp and J dt from -800 to 800:
    within 4 ulp of the increment + 1 ulp of the result + what exp()'s 1.5 ulp become through exp(z) - 1 (|f/J| ulp(exp);
    the polynomial windows do not have that term, the literal form outside them does).  Where exp(J dt) overflows in double
    the scheme -- and the oracle -- give +-inf, and so must the kernels.  (Before the exp clamp followed the flavour, TP06's
    updates at J dt in (709, 709.78] were those of J dt = 709: 40 % low.)"""
    k = "gate" if kind.startswith("gate") else "grl1"
    y, f, J, dt = dm.composite_inputs(k, 8)
    if kind == "gate_b":  # the polynomial branch: only where the kernel takes it (dt * bound <= 1/32)
        keep = J * dt <= 1 / 32
        y, f, J, dt = y[keep], f[keep], J[keep], dt[keep]
    got = host(fn, [y, f, J, dt])[0]
    ref, inc, cexp, cswitch = dm.composite_reference(k, y, f, J, dt)
    e = dm.composite_errors(got, ref, inc, cexp, cswitch)
    i = int(np.argmax(e))
    assert e.max() <= 1.0, (float(e[i]), y[i], f[i], J[i], dt[i], got[i], ref[i])
