"""Inputs, references and error measures for the tests of the ionic kernels' math layer (csrc/beat_math_probe.h): shared by
tests/test_device_math_host.py (the host build of the same source, tests/math_host_harness.cpp) and tests/test_device_math_gpu.py
(the device, through beat_math_probe).  ``run(fn, rows) -> rows`` evaluates helper ``fn`` (beat._hip.MATH_*) column by column.

References: mpmath at 50 digits for the edge points and a random sample, np.longdouble (64-bit mantissa) for the dense sweeps.
Errors are in ulps of the correctly rounded result (units of 2^-1074 where it is subnormal); log's is absolute, in units of
2^-53 max(|log x|, 1)."""
from __future__ import annotations

import math
import shutil
import subprocess
from pathlib import Path

import mpmath
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
mpmath.mp.dps = 50
TINY = 2.0 ** -1074
LN2 = math.log(2.0)
DBL_MIN = np.finfo(np.float64).tiny
DBL_MAX = np.finfo(np.float64).max
LONG_OK = np.finfo(np.longdouble).nmant >= 63  # x87 extended: dense sweeps against long double, otherwise mpmath only
EXP_NORMAL_LO = -708.3964185322641  # exp(x) >= DBL_MIN above this
EXP_LAST = -745.1332191019411  # the last x whose exp rounds to a nonzero double (2^-1074)
EXP_OVF = 709.782712893384  # ln(DBL_MAX), rounded

# the bounds (the host-form figures of the issue, rounded up); measured maxima in the tests' docstrings
EXP_ULP, EXP_SUB, LOG_UNIT, PHI_ULP, RCP_ULP, COMPOSITE_ULP = 1.5, 1.5, 2.0, 1.0, 1.0, 4.0
# rcp2 / rcp3 / rcp4, per output: the product's roundings, the reciprocal's ulp and two more products (first order: 2.5, 3.0, 3.5)
RCPN_ULP = {2: 2.5, 3: 3.5, 4: 4.0}


def nxt(x, k=1):
    x = np.asarray(x, dtype=np.float64)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def around(points, k=1):
    """each point and its k neighbours either side"""
    p = np.asarray(points, dtype=np.float64).ravel()
    return np.concatenate([p] + [nxt(p, j) for j in range(-k, k + 1) if j])


# ------------------------------------------------------------------------------------------------------------------- error
def ulp_of(r):
    """ulp of the correctly rounded result r (float64 array), 2^-1074 at subnormals and zero"""
    return np.maximum(np.spacing(np.abs(r)), TINY)


def err_ld(got, ref_ld):
    """error of float64 results against long double references, in ulps of the rounded reference"""
    r = ref_ld.astype(np.float64)
    return (np.abs(got.astype(np.longdouble) - ref_ld) / ulp_of(r).astype(np.longdouble)).astype(np.float64)


def err_mp(got, refs):
    """the same against mpmath values (list of mpf)"""
    out = np.empty(len(got))
    for i, (g, r) in enumerate(zip(got, refs)):
        rr = float(r)
        out[i] = float(abs(mpmath.mpf(float(g)) - r) / max(np.spacing(abs(rr)), TINY))
    return out


def mp_map(f, x):
    return [f(mpmath.mpf(float(v))) for v in x]


# ------------------------------------------------------------------------------------------------------------------- exp
def exp_edges():
    k = np.arange(-65536 * 2 - 1024, 65536 * 2 + 1024, 97, dtype=np.float64)
    bounds = (k + 0.5) * (LN2 / 256)  # where the rounding of x 256/ln2 switches table entry
    m = np.arange(-1021, 1024, dtype=np.float64)
    wrap = np.concatenate([m * LN2, m * LN2 - LN2 / 512])  # j = 255 -> 0 at every m ln2
    pts = np.concatenate([around(bounds), around(wrap), around([0.0, -0.0, 2.0 ** -60, -2.0 ** -60, EXP_NORMAL_LO, EXP_LAST,
                                                                 EXP_OVF, 1.0, -1.0, 700.0, -700.0])])
    return pts[(pts >= EXP_LAST) & (pts <= EXP_OVF)]


def exp_random(n, seed, lo=EXP_NORMAL_LO, hi=EXP_OVF):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def check_exp(run, fn, x, mp=False, lo=EXP_LAST):
    """max ulp error (normal results) and max error in 2^-1074 (subnormal results) of exp over x"""
    x = x[(x >= lo) & (x <= EXP_OVF)]
    got = run(fn, [x])[0]
    if mp:
        refs = mp_map(mpmath.exp, x)
        e = err_mp(got, refs)
        r = np.array([float(v) for v in refs])
    else:
        ref = np.exp(x.astype(np.longdouble))
        e = err_ld(got, ref)
        r = ref.astype(np.float64)
    sub = r < DBL_MIN
    return (float(e[~sub].max()) if (~sub).any() else 0.0), (float(e[sub].max()) if sub.any() else 0.0), x[np.argmax(e)]


# ------------------------------------------------------------------------------------------------------------------- log
def log_edges():
    i = np.arange(129, dtype=np.float64)
    pts = [1.0 + i / 128, 1.0 + (i + 0.5) / 128, [1.0, 1.0 + 1e-7, 1.0 - 1e-7, 0.5, 2.0, DBL_MIN, DBL_MAX, 1e-300, 1e300, 3.7e-5, 140.0]]
    pts = np.concatenate([np.asarray(p, dtype=np.float64) for p in pts])
    pts = np.concatenate([pts, pts * 2.0 ** -600, pts * 2.0 ** 500])
    sub = np.array([TINY, 2 * TINY, 3 * TINY, 1e-310, 1e-320, DBL_MIN / 2, DBL_MIN - TINY, 2.0 ** -1060])
    p = around(np.concatenate([pts, sub]))
    return p[(p > 0) & np.isfinite(p)]


def log_random(n, seed):
    rng = np.random.default_rng(seed)
    a = np.exp2(rng.uniform(-1022, 1024, n // 2))  # log-uniform over the normal range
    b = 1.0 + rng.uniform(-0.25, 0.25, n - n // 2) * np.exp2(rng.uniform(-52, 0, n - n // 2))  # next to 1
    x = np.concatenate([a, b])
    return x[np.isfinite(x) & (x > 0)]


def check_log(run, fn, x, mp=False):
    """max of |log error| / (2^-53 max(|log x|, 1))"""
    got = run(fn, [x])[0]
    if mp:
        refs = mp_map(mpmath.log, x)
        e = np.array([float(abs(mpmath.mpf(float(g)) - r) / (mpmath.mpf(2) ** -53 * max(abs(r), 1))) for g, r in zip(got, refs)])
    else:
        ref = np.log(x.astype(np.longdouble))
        e = (np.abs(got.astype(np.longdouble) - ref) / (np.longdouble(2.0 ** -53) * np.maximum(np.abs(ref), 1))).astype(np.float64)
    return float(e.max()), x[np.argmax(e)]


# ------------------------------------------------------------------------------------------------------------------- phi
def check_phi(run, fn, z, mp=False):
    """max ulp error of (exp(z) - 1)/z (1 at z = 0)"""
    got = run(fn, [z])[0]
    if mp:
        refs = [mpmath.expm1(v) / v if v != 0 else mpmath.mpf(1) for v in (mpmath.mpf(float(t)) for t in z)]
        e = err_mp(got, refs)
    else:
        zl = z.astype(np.longdouble)
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = np.where(zl == 0, np.longdouble(1), np.expm1(zl) / zl)
        e = err_ld(got, ref)
    return float(e.max()), z[np.argmax(e)]


def phi_inputs(w, n, seed):
    rng = np.random.default_rng(seed)
    edges = np.concatenate([around([w, -w, 0.0, 2.0 ** -30, -2.0 ** -30, w / 2, -w / 2]), [0.0, -0.0]])
    edges = edges[np.abs(edges) <= w]
    return edges, rng.uniform(-w, w, n)


# ------------------------------------------------------------------------------------------------------------------- composites
JDT = [-800.0, -746.0, -745.2, -708.5, -708.0, 0.0, 709.0, 709.5, 709.78, 709.79, 710.0, 800.0]


def composite_inputs(kind, seed):
    """(y, f-or-inf, J-or-rate, dt) columns at the edge points of the issue: |J dt| = 1/16 +- ulp, |J| = 1e-8 +- ulp and the
    J dt list above, each with a few y and f; kind 'gate' keeps the rate positive (exp's argument -dt rate <= 0)"""
    rng = np.random.default_rng(seed)
    rows = []
    dt16 = 0.25  # J dt = 1/16 exactly at J = 1/4
    for J in around([0.25, -0.25]):
        rows.append((J, dt16))
    for J in around([1e-8, -1e-8]):
        rows.append((J, 0.01))
    for z in JDT:
        rows.append((z, 1.0))  # dt = 1: J dt = J exactly
        rows.append((z / 0.05, 0.05))
    for z in rng.uniform(-2.0, 2.0, 64):
        rows.append((z / 0.01, 0.01))
    if kind == "gate":
        rows = [(-J, dt) for J, dt in rows if J < 0] + [(r, dt) for r, dt in rows if r > 0 and r * dt < 800]
    y0 = [0.0, 0.3, -1.0, 136.9]
    f0 = [1.0, -0.7, 1e-3]
    cols = [(y, f, J, dt) for J, dt in rows for y in y0 for f in f0]
    a = np.array(cols, dtype=np.float64).T
    return [np.ascontiguousarray(r) for r in a]


def composite_reference(kind, y, f, J, dt):
    """mpmath's value of the scheme's literal update, from the fp64 product J dt (the oracle and the kernels both round it
    first); where exp(J dt) overflows in double (libm) the fp64 value of the literal expression, as the oracle computes it
    (+-inf).  Returns (reference result, increment, |f / J| ulp(exp(J dt)) -- the part of the error budget exp()'s error
    becomes through exp(z) - 1 --, |f dt z| / 2 where |J| <= 1e-8 -- how far the scheme's switch to f dt there lies from
    the exact f (exp(z) - 1)/J that the polynomial form of advance() keeps evaluating), all float64"""
    n = len(y)
    ref, inc, cexp, cswitch = np.empty(n), np.empty(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        Y, F, X, D = (mpmath.mpf(float(v[i])) for v in (y, f, J, dt))
        if kind == "gate":  # y + (inf - y)(1 - exp(-dt rate))
            z = mpmath.mpf(float(-dt[i] * J[i]))
            e = mpmath.exp(z)
            d = (F - Y) * (1 - e)
            scale = abs(F - Y)
        else:
            z = mpmath.mpf(float(J[i] * dt[i]))
            e = mpmath.exp(z)
            if abs(X) <= mpmath.mpf("1e-8"):
                d, scale = F * D, mpmath.mpf(0)
                cswitch[i] = float(abs(F * D * z) / 2)
            else:
                d = F * (e - 1) / X
                scale = abs(F / X)
        with np.errstate(over="ignore"):
            ovf = not np.isfinite(np.exp(float(z)))
        if ovf:
            inc[i] = ref[i] = float(F) * np.inf * (1 if X > 0 else -1)
            continue
        ref[i] = float(Y + d)
        inc[i] = float(d)
        cexp[i] = float(scale * max(np.spacing(abs(float(e))), TINY))
    return ref, inc, cexp, cswitch


def composite_errors(got, ref, inc, cexp, cswitch):
    """|got - ref| in units of the bound: 4 ulp of the increment + 1 ulp of the result (its rounding and the rounded reference's)
    + exp()'s 1.5 ulp as exp(z) - 1 passes them on (|f/J| ulp(exp)) + the scheme's own switch at |J| <= 1e-8 (cswitch)"""
    both_inf = np.isinf(ref) & (got == ref)
    bound = COMPOSITE_ULP * ulp_of(inc) + ulp_of(ref) + EXP_ULP * cexp + cswitch
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.where(np.isfinite(bound), bound, np.inf)
    e[both_inf] = 0.0
    e[np.isnan(e)] = np.inf
    return e


# ------------------------------------------------------------------------------------------------------------------- host build
def build_host(tmp: Path):
    """g++ build of tests/math_host_harness.cpp; returns run(fn, rows) or None without g++"""
    if shutil.which("g++") is None:
        return None
    exe = tmp / "math_host"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-o", str(exe),
                    str(ROOT / "tests" / "math_host_harness.cpp")], check=True)

    def run(fn, rows):
        from beat import _hip

        rows = [np.ascontiguousarray(r, dtype=np.float64) for r in rows]
        n = len(rows[0])
        assert len(rows) == _hip.MATH_IN[fn] and all(len(r) == n for r in rows)
        np.concatenate(rows).tofile(tmp / "in.bin")
        res = subprocess.run([str(exe), str(fn), str(tmp / "in.bin"), str(tmp / "out.bin"), str(n)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        return list(np.fromfile(tmp / "out.bin").reshape(_hip.MATH_OUT[fn], n))

    return run
