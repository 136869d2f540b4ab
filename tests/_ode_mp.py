"""An independent evaluation of a gotran ``.ode`` file in mpmath (60 digits), for tests/test_ode_language_*.py.

The file's syntax is interpreted node by node with mpmath numbers, not through SymPy: Python's own meaning of ``%``,
comparisons, chained comparisons and ``and`` / ``or`` / ``not`` applies to numbers, as gotran intends.  Every value carries

* its derivative with respect to ONE state (forward mode: the total self-derivative J_ii that GRL1 needs, intermediates
  resolved, without a symbolic derivative), and
* a running-error magnitude for the value and for the derivative: the sum of the absolute sizes of the terms a double
  evaluation of the same formula rounds (first order; an input has magnitude 0).  An error bound of K ulp is then
  ``K * 2**-52 * magnitude`` (and one subnormal ulp), whatever cancellation the formula contains.

Real-valued semantics of double arithmetic: a result outside the real domain is NaN (log / sqrt of a negative number,
asin / acos outside [-1, 1], a negative base to a non-integer power), and a value beyond the largest double is an infinity."""
from __future__ import annotations

import ast
import os
from dataclasses import dataclass
from pathlib import Path

import mpmath
import numpy as np

DPS = 60
MPF = mpmath.mpf
ZERO, ONE = MPF(0), MPF(1)
NAN, INF = MPF("nan"), MPF("inf")
BIG = MPF(np.finfo(np.float64).max)
EPS = MPF(2) ** -52
TINY = MPF(2) ** -1074
GRL1_THRESHOLD = MPF(1e-8)


def _x(a, b):
    """a * b, 0 where either is 0 (an exact input's magnitude times an infinite sensitivity is no error)."""
    return ZERO if a == 0 or b == 0 else a * b


def _fin(v):
    if mpmath.isnan(v):
        return v
    return INF if v > BIG else (-INF if v < -BIG else v)


@dataclass
class Num:
    v: object           # value
    d: object = ZERO    # derivative with respect to the seeded state
    mv: object = ZERO   # running-error magnitude of v
    md: object = ZERO   # ... and of d

    def __bool__(self):
        return bool(self.v != 0)


def num(x) -> Num:
    if isinstance(x, Num):
        return x
    return Num(MPF(float(x)) if isinstance(x, (bool, int, float)) else MPF(x))


def _unary(x: Num, g, g1, g2, g1_terms=None) -> Num:
    """g(x) for g with first / second derivatives g1, g2 (values); g1_terms: the term size of the formula g1 is printed as."""
    v = _fin(g)
    d = _x(g1, x.d)
    mv = _x(abs(g1), x.mv) + abs(v)
    md = _x(abs(g1), x.md) + _x(abs(g1_terms if g1_terms is not None else g1), abs(x.d)) + _x(_x(abs(g2), abs(x.d)), x.mv) + abs(d)
    return Num(v, d, mv, md)


def _nan_like(x: Num) -> Num:
    return Num(NAN, NAN if x.d != 0 else ZERO, NAN, NAN)


def add(a, b) -> Num:
    a, b = num(a), num(b)
    v = _fin(a.v + b.v)
    d = a.d + b.d
    return Num(v, d, a.mv + b.mv + abs(v), a.md + b.md + abs(d))


def neg(a) -> Num:
    a = num(a)
    return Num(-a.v, -a.d, a.mv, a.md)


def mul(a, b) -> Num:
    a, b = num(a), num(b)
    v = _fin(a.v * b.v)
    d = _x(a.d, b.v) + _x(a.v, b.d)
    mv = _x(a.mv, abs(b.v)) + _x(abs(a.v), b.mv) + abs(v)
    md = (_x(a.md, abs(b.v)) + _x(abs(a.d), b.mv) + _x(a.mv, abs(b.d)) + _x(abs(a.v), b.md) + abs(_x(a.d, b.v)) + abs(_x(a.v, b.d))
          + abs(d))
    return Num(v, d, mv, md)


def recip(x) -> Num:
    x = num(x)
    if mpmath.isnan(x.v):
        return _nan_like(x)
    if x.v == 0:
        return Num(INF, ZERO if x.d == 0 else NAN, ZERO, ZERO)
    if mpmath.isinf(x.v):
        return Num(ZERO, ZERO, ZERO, ZERO)
    return _unary(x, ONE / x.v, -ONE / x.v ** 2, 2 / x.v ** 3)


def div(a, b) -> Num:
    a, b = num(a), num(b)
    if b.v == 0 and not mpmath.isnan(a.v):  # (x / 0: an infinity, or NaN for 0 / 0)
        return Num(NAN if a.v == 0 else INF, ZERO if a.d == b.d == 0 else NAN, ZERO, ZERO)
    return mul(a, recip(b))


def power(a, b) -> Num:
    a, b = num(a), num(b)
    if b.d != 0 or b.mv != 0:
        raise NotImplementedError("an exponent that is not an input or a literal")
    x, e = a.v, b.v
    if mpmath.isnan(x) or mpmath.isnan(e):
        return _nan_like(a)
    integer = e == mpmath.floor(e)
    if x < 0 and not integer:
        return _nan_like(a)
    if x == 0:
        if e < 0:
            return Num(INF, ZERO if a.d == 0 else NAN, ZERO, ZERO)
        return Num(ONE if e == 0 else ZERO, ZERO if a.d == 0 or e > 1 else NAN, ZERO, ZERO)
    p = (lambda k: mpmath.power(x, int(e) - k) if integer else mpmath.power(x, e - k))
    return _unary(a, p(0), e * p(1), e * (e - 1) * p(2))


def mod(a, b) -> Num:
    """Python's a % b: the result takes the divisor's sign."""
    a, b = num(a), num(b)
    if b.v == 0 or not (mpmath.isfinite(a.v) and mpmath.isfinite(b.v)):
        return _nan_like(a)
    k = mpmath.floor(a.v / b.v)
    v = a.v - k * b.v
    return Num(v, a.d - _x(k, b.d), a.mv + _x(b.mv, abs(k)) + abs(v), a.md + _x(b.md, abs(k)))


def floor(x) -> Num:
    x = num(x)
    if not mpmath.isfinite(x.v):
        return Num(x.v)
    return Num(mpmath.floor(x.v))


def absolute(x) -> Num:
    x = num(x)
    s = ONE if x.v > 0 else (-ONE if x.v < 0 else ZERO)
    if mpmath.isnan(x.v):
        return _nan_like(x)
    return Num(abs(x.v), _x(s, x.d), x.mv, x.md)


def _f(name):
    """The transcendental functions: value, first and second derivative, and the real domain."""
    def f(x):
        x = num(x)
        v = x.v
        if mpmath.isnan(v):
            return _nan_like(x)
        if name == "exp":
            if v > 1000:
                return Num(INF, ZERO if x.d == 0 else NAN, ZERO, ZERO)
            e = mpmath.exp(v)
            return _unary(x, e, e, e)
        if name == "log":
            if v < 0:
                return _nan_like(x)
            if v == 0:
                return Num(-INF, ZERO if x.d == 0 else NAN, ZERO, ZERO)
            return _unary(x, mpmath.log(v), 1 / v, -1 / v ** 2)
        if name == "sqrt":
            if v < 0:
                return _nan_like(x)
            if v == 0:
                return Num(ZERO, ZERO if x.d == 0 else NAN, ZERO, ZERO)
            r = mpmath.sqrt(v)
            return _unary(x, r, 1 / (2 * r), -1 / (4 * r * v))
        if name in ("asin", "acos"):
            if abs(v) > 1:
                return _nan_like(x)
            sgn = 1 if name == "asin" else -1
            val = mpmath.asin(v) if name == "asin" else mpmath.acos(v)
            if abs(v) == 1:
                return Num(val, ZERO if x.d == 0 else NAN, ZERO, ZERO)
            w = 1 - v * v
            g1 = sgn / mpmath.sqrt(w)
            return _unary(x, val, g1, sgn * v / w ** MPF(1.5), abs(g1) * (1 + (1 + v * v) / (2 * w)))
        if not mpmath.isfinite(v):  # (inputs of the tests are finite; an infinite argument only after an overflow)
            return _nan_like(x)
        if name == "sin":
            return _unary(x, mpmath.sin(v), mpmath.cos(v), -mpmath.sin(v))
        if name == "cos":
            return _unary(x, mpmath.cos(v), -mpmath.sin(v), -mpmath.cos(v))
        if name == "tan":
            tv = mpmath.tan(v)
            return _unary(x, tv, 1 + tv * tv, 2 * tv * (1 + tv * tv))
        if name == "tanh":
            tv = mpmath.tanh(v)
            return _unary(x, tv, 1 - tv * tv, -2 * tv * (1 - tv * tv), 1 + tv * tv)
        if name == "sinh":
            return _unary(x, mpmath.sinh(v), mpmath.cosh(v), mpmath.sinh(v))
        if name == "cosh":
            return _unary(x, mpmath.cosh(v), mpmath.sinh(v), mpmath.cosh(v))
        if name == "atan":
            w = 1 + v * v
            return _unary(x, mpmath.atan(v), 1 / w, -2 * v / w ** 2)
        raise KeyError(name)

    return f


def _truth(x) -> Num:
    return Num(ONE if x else ZERO)


def _rel(op):
    def r(a, b):
        a, b = num(a), num(b)
        return _truth(op(a.v, b.v))

    return r


_CMP = {ast.Lt: lambda x, y: x < y, ast.LtE: lambda x, y: x <= y, ast.Gt: lambda x, y: x > y, ast.GtE: lambda x, y: x >= y,
        ast.Eq: lambda x, y: x == y, ast.NotEq: lambda x, y: x != y}
FUNCTIONS = {
    **{nm: _f(nm) for nm in ("exp", "log", "sqrt", "sin", "cos", "tan", "tanh", "sinh", "cosh", "atan", "asin", "acos")},
    "floor": floor, "abs": absolute, "Abs": absolute, "pow": power,
    "Conditional": lambda c, a, b: num(a) if c else num(b),
    "Lt": _rel(_CMP[ast.Lt]), "Le": _rel(_CMP[ast.LtE]), "Gt": _rel(_CMP[ast.Gt]), "Ge": _rel(_CMP[ast.GtE]),
    "Eq": _rel(_CMP[ast.Eq]),
    "And": lambda *c: _truth(all(c)), "Or": lambda *c: _truth(any(c)), "Not": lambda c: _truth(not c),
}
_BIN = {ast.Add: add, ast.Sub: lambda a, b: add(a, neg(b)), ast.Mult: mul, ast.Div: div, ast.Pow: power, ast.Mod: mod}


class OdeMp:
    """The file's states, parameters and assignments, evaluated at one point: ``rhs(y, p, t, i)`` -> (f_i, J_ii) as Num."""

    def __init__(self, path):
        self.path = Path(path)
        tree = ast.parse(self.path.read_text())
        self.states, self.params, self.exprs = {}, {}, {}
        for node in tree.body:
            if isinstance(node, ast.Expr) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Name):
                target = {"states": self.states, "parameters": self.params}.get(node.value.func.id)
                for kw in node.value.keywords if target is not None else ():
                    v = kw.value.args[0] if isinstance(kw.value, ast.Call) else kw.value  # ScalarParam(value, unit=...)
                    target[kw.arg] = float(ast.literal_eval(v))
            elif isinstance(node, ast.Assign):
                self.exprs[node.targets[0].id] = node.value
        self.state_names = list(self.states)
        self.parameter_names = list(self.params)

    def rhs(self, y: dict, p: dict, t: float, seed: str):
        """f and J = d f / d seed of d<seed>_dt: y, p map names to floats."""
        env = {"time": num(t), "t": num(t), "pi": Num(+mpmath.pi)}
        env.update({k: num(v) for k, v in p.items()})
        env.update({k: Num(MPF(float(v)), ONE if k == seed else ZERO) for k, v in y.items()})
        memo = {}

        def ev(node):
            if isinstance(node, ast.Constant):
                return num(node.value)
            if isinstance(node, ast.Name):
                if node.id in env:
                    return env[node.id]
                if node.id not in memo:
                    memo[node.id] = ev(self.exprs[node.id])
                return memo[node.id]
            if isinstance(node, ast.BinOp):
                return _BIN[type(node.op)](ev(node.left), ev(node.right))
            if isinstance(node, ast.UnaryOp):
                x = ev(node.operand)
                return {ast.USub: neg, ast.UAdd: num, ast.Not: lambda c: _truth(not c)}[type(node.op)](x)
            if isinstance(node, ast.Compare):  # Python's chained comparison on numbers
                left = ev(node.left)
                for op, right in zip(node.ops, node.comparators):
                    right = ev(right)
                    if not _CMP[type(op)](left.v, right.v):
                        return _truth(False)
                    left = right
                return _truth(True)
            if isinstance(node, ast.BoolOp):  # Python's and / or: the deciding operand
                vals = [ev(v) for v in node.values]
                out = vals[0]
                for v in vals[1:]:
                    out = (v if out else out) if isinstance(node.op, ast.And) else (out if out else v)
                return out
            if isinstance(node, ast.Call):
                return FUNCTIONS[node.func.id](*[ev(a) for a in node.args])
            raise TypeError(type(node).__name__)

        out = ev(self.exprs[f"d{seed}_dt"])
        return out, Num(out.d, ZERO, out.md, ZERO)


def _update(y, f: Num, J: Num, dt, scheme):
    """The step (y, f, J as Num; J's value and magnitude in .v / .mv) in mpmath -> (new value, its running-error magnitude)."""
    y = num(y)
    if scheme == "generalized_rush_larsen" and abs(J.v) > GRL1_THRESHOLD:
        inc = mul(div(f, J), add(FUNCTIONS["exp"](mul(J, dt)), -1.0))
    else:
        inc = mul(f, dt)
    u = add(y, inc)
    return u.v, u.mv


def reference(path, Y, P, t, dt, schemes=("generalized_rush_larsen", "forward_euler")):
    """Y: (NS, N) states, P: (NP,) or (NP, N) parameters (floats) -> {scheme: (value, magnitude)} as (NS, N) object arrays of mpf."""
    with mpmath.workdps(DPS):
        return _reference(path, Y, P, t, dt, schemes)


def _reference(path, Y, P, t, dt, schemes):
    m = OdeMp(path)
    Y = np.asarray(Y, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    ns, n = Y.shape
    out = {s: (np.empty((ns, n), dtype=object), np.empty((ns, n), dtype=object)) for s in schemes}
    dtm = MPF(float(dt))
    for j in range(n):
        y = dict(zip(m.state_names, Y[:, j]))
        p = dict(zip(m.parameter_names, P[:, j] if P.ndim == 2 else P))
        for i, s in enumerate(m.state_names):
            f, J = m.rhs(y, p, t, s)
            for sch in schemes:
                out[sch][0][i, j], out[sch][1][i, j] = _update(y[s], f, J, dtm, sch)
    return out


def ulp_errors(got, ref):
    """|got - value| in units of 2^-52 * magnitude (+ one subnormal ulp), per entry; NaN where the reference is not finite
    (those entries are checked for being non-finite instead)."""
    value, mag = ref
    got = np.asarray(got, dtype=np.float64)
    err = np.full(got.shape, np.nan)
    with mpmath.workdps(DPS):
        for idx in np.ndindex(got.shape):
            v = value[idx]
            if mpmath.isfinite(v) and abs(v) <= BIG:
                err[idx] = float(abs(MPF(float(got[idx])) - v) / (EPS * mag[idx] + TINY)) if np.isfinite(got[idx]) else np.inf
    return err


def nonfinite(ref):
    value = ref[0]
    return np.vectorize(lambda v: not (mpmath.isfinite(v) and abs(v) <= BIG), otypes=[bool])(value)


# ---------------------------------------------------------------------------------------------------- tests/data/language_cell.ode
LANGUAGE_CELL = Path(__file__).resolve().parent / "data" / "language_cell.ode"
# the drivers' edge values: each column of the edge nodes takes the next value of every list
DRIVER_EDGES = {
    "a": [0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 1.5707963267948966, -1.5707963267948966, 800.0, -800.0, 709.0, 5e-324, -2.0, 1.5],
    "b": [1.0, 0.25, 2.0, 3.0, 0.5, 1.0, 4.0],
    "z": [0.0, -0.0, 5e-324, 2.2250738585072014e-308, -1.0, -5e-324, 1.0, 700.0, 1e-300],
    "u": [1.0, -1.0, 1.0000000000000002, -1.0000000000000002, 0.0, -0.0, 0.5],
    "num": [-7.5, 7.5, 0.0, -0.0, -6.0, 6.0, -2.5, 1e-300],
    "den": [-2.0, 2.0, -1.5, 3.0, 1.5, -3.0],
}
EDGE_NODES = 42
# the random nodes: the drivers' ranges, and the self-dependent probes' (|J dt| of order 1 at dt = 0.5, away from r_abs's and
# r_cond's switches)
DRIVER_RANGES = {"a": (-3.0, 3.0), "b": (0.2, 4.0), "z": (0.05, 5.0), "u": (-0.95, 0.95), "num": (-10.0, 10.0)}
SELF_RANGES = {"r_tanh": (-1.5, 1.5), "r_pow": (0.2, 1.2), "r_powp": (0.3, 2.0), "r_atan": (-1.5, 1.5), "r_sqrt": (0.2, 2.0),
               "r_log": (0.5, 3.0), "r_abs": (-0.5, 1.0), "r_cond": (0.1, 0.9), "r_inv": (0.45, 1.0)}
THRESHOLDS = (0.0, 5e-9, 1e-8, 1.0000001e-8, 2e-8)  # e_0 .. e_4: GRL1 where |J| > 1e-8, forward Euler elsewhere


def language_points(state_names, n_random, seed):
    """(NS, n_random + EDGE_NODES) states of tests/data/language_cell.ode: random drivers, then the edge nodes."""
    rng = np.random.default_rng(seed)
    n = n_random + EDGE_NODES
    Y = np.empty((len(state_names), n))
    for k, s in enumerate(state_names):
        if s in DRIVER_RANGES:
            Y[k, :n_random] = rng.uniform(*DRIVER_RANGES[s], n_random)
        elif s == "den":
            Y[k, :n_random] = rng.choice([-1.0, 1.0], n_random) * rng.uniform(0.5, 3.0, n_random)
        if s in DRIVER_EDGES:
            Y[k, n_random:] = [DRIVER_EDGES[s][j % len(DRIVER_EDGES[s])] for j in range(EDGE_NODES)]
        elif s in SELF_RANGES:
            Y[k] = rng.uniform(*SELF_RANGES[s], n)
        elif s.startswith("q_"):
            Y[k] = rng.uniform(-2.0, 2.0, n)
        else:  # the probes s_*
            Y[k] = rng.uniform(-1.0, 1.0, n)
    return Y


def language_parameters(model, n=None, seed=0):
    """The file's parameters (P,), or per node (P, n): the period, start, exponent and every threshold coefficient varied."""
    p = model.init_parameter_values()
    if n is None:
        return p
    rng = np.random.default_rng(seed)
    P = np.repeat(p[:, None], n, axis=1)
    P[model.parameter_index("period")] = rng.uniform(0.7, 6.0, n)
    P[model.parameter_index("start")] = rng.uniform(-2.0, 3.0, n)
    P[model.parameter_index("p_e")] = rng.uniform(0.55, 1.2, n)
    for k in range(len(THRESHOLDS)):
        P[model.parameter_index(f"e_{k}")] = np.roll(THRESHOLDS, k)[np.arange(n) % len(THRESHOLDS)]
    return P


def compare(got, ref, state_names):
    """Per state: the largest error in ulp of the running-error magnitude over the nodes where the reference is finite (inf
    where the tested side is not finite there), and the nodes where the reference is not finite but the tested side is."""
    err = ulp_errors(got, ref)
    leak = nonfinite(ref) & np.isfinite(np.asarray(got, dtype=np.float64))
    worst = {s: float(np.nanmax(err[k])) if np.isfinite(err[k]).any() or np.isinf(err[k]).any() else 0.0
             for k, s in enumerate(state_names)}
    return worst, [(state_names[k], int(j)) for k, j in np.argwhere(leak)]


# the probes whose construct is made of correctly rounded operations (arithmetic, sqrt, %, floor, selects, comparisons, integer
# powers printed as products); every other probe uses a transcendental function or pow
CORRECTLY_ROUNDED = ("s_arith", "s_unary", "s_floor", "s_mod", "s_pace", "s_time", "s_sqrt", "s_abs", "s_p2", "s_p3", "s_p4", "s_m1",
                     "s_m2", "s_m3", "s_m4", "s_fm1", "s_cmp", "s_chain", "s_rel", "s_cond", "q_0", "q_1", "q_2", "q_3", "q_4")
DRIVERS = ("a", "b", "z", "u", "num", "den")


def build_host(tmp, model):
    """tests/ode_host_harness.cpp built with g++ on the model's generated source -> run(states, params, t, dt), or None
    without g++."""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        return None
    here = Path(__file__).resolve().parent
    src = tmp / f"{model.cxx_name}.h"
    src.write_text(model.source)
    exe = tmp / model.cxx_name
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{rocm}", f'-DBEAT_ODE_SOURCE="{src}"',
                    f"-DBEAT_ODE_MODEL={model.cxx_name}", "-o", str(exe), str(here / "ode_host_harness.cpp")], check=True)

    def run(S, P, t, dt):
        S = np.ascontiguousarray(S, dtype=np.float64)
        S.tofile(tmp / "s.bin")
        P = np.asarray(P, dtype=np.float64)
        np.ascontiguousarray(P if P.size else np.zeros(1)).tofile(tmp / "p.bin")  # (NP is at least 1)
        res = subprocess.run([str(exe), str(tmp / "s.bin"), str(tmp / "p.bin"), str(tmp / "o.bin"), str(S.shape[1]), repr(float(t)),
                              repr(float(dt))], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        return np.fromfile(tmp / "o.bin").reshape(S.shape)

    return run
