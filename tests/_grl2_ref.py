"""The second-order generalised Rush-Larsen step (GRL2) of an ``.ode`` file in mpmath, for tests/test_grl2_*.py: the two stages
evaluated on ``_ode_mp.OdeMp.rhs`` -- the file's syntax interpreted with mpmath numbers, no SymPy -- at the working precision and
with the running-error magnitudes of ``_ode_mp.reference``.

    stage 1   a_i = J_ii(y, t),        b_i = f_i(y, t),                          yh_i = y_i + phi(a_i, dt/2) b_i
    stage 2   A_i = J_ii(yh, t+dt/2),  B_i = f_i(yh, t+dt/2) + A_i (y_i - yh_i),  y_i' = y_i + phi(A_i, dt) B_i

with phi(a, h) = (exp(a h) - 1) / a where |a| > 1e-8 and h elsewhere.  A state whose self-derivative is identically zero has
a = A = 0 at every point, and the formulas above are the explicit midpoint rule for it: the reference needs no symbols.

The error budget of a double evaluation of the two stages.  Stage 2 is a function g_i(yh; y, p, t, dt) of the midpoint values.
A double evaluation computes yh_j with an error of at most K_j eps m1_j (m1_j: the running-error magnitude of stage 1, K_j: the
bound in ulp the project holds a single step of state j to), then evaluates g_i at ITS yh with an error of at most
K_i eps m2_i (m2_i: the running-error magnitude of stage 2 with yh as exact inputs).  To first order

    |y_i' - ref_i| <= eps (K_i m2_i + sum_j |d g_i / d yh_j| K_j m1_j),

the partial derivatives taken in mpmath by central differences.  ``OdeMp.rhs`` takes its states as doubles, so the reference
rounds its midpoint values to double before stage 2: half an ulp of yh_j more between the two sides' midpoints, and m1_j is
at least |yh_j| (the magnitude of a sum includes the sum), so K_j + 1/2 stands for K_j in the sum above.  The differences are
taken over 2^-26 of the midpoint value's size to either side -- doubles again; stage 2 itself is evaluated at 60 digits, so
the quotient is the derivative to about 2^-52 of itself.  A state whose stage-1 increment is an exact zero (f_j = 0 with
magnitude 0: a constant right-hand side 0) has yh_j = y_j without rounding, so its m1_j is 0; and g_i depends on yh_j only where
d<i>_dt names state j, directly or through intermediates."""
from __future__ import annotations

import ast

import mpmath
import numpy as np

import _ode_mp as M

MPF = M.MPF
FD_STEP = 2.0 ** -26


def _dependencies(m: M.OdeMp):
    """{state: the states its d<state>_dt names, directly or through intermediates, in the file's order}."""
    memo = {}

    def names(key):
        if key not in memo:
            memo[key] = set()  # (a cyclic definition is the generator's to refuse)
            out = set()
            for n in ast.walk(m.exprs[key]):
                if isinstance(n, ast.Name):
                    if n.id in m.states:
                        out.add(n.id)
                    elif n.id in m.exprs:
                        out |= names(n.id)
            memo[key] = out
        return memo[key]

    return {s: [x for x in m.state_names if x in names(f"d{s}_dt")] for s in m.state_names}


def _stage2(m, y, yh, p, th, dtm, s):
    """g_s(yh): (value, running-error magnitude) of the second stage of state ``s``, the midpoint values (doubles) as exact
    inputs."""
    f, J = m.rhs(yh, p, th, s)
    b = M.add(f, M.mul(J, M.add(M.num(float(y[s])), M.neg(M.num(float(yh[s]))))))
    return M._update(y[s], b, J, dtm, "generalized_rush_larsen")


def reference(path, Y, P, t, dt, correctly_rounded=()):
    """Y: (NS, N) states, P: (NP,) or (NP, N) parameters, floats -> (value, m2, s_cr, s_tr), each an (NS, N) object array of mpf:
    the GRL2 step, the running-error magnitude of its second stage, and sum_j |d g_i / d yh_j| m1_j over the states j in
    ``correctly_rounded`` and over the others.  (``t`` + ``dt`` / 2 is taken in double, as both tested sides take it.)"""
    with mpmath.workdps(M.DPS):
        return _reference(path, Y, P, t, dt, set(correctly_rounded))


def _reference(path, Y, P, t, dt, correctly_rounded):
    m = M.OdeMp(path)
    deps = _dependencies(m)
    Y = np.asarray(Y, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    ns, n = Y.shape
    value, m2, s_cr, s_tr = (np.empty((ns, n), dtype=object) for _ in range(4))
    dtm = MPF(float(dt))
    hdt = dtm / 2
    th = float(t) + 0.5 * float(dt)
    for j in range(n):
        y = dict(zip(m.state_names, Y[:, j]))
        p = dict(zip(m.parameter_names, P[:, j] if P.ndim == 2 else P))
        yh, m1 = {}, {}
        for s in m.state_names:
            f, J = m.rhs(y, p, t, s)
            v, m1[s] = M._update(y[s], f, J, hdt, "generalized_rush_larsen")
            yh[s] = float(v)
            if f.v == 0 and f.mv == 0:
                m1[s] = M.ZERO
        for i, s in enumerate(m.state_names):
            value[i, j], m2[i, j] = _stage2(m, y, yh, p, th, dtm, s)
            s_cr[i, j] = s_tr[i, j] = M.ZERO
            for d in deps[s]:
                if m1[d] == 0 or not mpmath.isfinite(value[i, j]):
                    continue
                if not np.isfinite(yh[d]):
                    continue
                h = FD_STEP * (abs(yh[d]) if yh[d] != 0 else 1.0)
                hi, lo = yh[d] + h, yh[d] - h
                up = _stage2(m, y, {**yh, d: hi}, p, th, dtm, s)[0]
                dn = _stage2(m, y, {**yh, d: lo}, p, th, dtm, s)[0]
                term = M._x(abs((up - dn) / (MPF(hi) - MPF(lo))), m1[d])
                if d in correctly_rounded:
                    s_cr[i, j] += term
                else:
                    s_tr[i, j] += term
    return value, m2, s_cr, s_tr


def budgeted(ref, names, correctly_rounded, bound_cr, bound_tr):
    """``ref`` as the (value, magnitude) pair ``_ode_mp.compare`` takes, the magnitude such that state i's bound (``bound_cr`` ulp
    for the states in ``correctly_rounded``, ``bound_tr`` for the others) times eps times it is the whole budget:
    m2_i + ((bound_cr + 1/2) s_cr_i + (bound_tr + 1/2) s_tr_i) / K_i."""
    value, m2, s_cr, s_tr = ref
    mag = np.empty(value.shape, dtype=object)
    with mpmath.workdps(M.DPS):
        for i, s in enumerate(names):
            k = MPF(bound_cr if s in correctly_rounded else bound_tr)
            for j in range(value.shape[1]):
                mag[i, j] = m2[i, j] + ((MPF(bound_cr) + 0.5) * s_cr[i, j] + (MPF(bound_tr) + 0.5) * s_tr[i, j]) / k
    return value, mag


def floats(value):
    """An (NS, N) object array of mpf as doubles (non-finite entries as they are)."""
    return np.vectorize(float, otypes=[np.float64])(value)


SMALL_DT = 0.05  # the step the small cell is held to the reference at: the largest of the order tests
SMALL_N = 48


def small_points(model, n=SMALL_N, seed=3):
    """States of tests/data/small_cell.ode over its physiological range (tests/test_ode_file_cpu.py's), the first node at rest."""
    rng = np.random.default_rng(seed)
    y = np.repeat(model.init_state_values()[:, None], n, axis=1)
    y[model.state_index("V"), 1:] = rng.uniform(-95.0, 45.0, n - 1)
    for g in ("m", "h", "n"):
        y[model.state_index(g), 1:] = rng.uniform(0.0, 1.0, n - 1)
    y[model.state_index("ca"), 1:] = 10.0 ** rng.uniform(-4.5, -2.5, n - 1)
    return y


def small_parameters(model, n=None, seed=4):
    """Uniform (P,) with the stimulus at 30, or per node (P, n): two conductances, a reversal potential and the pump varied."""
    p = model.init_parameter_values(stim_amplitude=30.0)
    if n is None:
        return p
    rng = np.random.default_rng(seed)
    P = np.repeat(p[:, None], n, axis=1)
    for name in ("g_in", "g_out", "v_pump"):
        P[model.parameter_index(name)] *= rng.uniform(0.5, 1.5, n)
    P[model.parameter_index("E_out")] += rng.uniform(-5.0, 5.0, n)
    return P


def strang_cable(model, dt, nsteps, cells=64, h=0.25, conductivity=0.1, raised=6, v_raised=-20.0):
    """The Strang split step on the host with ``model.numpy_step`` as the cell step and ``oracle.fem`` as the PDE step: an interval
    of ``cells`` P1 cells of length ``h``, C_m = 1, Crank-Nicolson with a direct solve (theta_pde = 0.5), the ionic half step /
    PDE step / ionic half step of ``oracle.splitting`` (theta_split = 0.5), ``stim_amplitude`` = 0, the potential raised to
    ``v_raised`` on the first ``raised`` nodes.  Returns the (NS, cells + 1) states after ``nsteps`` steps of ``dt``."""
    from oracle.fem import BoxMesh, OracleMonodomainModel
    from oracle.splitting import OracleODE, OracleSplitting

    mesh = BoxMesh((cells,), (cells * h,))
    pde = OracleMonodomainModel(mesh, conductivity, C_m=1.0, theta=0.5, default_timestep=dt)
    vi = model.state_index(model.v_name)
    y0 = np.repeat(model.init_state_values()[:, None], mesh.num_nodes, axis=1)
    y0[vi, :raised] = v_raised
    ode = OracleODE(mesh.num_nodes, y0, model.init_parameter_values(stim_amplitude=0.0),
                    lambda states, t, step, parameters: model.numpy_step(states, t, parameters, step), model.num_states, vi)
    split = OracleSplitting(pde, ode, theta=0.5)
    t0 = 0.0  # (the intervals as the solvers' own loops form them: t1 = t0 + dt accumulated)
    for _ in range(nsteps):
        split.step((t0, t0 + dt))
        t0 = t0 + dt
    return ode.values.copy()


def observed_orders(errors):
    """log2 of the ratios of consecutive errors (the step halves from one to the next)."""
    return [float(np.log2(a / b)) for a, b in zip(errors[:-1], errors[1:])]


def assert_second_against_first_order(e1, e2, what):
    """The conditions the order tests share: every observed order of GRL2 >= 1.5, every one of GRL1 <= 1.3, and GRL2's error at
    the smallest step at least 10 times smaller than GRL1's."""
    o1, o2 = observed_orders(e1), observed_orders(e2)
    print(f"{what}: GRL1 errors {e1} orders {o1}; GRL2 errors {e2} orders {o2}")
    assert all(o >= 1.5 for o in o2), (what, "GRL2", e2, o2)
    assert all(o <= 1.3 for o in o1), (what, "GRL1", e1, o1)
    assert 10.0 * e2[-1] <= e1[-1], (what, e1, e2)
