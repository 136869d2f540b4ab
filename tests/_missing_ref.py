"""What tests/test_missing_cpu.py and tests/test_missing_gpu.py share: the split halves of tests/data/small_cell.ode
(``split_membrane.ode`` misses ``ca``; ``split_calcium.ode`` misses ``V, m, h``), their nodes and parameters, the mpmath reference of the
membrane half -- taken on ``split_membrane_as_parameters.ode``, the same equations with ``ca`` as a per-node PARAMETER, which the
independent evaluation of tests/_ode_mp.py reads without knowing what a missing variable is -- and one kernel step of a model's
(S + M, N) rows by each parameter route."""
from __future__ import annotations

from pathlib import Path

import numpy as np

import _grl2_ref as R
import _ode_mp as M

DATA = Path(__file__).resolve().parent / "data"
SMALL = DATA / "small_cell.ode"
MEMBRANE = DATA / "split_membrane.ode"
CALCIUM = DATA / "split_calcium.ode"
AS_PARAMETERS = DATA / "split_membrane_as_parameters.ode"
GRL1, FE, GRL2 = "generalized_rush_larsen", "forward_euler", "generalized_rush_larsen_2"
MEMBRANE_STATES = ("V", "m", "h", "n")
CALCIUM_MISSING = ("V", "m", "h")
DT = R.SMALL_DT


def whole(scheme=GRL1, **kw):
    from beat.models import from_ode

    return from_ode(SMALL, scheme=scheme, **kw)


def membrane(scheme=GRL1, **kw):
    from beat.models import from_ode

    return from_ode(MEMBRANE, scheme=scheme, missing=["ca"], **kw)


def calcium(scheme=GRL1, **kw):
    """The calcium half; V is drawn from the potential's range where its kernel is tried (``missing_ranges``)."""
    from beat.models import from_ode

    return from_ode(CALCIUM, scheme=scheme, missing=CALCIUM_MISSING, missing_ranges={"V": (-100.0, 60.0)}, **kw)


def points(n=R.SMALL_N, seed=3):
    """(the (4, n) states of the membrane half, the (1, n) values of ``ca``, the (5, n) states of small_cell they come from):
    ``_grl2_ref.small_points``, so ``ca`` is drawn from the range it gives that state."""
    w = whole()
    Y = R.small_points(w, n, seed)
    return Y[[w.state_index(s) for s in MEMBRANE_STATES]], Y[[w.state_index("ca")]], Y


def membrane_parameters(model, n=None, seed=4):
    """Uniform (P,) with the stimulus at 30, or per node (P, n): two conductances and a reversal potential varied (what
    ``_grl2_ref.small_parameters`` varies of the parameters this half has)."""
    p = model.init_parameter_values(stim_amplitude=30.0)
    if n is None:
        return p
    rng = np.random.default_rng(seed)
    P = np.repeat(p[:, None], n, axis=1)
    for name in ("g_in", "g_out"):
        P[model.parameter_index(name)] *= rng.uniform(0.5, 1.5, n)
    P[model.parameter_index("E_out")] += rng.uniform(-5.0, 5.0, n)
    return P


def as_parameters(P, C):
    """The membrane half's parameters ``P`` ((P,) or (P, n)) and its missing values ``C`` (1, n) as the per-node parameter array
    of split_membrane_as_parameters.ode: the same rows, then ``ca``."""
    n = C.shape[1]
    P = np.asarray(P, dtype=np.float64)
    return np.concatenate([np.broadcast_to(P.reshape(P.shape[0], -1), (P.shape[0], n)), C], axis=0)


def membrane_case(route, n=R.SMALL_N):
    """(Y, C, P, t, marker bytes | None) for one parameter route: uniform inside the stimulus window, per node outside it, two
    classes alternating inside it (tests/test_grl2_gpu.py's cases)."""
    model = membrane()
    Y, C, _ = points(n)
    if route == "uniform":
        return Y, C, membrane_parameters(model), 0.9, None
    if route == "per_node":
        return Y, C, membrane_parameters(model, n), 0.2, None
    two = membrane_parameters(model, 2, seed=7)
    marks = (np.arange(n) % 2).astype(np.uint8)
    return Y, C, two[:, marks], 0.9, marks


_REFS = {}


def membrane_reference(route):
    """{scheme: (value, magnitude) | GRL2's (value, m2, s_cr, s_tr)} of ``membrane_case(route)`` in mpmath, once per session."""
    if route not in _REFS:
        Y, C, P, t, _ = membrane_case(route)
        Pa = as_parameters(P, C)
        ref = dict(M.reference(AS_PARAMETERS, Y, Pa, t, DT))
        ref[GRL2] = R.reference(AS_PARAMETERS, Y, Pa, t, DT)
        _REFS[route] = ref
    return _REFS[route]


def budget(ref, scheme, bound_cr, bound_tr):
    """The (value, magnitude) pair ``_ode_mp.compare`` takes (no state of these files is in the correctly rounded group)."""
    return R.budgeted(ref[scheme], MEMBRANE_STATES, (), bound_cr, bound_tr) if scheme == GRL2 else ref[scheme]


def split_step(mem, cal, Y5, t, dt, p_mem, p_cal, step=None):
    """One step of small_cell's (5, n) states ``Y5`` by the two halves, each fed the other's step-start rows: V, m, h, n from the
    membrane half, ca from the calcium half.  ``step(model, states, t, p, dt, missing)``: the twin unless given."""
    w = whole()
    if step is None:
        step = lambda model, y, t, p, dt, c: model.numpy_step(y, t, p, dt, missing_variables=c)  # noqa: E731
    rows = [w.state_index(s) for s in MEMBRANE_STATES]
    ca = w.state_index("ca")
    out = np.empty_like(Y5)
    out[rows] = step(mem, Y5[rows], t, p_mem, dt, Y5[[ca]])
    out[[ca]] = step(cal, Y5[[ca]], t, p_cal, dt, Y5[[w.state_index(s) for s in cal.missing_names]])
    return out


def half_parameters(half, p_whole):
    """The parameters of a half, by name, from small_cell's (P,) vector."""
    w = whole()
    return np.array([p_whole[w.parameter_index(nm)] for nm in half.parameter_names])


def launch(hip_ctx, model, route, rows, P, t, dt, marks):
    """One kernel step of the (S + M, n) ``rows`` by ``route`` -> all rows back: the staged call (uniform vector, per-node rows)
    or a ``_DeviceODE`` with an explicit class byte per node (tests/test_grl2_gpu.py's ``_launch`` for a model with input rows)."""
    import beat
    from beat.odesolver import _DeviceODE

    rows = np.ascontiguousarray(rows)
    if route != "classes":
        return model.step_rows(rows, t, P, dt)
    n = rows.shape[1]
    sets = [np.ascontiguousarray(P[:, int(np.argmax(marks == c))]) for c in (0, 1)] if n > 1 else [np.ascontiguousarray(P[:, 0])] * 2
    ode = _DeviceODE(hip_ctx, model, model.num_states, n, 0, None, beat.telemetry.NullMonitor())
    ode.states.set(rows)
    ode.explicit_classes = True
    ode.set_classes(hip_ctx.from_numpy(np.ascontiguousarray(marks)), sets)
    ode.step(t, dt, v_index=model.state_index(model.v_name) if model.v_name else 0)
    return ode.states.numpy()


def interval_v0(x):
    """The initial potential of the coupled runs: rest at one end of the interval, 30 mV above it at the other."""
    x = np.asarray(x, dtype=np.float64)
    return -84.0 + 30.0 * x / x.max()


def twin_split_against_whole(v0, steps, dt, scheme=GRL1):
    """The three NumPy twins over ``steps`` steps from rest with the potential at ``v0`` (default parameters: the file's own stimulus
    window): the largest |split - whole| relative to each state's range over the nodes -- what rounding alone makes of the two
    mathematically equal runs on the host."""
    w, mem, cal = whole(scheme), membrane(scheme), calcium(scheme)
    y = np.repeat(w.init_state_values()[:, None], len(v0), axis=1)
    y[w.state_index("V")] = v0
    ys, p = y.copy(), w.init_parameter_values()
    pm, pc = half_parameters(mem, p), half_parameters(cal, p)
    t = 0.0
    for _ in range(steps):
        y = w.numpy_step(y, t, p, dt)
        ys = split_step(mem, cal, ys, t, dt, pm, pc)
        t += dt
    span = y.max(axis=1) - y.min(axis=1)
    return float((np.abs(ys - y).max(axis=1) / span).max())
