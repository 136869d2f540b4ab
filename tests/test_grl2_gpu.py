"""GPU: the kernel ``beat.models.from_ode`` generates under ``scheme="generalized_rush_larsen_2"``, through the routes every generated
model takes: one step against the two stages in mpmath (tests/_grl2_ref.py) over the launch's edge sizes and the three
parameter routes; the routes against each other bit for bit; the fused Strang split step against its host restatement, with
the one-launch solve and with the solve that defers the potential's last update to the next ionic launch; the observed order
on the device; the in-kernel time loop; and a GRL1 and a GRL2 model of one file behind two markers."""
import sys
from pathlib import Path

import numpy as np
import pytest

import _grl2_ref as R
import _ode_mp as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
GRL1, GRL2 = "generalized_rush_larsen", "generalized_rush_larsen_2"
# the kernel-side bounds of tests/test_ode_language_gpu.py (ulp of the budget's magnitude)
BOUND_CR = 1.0
BOUND_TR = 2.0
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)  # the wave's edge, the 256-node tile's edge, a second tile
CABLE_CELLS, CABLE_H, CABLE_D = 64, 0.25, 0.1


# ---------------------------------------------------------------------------------------------------- one step against mpmath
def _language_case(route):
    """(path, correctly rounded states, dt, states, parameters, t, marker bytes | None) of tests/data/language_cell.ode for one
    route: the nodes and parameter cases of tests/test_ode_language_cpu.py (uniform at t = 0, per node at t = 13.7); for the
    classes 22 random nodes and the 42 edge nodes, two parameter sets alternating."""
    from beat.models import from_ode

    model = from_ode(M.LANGUAGE_CELL, scheme=GRL2)
    if route == "classes":
        Y = M.language_points(model.state_names, 22, seed=3)
        two = M.language_parameters(model, 2, seed=4)
        marks = (np.arange(Y.shape[1]) % 2).astype(np.uint8)
        return M.LANGUAGE_CELL, M.CORRECTLY_ROUNDED, 0.5, Y, two[:, marks], 13.7, marks, 22
    Y = M.language_points(model.state_names, 150, seed=1)
    if route == "uniform":
        return M.LANGUAGE_CELL, M.CORRECTLY_ROUNDED, 0.5, Y, M.language_parameters(model), 0.0, None, 150
    return M.LANGUAGE_CELL, M.CORRECTLY_ROUNDED, 0.5, Y, M.language_parameters(model, Y.shape[1], seed=2), 13.7, None, 150


def _small_case(route):
    """The same for tests/data/small_cell.ode: the points and parameters of tests/_grl2_ref.py (every node finite)."""
    from beat.models import from_ode

    model = from_ode(SMALL, scheme=GRL2)
    Y = R.small_points(model)
    n = Y.shape[1]
    if route == "uniform":
        return SMALL, (), R.SMALL_DT, Y, R.small_parameters(model), 0.9, None, n
    if route == "per_node":
        return SMALL, (), R.SMALL_DT, Y, R.small_parameters(model, n), 0.2, None, n
    two = R.small_parameters(model, 2, seed=7)
    marks = (np.arange(n) % 2).astype(np.uint8)
    return SMALL, (), R.SMALL_DT, Y, two[:, marks], 0.9, marks, n


_CASES = {}


def _case(which, route):
    """A case and its mpmath reference, computed once per session."""
    if (which, route) not in _CASES:
        case = (_language_case if which == "language" else _small_case)(route)
        path, cr, dt, Y, P, t = case[:6]
        _CASES[which, route] = case + (R.reference(path, Y, P, t, dt, cr),)
    return _CASES[which, route]


def _launch(hip_ctx, model, route, Y, P, t, dt, marks):
    """One step of the states ``Y`` by ``route``: the handle's call (uniform vector, per-node rows) or a ``_DeviceODE`` with an
    explicit class byte per node."""
    import beat
    from beat.odesolver import _DeviceODE

    if route != "classes":
        return model(states=Y, t=t, parameters=P, dt=dt)
    n = Y.shape[1]
    sets = [np.ascontiguousarray(P[:, int(np.argmax(marks == c))]) for c in (0, 1)] if n > 1 else [np.ascontiguousarray(P[:, 0])] * 2
    ode = _DeviceODE(hip_ctx, model, model.num_states, n, 0, None, beat.telemetry.NullMonitor())
    ode.set_initial(np.ascontiguousarray(Y))
    ode.explicit_classes = True
    ode.set_classes(hip_ctx.from_numpy(np.ascontiguousarray(marks)), sets)
    ode.step(t, dt, v_index=model.state_index(model.v_name) if model.v_name else 0)
    return ode.states.numpy()


@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("route", ["uniform", "per_node", "classes"])
@pytest.mark.parametrize("which", ["language", "small"])
def test_generated_grl2_kernel_against_mpmath(hip_ctx, which, route, fast_exp):
    """One step of n = 1, 63, 64, 65, 255, 256, 257, 513 nodes (the case's nodes, repeated cyclically) by each parameter route,
    with the table-driven exp and libm's, against the two stages in mpmath: every state within the budget of
    tests/_grl2_ref.py, eps (K_i m2_i + sum_j |d y'_i / d yh_j| (K_j + 1/2) m1_j), with the kernel-side bounds K of
    tests/test_ode_language_gpu.py; where the reference is not finite the kernel's value is not finite; drivers unchanged.
    Measured on an MI355X (largest over states, nodes and sizes, in ulp of the budget's magnitude): language_cell 0.39 / 0.40 / 0.36
    and small_cell 0.38 / 0.41 / 0.83 for the uniform / per-node / class routes (the cases differ in their parameters)."""
    from beat.models import from_ode

    path, cr, dt, Y, P, t, marks, n_finite, ref = _case(which, route)
    model = from_ode(path, scheme=GRL2, fast_exp=fast_exp, name=f"{which}_grl2_{int(fast_exp)}")
    names = model.state_names
    value, mag = R.budgeted(ref, names, cr, BOUND_CR, BOUND_TR)
    if route != "uniform":
        # (the library holds a variant instance against the plain one at its first launch, and that check takes two equal
        # infinities for a difference: the first launch is on the case's random nodes, all finite)
        _launch(hip_ctx, model, route, Y[:, :n_finite], P[:, :n_finite], t, dt, None if marks is None else marks[:n_finite])
    for n in SIZES:
        idx = np.arange(n) % Y.shape[1]
        got = _launch(hip_ctx, model, route, Y[:, idx], P if P.ndim == 1 else P[:, idx], t, dt, None if marks is None else marks[idx])
        assert got.shape == (len(names), n)
        worst, leak = M.compare(got, (value[:, idx], mag[:, idx]), names)
        print(which, route, fast_exp, n, "largest", max(worst.values()))
        assert not leak, (n, "finite where the reference is not", leak[:10])
        for k, s in enumerate(names):
            if s in M.DRIVERS:
                np.testing.assert_array_equal(got[k], Y[k, idx], err_msg=f"n = {n}: driver {s}")
        bad = {s: v for s, v in worst.items() if v > (BOUND_CR if s in cr else BOUND_TR)}
        assert not bad, (n, bad)


def test_parameter_routes_give_the_same_bits(hip_ctx):
    """small_cell, 513 nodes, two parameter sets: the per-node rows and the class bytes give, node by node, the bits the
    uniform route gives with the node's set.  (How far the uniform route is from the exact step is the test above's; how far the
    twin is, tests/test_grl2_cpu.py's: the two differ by the sum of their budgets at most.)"""
    from beat.models import from_ode

    model = from_ode(SMALL, scheme=GRL2)
    n, t, dt = 513, 0.9, 0.05
    Y = R.small_points(model, n, seed=9)
    two = R.small_parameters(model, 2, seed=7)
    marks = (np.arange(n) % 2).astype(np.uint8)
    uniform = [model(states=Y, t=t, parameters=np.ascontiguousarray(two[:, c]), dt=dt) for c in (0, 1)]
    want = np.where(marks[None, :] == 0, uniform[0], uniform[1])
    assert np.isfinite(want).all() and not np.array_equal(uniform[0], uniform[1])
    P = two[:, marks]
    np.testing.assert_array_equal(_launch(hip_ctx, model, "per_node", Y, P, t, dt, None), want)
    np.testing.assert_array_equal(_launch(hip_ctx, model, "classes", Y, P, t, dt, marks), want)


# ---------------------------------------------------------------------------------------------------- the split step
def _device_cable(scheme, dt, nsteps):
    """``_grl2_ref.strang_cable`` on the device: MonodomainSplittingSolver(theta=0.5) on a 64-cell interval, theta_pde = 0.5,
    ksp_rtol 1e-13, the fused route.  Returns the (NS, 65) states ordered by x."""
    import beat
    from beat import grid as g
    from beat.models import from_ode

    model = from_ode(SMALL, scheme=scheme)
    mesh = g.create_interval(g.COMM_WORLD, CABLE_CELLS, [0.0, CABLE_CELLS * CABLE_H])
    V = g.functionspace(mesh, ("P", 1))
    x = np.asarray(V.tabulate_dof_coordinates())[:, 0]
    node = np.rint(x / CABLE_H).astype(int)
    pde = beat.MonodomainModel(time=g.Constant(mesh, 0.0), mesh=mesh, M=CABLE_D, C_m=1.0,
                               params={"theta": 0.5, "petsc_options": {"ksp_rtol": 1e-13, "ksp_atol": 1e-50}})
    y0 = np.repeat(model.init_state_values()[:, None], len(x), axis=1)
    y0[model.state_index("V"), node < 6] = -20.0
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=pde.state, fun=model, init_states=y0,
                                         parameters=model.init_parameter_values(stim_amplitude=0.0), num_states=model.num_states,
                                         v_index=model.state_index("V"))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=0.5)
    assert ode.on_device and solver._can_fuse()
    t0 = 0.0
    for _ in range(nsteps):
        solver.step((t0, t0 + dt))
        t0 = t0 + dt
    out = np.empty((model.num_states, len(x)))
    out[:, node] = np.asarray(ode.values)
    return out


@pytest.fixture(params=["one-launch", "deferred"])
def small_solve(request):
    """The one-launch solve of small grids, or the multi-launch solve that leaves the potential's last update to the next
    ionic launch (the pending-update load of V under a two-stage step)."""
    from beat._engine import HipOps

    old = HipOps.default_small
    HipOps.default_small = request.param == "one-launch"
    yield request.param
    HipOps.default_small = old


def test_fused_strang_step_against_its_host_restatement(hip_ctx, small_solve):
    """40 steps of dt = 0.025 on the 64-cell interval against ``_grl2_ref.strang_cable`` -- the twin and ``oracle.fem`` in the
    same order -- to 1e-7 on every state, relative to the value or, where that is smaller, to 1e-6 of the state's largest (a
    gate at rest is 1e-3 of one that is open).  A corrective launch or a deferred update applied twice is an error of the size
    of the potential's change per step.  Measured on an MI355X: at most 2.0e-9 (the calcium state) with either solve."""
    from beat.models import from_ode

    dev = _device_cable(GRL2, 0.025, 40)
    host = R.strang_cable(from_ode(SMALL, scheme=GRL2), 0.025, 40, CABLE_CELLS, CABLE_H, CABLE_D)
    scale = np.maximum(np.abs(host), 1e-6 * np.abs(host).max(axis=1, keepdims=True))
    err = (np.abs(dev - host) / scale).max(axis=1)
    print(small_solve, "largest relative difference per state", err)
    assert host[0, 6:].max() > -20.0  # (the front has left the nodes that were raised)
    assert (err <= 1e-7).all(), err


def test_order_on_the_device(hip_ctx):
    """The cable of the split-step test at dt = 0.05, 0.025, 0.0125 over 2 ms against the device's own GRL2 run at dt = 0.05 / 64
    (2840 steps of GRL2 and 280 of GRL1 on 65 nodes); error: max |difference of V| in mV; the conditions of the CPU order tests.  Measured on an MI355X: GRL1 6.16 / 3.41 / 1.82
    (orders 0.85, 0.91), GRL2 0.988 / 0.293 / 0.0677 (orders 1.75, 2.11) -- the host's figures."""
    ref = _device_cable(GRL2, 0.05 / 64, 2560)[0]
    errors = {s: [float(np.max(np.abs(_device_cable(s, dt, int(round(2.0 / dt)))[0] - ref))) for dt in (0.05, 0.025, 0.0125)] for s in (GRL1, GRL2)}
    R.assert_second_against_first_order(errors[GRL1], errors[GRL2], "Strang cable on the device")


# ---------------------------------------------------------------------------------------------------- the other routes
def test_in_kernel_time_loop(hip_ctx):
    """``run``: 400 steps of dt = 0.025 in one launch (through the file's own stimulus window), V tracked every
    step, against 400 twin steps: every state and every tracked value to 1e-9, relative to the value or, where that is
    smaller (a potential near zero), to 1e-3 of the row's largest.  Measured on an MI355X: 2.5e-13 on the states, 2.8e-14 on the track."""
    from beat.models import from_ode

    model = from_ode(SMALL, scheme=GRL2)
    vi = model.state_index("V")
    y0, p, dt = model.init_state_values(), model.init_parameter_values(), 0.025
    out, track = model.run(y0, p, dt, 400, nbeats=1, t0=0.0, track_indices=[vi], save_freq=1)
    y, rows = y0.copy(), []
    for j in range(400):
        rows.append(y[vi])
        y = model.numpy_step(y, j * dt, p, dt)
    rows = np.array(rows)
    assert track.shape == (400, 1) and rows.max() > rows[0] + 10.0  # (the stimulus has depolarised the cell)
    err_state = np.abs(out - y) / np.abs(y)
    err_track = np.abs(track[:, 0] - rows) / np.maximum(np.abs(rows), 1e-3 * np.abs(rows).max())
    print("in-kernel loop: states", err_state, "track", err_track.max())
    assert (err_state <= 1e-9).all() and err_track.max() <= 1e-9


def test_grl1_and_grl2_models_of_one_file_behind_two_markers(hip_ctx):
    """DolfinMultiODESolver with a GRL1 model on one half of an interval and a GRL2 model of the same file on the other: after 20
    steps inside the stimulus window each region holds, bit for bit, what its model gives alone on the region's nodes."""
    import beat
    from beat import grid as g
    from beat.models import from_ode

    models = {0: from_ode(SMALL, scheme=GRL1), 1: from_ode(SMALL, scheme=GRL2)}
    mesh = g.create_interval(g.COMM_WORLD, CABLE_CELLS, [0.0, CABLE_CELLS * CABLE_H])
    V = g.functionspace(mesh, ("P", 1))
    x = np.asarray(V.tabulate_dof_coordinates())[:, 0]
    markers = g.Function(V)
    markers.x.array[:] = np.where(x < 7.1, 0.0, 1.0)
    where = {k: np.asarray(markers.x.array) == k for k in models}
    rng = np.random.default_rng(12)
    init = {}
    for k, m in models.items():
        init[k] = np.repeat(m.init_state_values()[:, None], int(where[k].sum()), axis=1)
        init[k][m.state_index("V")] += rng.uniform(0.0, 10.0, init[k].shape[1])
    params = {k: m.init_parameter_values(stim_amplitude=30.0, stim_start=0.0) for k, m in models.items()}
    v_pde = g.Function(V)
    ode = beat.odesolver.DolfinMultiODESolver(v_ode=g.Function(V), v_pde=v_pde, markers=markers, num_states={k: m.num_states for k, m in models.items()},
                                              fun=models, init_states={k: init[k].copy() for k in models}, parameters=params,
                                              v_index={k: m.state_index("V") for k, m in models.items()})
    assert ode.on_device
    alone = {k: init[k].copy() for k in models}
    dt = 0.025
    for j in range(20):
        ode.step(j * dt, dt)
        for k, m in models.items():
            alone[k] = m(states=alone[k], t=j * dt, parameters=params[k], dt=dt)
    for k in models:
        np.testing.assert_array_equal(np.asarray(ode.values(k)), alone[k])
    assert models[0].model_id != models[1].model_id and not ode._marked  # (two kernels, a launch per marker)
