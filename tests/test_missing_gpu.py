"""GPU: missing variables of split cell models (``beat.models.from_ode(path, missing=...)``) as input rows behind the state rows:
the generated kernel against mpmath over the launch's edge sizes, the three parameter routes and both exps; the routes against
each other bit for bit; one step of the two halves of tests/data/small_cell.ode against one step of the whole; two
``DolfinODESolver``s coupled on the device against the monolithic one; the fused split step and the library's step loop; the live
``missing_variables`` array; the monitor kernel; the in-kernel time loop; the refusals; the demo."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

import _missing_ref as X
import _ode_mp as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
DEMOS = ROOT / "demos"
GRL1, FE, GRL2 = X.GRL1, X.FE, X.GRL2
# the kernel-side bounds of tests/test_ode_language_gpu.py (ulp of the budget's magnitude)
BOUND_CR = 1.0
BOUND_TR = 2.0
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)  # the wave's edge, the 256-node tile's edge, a second tile
CABLE_CELLS, CABLE_H, CABLE_D = 64, 0.25, 0.1  # the 64-cell interval of tests/test_grl2_gpu.py
CA0 = 2.5e-4


def _demo():
    sys.path.insert(0, str(DEMOS))
    try:
        spec = importlib.util.spec_from_file_location("demo_split_cell", DEMOS / "split_cell.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(str(DEMOS))
    return mod


# ---------------------------------------------------------------------------------------------------- 6. one step against mpmath
@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("route", ["uniform", "per_node", "classes"])
@pytest.mark.parametrize("scheme", [GRL1, GRL2])
def test_kernel_with_an_input_row_against_mpmath(hip_ctx, scheme, route, fast_exp):
    """One step of the membrane half -- ``ca`` in input row 4 -- at n = 1, 63, 64, 65, 255, 256, 257, 513 nodes (the case's 48
    nodes repeated cyclically) by each parameter route, with the table-driven exp and libm's, against mpmath on the
    as-parameters form of the file (tests/_missing_ref.py): every state within the kernel-side bounds of
    tests/test_ode_language_gpu.py (2 ulp of the budget's magnitude), and the input row back bit for bit as it went in.
    Measured on an MI355X (largest over states, sizes and exps): GRL1 0.30 / 0.30 / 0.30, GRL2 0.38 / 0.57 / 0.80 for the
    uniform / per-node / class routes."""
    Y, C, P, t, marks = X.membrane_case(route)
    model = X.membrane(scheme, fast_exp=fast_exp, name=f"split_membrane_{int(fast_exp)}")
    value, mag = X.budget(X.membrane_reference(route), scheme, BOUND_CR, BOUND_TR)
    rows = np.concatenate([Y, C], axis=0)
    if route != "uniform":  # (the variant instance's first launch, where the library holds it against the plain one: every node finite)
        X.launch(hip_ctx, model, route, rows, P, t, X.DT, marks)
    for n in SIZES:
        idx = np.arange(n) % Y.shape[1]
        got = X.launch(hip_ctx, model, route, rows[:, idx], P if P.ndim == 1 else P[:, idx], t, X.DT, None if marks is None else marks[idx])
        assert got.shape == (5, n)
        np.testing.assert_array_equal(got[4], C[0, idx], err_msg=f"n = {n}: the input row")
        worst, leak = M.compare(got[:4], (value[:, idx], mag[:, idx]), X.MEMBRANE_STATES)
        print(scheme, route, fast_exp, n, "largest", max(worst.values()))
        assert not leak, (n, leak[:10])
        assert max(worst.values()) <= BOUND_TR, (n, worst)


# ---------------------------------------------------------------------------------------------------- 7. the routes agree
def test_parameter_routes_give_the_same_bits_with_input_rows(hip_ctx):
    """The membrane half under GRL2, 513 nodes, two parameter sets: the per-node rows and the class bytes give, node by node, the
    bits the uniform route gives with the node's set -- the input row read by all three (tests/test_grl2_gpu.py's
    test_parameter_routes_give_the_same_bits with an input row present)."""
    model = X.membrane(GRL2)
    n, t = 513, 0.9
    Y, C, _ = X.points(n, seed=9)
    rows = np.concatenate([Y, C], axis=0)
    two = X.membrane_parameters(model, 2, seed=7)
    marks = (np.arange(n) % 2).astype(np.uint8)
    uniform = [X.launch(hip_ctx, model, "uniform", rows, np.ascontiguousarray(two[:, c]), t, X.DT, None) for c in (0, 1)]
    want = np.where(marks[None, :] == 0, uniform[0], uniform[1])
    assert np.isfinite(want).all() and not np.array_equal(uniform[0], uniform[1])
    np.testing.assert_array_equal(want[4], C[0])
    P = two[:, marks]
    np.testing.assert_array_equal(X.launch(hip_ctx, model, "per_node", rows, P, t, X.DT, None), want)
    np.testing.assert_array_equal(X.launch(hip_ctx, model, "classes", rows, P, t, X.DT, marks), want)


# ---------------------------------------------------------------------------------------------------- 8. the split equals the whole
@pytest.mark.parametrize("scheme", [GRL1, FE])
def test_one_device_step_of_the_halves_is_one_step_of_the_whole(hip_ctx, scheme):
    """Two ``_DeviceODE``s of 513 nodes (the 48 nodes of the CPU test, cyclically), each half's input rows holding the other's
    step-start rows: V, m, h, n of one and ca of the other against mpmath on small_cell.ode, within the kernel-side bound;
    the input rows unchanged.  Measured on an MI355X: 0.30 ulp under GRL1, 0.46 under forward Euler."""
    import _grl2_ref as R
    import beat
    from beat.odesolver import _DeviceODE

    w, mem, cal = X.whole(scheme), X.membrane(scheme), X.calcium(scheme)
    _, _, Y48 = X.points()
    p = R.small_parameters(w)
    ref = M.reference(X.SMALL, Y48, p, 0.9, X.DT)[scheme]
    idx = np.arange(513) % Y48.shape[1]
    inputs = {}

    def step(model, y, t, par, dt, c):
        ode = _DeviceODE(hip_ctx, model, model.num_states, y.shape[1], 0, par, beat.telemetry.NullMonitor())
        ode.states.set(np.concatenate([y, c], axis=0))
        ode.step(t, dt, v_index=model.state_index(model.v_name) if model.v_name else 0)
        inputs[model.name] = (ode.states.numpy()[model.num_states:], c)
        return ode.state_values()

    got = X.split_step(mem, cal, Y48[:, idx], 0.9, X.DT, X.half_parameters(mem, p), X.half_parameters(cal, p), step=step)
    for back, went in inputs.values():
        np.testing.assert_array_equal(back, went)
    worst, leak = M.compare(got, (ref[0][:, idx], ref[1][:, idx]), w.state_names)
    print(scheme, worst)
    assert len(inputs) == 2 and not leak and max(worst.values()) <= BOUND_TR, (worst, leak)


# ---------------------------------------------------------------------------------------------------- 9. the public interface
def _interval_space():
    from beat import grid as g

    mesh = g.create_interval(g.COMM_WORLD, CABLE_CELLS, [0.0, CABLE_CELLS * CABLE_H])
    V = g.functionspace(mesh, ("P", 1))
    return V, np.asarray(V.tabulate_dof_coordinates())[:, 0]


_TWINS = []


def _twins_on_the_interval():
    """What the three NumPy twins differ by over 40 steps of dt = 0.05 on the 64-cell interval (once per session): the coupled
    runs on the device are allowed 8 times this."""
    if not _TWINS:
        _TWINS.append(X.twin_split_against_whole(X.interval_v0(np.arange(CABLE_CELLS + 1) * CABLE_H), 40, 0.05))
    return _TWINS[0]


def test_two_coupled_solvers_against_the_monolithic_one(hip_ctx, monkeypatch):
    """The halves as two ``DolfinODESolver``s on the 64-cell interval, 40 steps of dt = 0.05 (through the file's stimulus window)
    with ``state_to_function`` -> ``missing_function`` exchanges ahead of every step, against the monolithic solver over the same
    steps; inside the loop no function's values and no state array are fetched to the host (counted).

    The allowed difference is measured, not chosen: the three NumPy twins over the same 40 steps differ by 4.75e-10 of a state's
    range at most (``_missing_ref.twin_split_against_whole``, recomputed here; ca, whose range over the interval is 1e-6 of its
    size); the bound is 8 times that, 3.80e-9 -- the margin for the table-driven exp against libm's.  Measured on an MI355X:
    1.68e-10 (profiles/missing_variables.md)."""
    from beat import grid as g
    from beat.odesolver import _DeviceODE

    demo = _demo()
    V, x = _interval_space()
    v0 = X.interval_v0(x)
    whole, mem, cal = demo.build(V, GRL1, v0)
    assert whole.on_device and mem.on_device and cal.on_device
    assert mem.shape == (4, 65) and mem.shape_missing_values == (1, 65) and cal.shape_missing_values == (3, 65)
    assert mem.values.shape == (4, 65) and cal.full_values.shape == (1, 65) and len(mem.states_to_dolfin()) == 4
    fetches = []
    host, values = g.Function._host, _DeviceODE.state_values
    monkeypatch.setattr(g.Function, "_host", lambda self: (fetches.append("function"), host(self))[1])
    monkeypatch.setattr(_DeviceODE, "state_values", lambda self: (fetches.append("states"), values(self))[1])
    demo.run(whole, mem, cal, 40, 0.05)
    assert fetches == []
    monkeypatch.undo()
    diff, w = demo.difference(whole, mem, cal)
    np.testing.assert_allclose(np.sort(x), np.arange(CABLE_CELLS + 1) * CABLE_H, rtol=0, atol=1e-12)  # (the twins' nodes)
    twins = _twins_on_the_interval()
    print(f"coupled solvers against the monolithic one: {diff:.3e} of a state's range; the twins {twins:.3e}, bound {8.0 * twins:.3e}")
    assert w[0].max() > v0.max() + 10.0  # (the stimulus has acted)
    assert diff <= 8.0 * twins, (diff, twins)
    # the rows written through the functions are resident: the NumPy array no longer decides them
    before = mem._dev.input_field(0).numpy()
    mem.missing_variables[:] = 7.0
    mem.step(2.0, 0.05)
    np.testing.assert_array_equal(mem._dev.input_field(0).numpy(), before)
    assert before.max() < 1.0


# ---------------------------------------------------------------------------------------------------- 10. the fused split step
def _cable(model, theta, parameters, guess_order=None, **missing):
    """tests/test_grl2_gpu.py's ``_device_cable`` for a given model: MonodomainSplittingSolver(theta) on the 64-cell interval,
    theta_pde = 0.5 (1 at theta = 1, so that the library's step loop is reachable), ksp_rtol 1e-13, V raised on the first six
    nodes.  ``guess_order``: a fixed order of the solve's initial guess (the adaptive default is frozen through a batch of the
    library's step loop, which then agrees with the step() loop to the solver's tolerance only: tests/test_api_gpu.py).  Returns
    (solver, the nodes' order by x)."""
    import beat
    from beat import grid as g

    V, x = _interval_space()
    mesh = V.mesh
    node = np.rint(x / CABLE_H).astype(int)
    pde = beat.MonodomainModel(time=g.Constant(mesh, 0.0), mesh=mesh, M=CABLE_D, C_m=1.0,
                               params={"theta": 1.0 if theta == 1.0 else 0.5,
                                       "petsc_options": {"ksp_rtol": 1e-13, "ksp_atol": 1e-50, **({} if guess_order is None else {"ksp_guess_order": guess_order})}})
    y0 = np.repeat(model.init_state_values()[:, None], len(x), axis=1)
    y0[model.state_index("V"), node < 6] = -20.0
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=pde.state, fun=model, init_states=y0, parameters=parameters,
                                         num_states=model.num_states, v_index=model.state_index("V"), **missing)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=theta)
    assert ode.on_device and solver._can_fuse()
    return solver, node


def _run_cable(solver, node, nsteps, dt, batched=False):
    if batched:
        solver.solve((0.0, nsteps * dt), dt=dt)
    else:
        t0 = 0.0
        for _ in range(nsteps):
            solver.step((t0, t0 + dt))
            t0 = t0 + dt
    out = np.empty((solver.ode.num_states, len(node)))
    out[:, node] = np.asarray(solver.ode.values)
    return out


# |difference of V| / (range of V) between the input-row form and the as-parameters form over the cable, measured on an MI355X:
# none at either theta -- the two kernels do the same operations on the same numbers, one reading ca from a row, the other from
# the parameter vector -- so 100 times the measured difference asks for equal bits
MEASURED_FUSED = {1.0: 0.0, 0.5: 0.0}


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_fused_split_step_with_a_constant_missing_variable(hip_ctx, theta):
    """40 fused split steps of dt = 0.025 with ``from_ode(split_membrane.ode, missing=["ca"])`` and ca = 2.5e-4 at every node,
    against the same cable with split_membrane_as_parameters.ode and ca as a uniform parameter (what runs without this
    feature).  Bound: 100 times the difference measured on an MI355X (MEASURED_FUSED, relative to the potential's range), and
    never above 1e-9 of that range (bench_parity.py's ceiling).  At theta = 1 ``solve()`` -- the library's own step loop,
    beat_split_steps -- ends on the bits of the ``step()`` loop (both with the guess order fixed at 3, the condition
    tests/test_api_gpu.py::test_batched_solve_equals_the_step_loop names for equal bits)."""
    from beat.models import from_ode

    mem, ref = X.membrane(), from_ode(X.AS_PARAMETERS)
    nsteps, dt = 40, 0.025
    p = mem.init_parameter_values(stim_amplitude=0.0)
    missing = dict(missing_variables=np.full((1, CABLE_CELLS + 1), CA0), num_missing_variables=1)
    a = _run_cable(*_cable(mem, theta, p, **missing), nsteps, dt)
    b = _run_cable(*_cable(ref, theta, ref.init_parameter_values(stim_amplitude=0.0, ca=CA0)), nsteps, dt)
    span = b[0].max() - b[0].min()
    diff = float(np.abs(a[0] - b[0]).max() / span)
    print(f"theta = {theta}: input row against parameter, {diff:.3e} of the potential's range ({span:.1f} mV)")
    assert b[0, 6:].max() > -20.0 and span > 50.0  # (the front has left the nodes that were raised)
    assert diff <= min(100.0 * MEASURED_FUSED[theta], 1e-9), diff
    if theta == 1.0:
        looped = _run_cable(*_cable(mem, theta, p, guess_order=3, **missing), nsteps, dt)
        solver, node = _cable(mem, theta, p, guess_order=3, **missing)
        assert solver._can_batch(None)
        np.testing.assert_array_equal(_run_cable(solver, node, nsteps, dt, batched=True), looped)
        assert np.abs(looped[0] - a[0]).max() <= 1e-6 * span


# ---------------------------------------------------------------------------------------------------- 11. the live array
def _membrane_solver(c, init=None):
    import beat
    from beat import grid as g

    V, x = _interval_space()
    mem = X.membrane()
    y0 = np.repeat(mem.init_state_values()[:, None], len(x), axis=1)
    y0[0] = X.interval_v0(x)
    return beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=mem, init_states=y0 if init is None else init,
                                          parameters=mem.init_parameter_values(), num_states=4, v_index=0, missing_variables=c,
                                          num_missing_variables=1)


def test_live_array_is_seen_by_the_next_step(hip_ctx):
    """``missing_variables[:] = ...`` between two steps changes the second step exactly as a fresh solver built with the edited
    array on the states the first step left: bits equal (and not the bits of a run without the edit).  ``None`` is the model's
    ``init_missing_values()``; an (M,) vector is broadcast."""
    rng = np.random.default_rng(5)
    c0, c1 = 10.0 ** rng.uniform(-4.5, -2.5, (1, 65)), 10.0 ** rng.uniform(-4.5, -2.5, (1, 65))
    live = c0.copy()
    a, plain = _membrane_solver(live), _membrane_solver(c0.copy())
    a.step(0.6, 0.05)
    plain.step(0.6, 0.05)
    after_one = np.asarray(a.values).copy()
    np.testing.assert_array_equal(after_one, np.asarray(plain.values))
    live[:] = c1
    a.step(0.65, 0.05)
    plain.step(0.65, 0.05)
    fresh = _membrane_solver(c1.copy(), init=after_one)
    fresh.step(0.65, 0.05)
    np.testing.assert_array_equal(np.asarray(a.values), np.asarray(fresh.values))
    assert not np.array_equal(np.asarray(a.values), np.asarray(plain.values))
    zero, vec = _membrane_solver(None), _membrane_solver(np.zeros(1))
    zero.step(0.6, 0.05)
    vec.step(0.6, 0.05)
    np.testing.assert_array_equal(np.asarray(zero.values), np.asarray(vec.values))
    np.testing.assert_array_equal(np.asarray(zero.missing_function("ca").x.array), np.zeros(65))
    vec.set_missing("ca", c0[0])  # (resident from here on: the array is no longer consulted)
    vec.step(0.65, 0.05)
    zero.set_missing("ca", plain.missing_function("ca"))
    zero.step(0.65, 0.05)
    np.testing.assert_array_equal(np.asarray(zero.values), np.asarray(vec.values))


# ---------------------------------------------------------------------------------------------------- 12. the monitor
def test_monitor_reads_the_input_rows_and_leaves_the_run_alone(hip_ctx):
    """``ode.monitor(["i_out"], t)`` on the membrane half against ``numpy_monitor(..., missing_variables=...)``, to 1e-6 of each
    value or of its row's scale (``OdeFileModel.monitor_error``); a fused run that monitors after steps 3 and 8 ends on the bits
    of one that does not."""
    mem = X.membrane()
    rng = np.random.default_rng(6)
    c = 10.0 ** rng.uniform(-4.5, -2.5, (1, CABLE_CELLS + 1))
    p = mem.init_parameter_values(stim_amplitude=0.0)
    missing = lambda: dict(missing_variables=c.copy(), num_missing_variables=1)  # noqa: E731
    (a, node), (b, _) = _cable(mem, 1.0, p, **missing()), _cable(mem, 1.0, p, **missing())
    dt, t0 = 0.025, 0.0
    for i in range(12):
        a.step((t0, t0 + dt))
        b.step((t0, t0 + dt))
        t0 = t0 + dt
        if i + 1 in (3, 8):
            funs = b.ode.monitor(["i_out", "dV_dt"], t0)
            dev = np.array([np.asarray(f.x.array) for f in funs])
            ref = mem.numpy_monitor(b.ode.full_values, t0, p, ["i_out", "dV_dt"], missing_variables=c)
            err = mem.monitor_error(dev, ref)
            print(f"monitor after step {i + 1}: {err.max():.3e}")
            assert err.max() <= 1e-6 and np.abs(ref[0]).max() > 0.0
    assert np.asarray(a.ode.full_values).tobytes() == np.asarray(b.ode.full_values).tobytes()
    assert np.asarray(a.pde.state.x.array).tobytes() == np.asarray(b.pde.state.x.array).tobytes()
    # staged: monitor_values with missing_variables, (S,) and (M,) too
    y = np.asarray(b.ode.full_values)
    dev = mem.monitor_values(t0, y, p, ["i_out"], missing_variables=c)
    assert mem.monitor_error(dev, mem.numpy_monitor(y, t0, p, ["i_out"], missing_variables=c)).max() <= 1e-6
    np.testing.assert_array_equal(mem.monitor_values(t0, y[:, 0], p, ["i_out"], missing_variables=c[:, 0]), dev[:, 0])


# ---------------------------------------------------------------------------------------------------- 13. the in-kernel loop
def test_in_kernel_loop_holds_the_missing_variables(hip_ctx):
    """``model.run(..., missing_variables=c)`` for 200 steps equals 200 calls of ``model(...)``, bit for bit, for (M, N) and (M,)
    values; the input rows come back unchanged; ``single_cell.get_steady_state`` passes them on."""
    from beat.models._base import DeviceModel

    mem = X.membrane()
    Y, C, _ = X.points(65, seed=11)
    p, dt = mem.init_parameter_values(), 0.025
    out, track = mem.run(Y, p, dt, 200, track_indices=[0], missing_variables=C)
    y = Y.copy()
    for j in range(200):
        y = mem(states=y, t=j * dt, parameters=p, dt=dt, missing_variables=C)
    assert out.shape == (4, 65) and track.shape == (200, 1, 65) and np.isfinite(out).all()
    np.testing.assert_array_equal(out, y)
    rows, _ = DeviceModel.run(mem, np.concatenate([Y, C], axis=0), p, dt, 200)
    np.testing.assert_array_equal(rows[4:], C)
    np.testing.assert_array_equal(rows[:4], out)
    one, _ = mem.run(Y[:, 3], p, dt, 200, missing_variables=C[:, 3])
    np.testing.assert_array_equal(one, out[:, 3])
    with pytest.raises(TypeError):
        mem.run(Y, p, dt, 2)


def test_steady_state_with_constant_missing_variables(hip_ctx, tmp_path):
    import beat

    mem = X.membrane()
    y0, p, c = mem.init_state_values(), mem.init_parameter_values(), np.array([CA0])
    got = beat.single_cell.get_steady_state(mem, y0, p, tmp_path, nbeats=2, BCL=5, dt=0.05, missing_variables=c)
    want, _ = mem.run(y0, p, 0.05, len(np.arange(0.0, 5, 0.05)), nbeats=2, missing_variables=c)
    np.testing.assert_array_equal(got, want)
    other = beat.single_cell.get_steady_state(mem, y0, p, tmp_path, nbeats=2, BCL=5, dt=0.05, missing_variables=2.0 * c)
    assert not np.array_equal(other, got)  # (the values are part of the cache key)


# ---------------------------------------------------------------------------------------------------- 14. loud errors
def test_errors_instead_of_silence(hip_ctx):
    import beat
    from beat import grid as g
    from beat.models import tp06

    V, x = _interval_space()
    n = len(x)

    def solver(fun, init, parameters=None, **kw):
        return beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=fun, init_states=init,
                                              parameters=fun.init_parameter_values() if parameters is None else parameters,
                                              num_states=len(init), v_index=0, **kw)

    for count in (0, 1):  # (the array was ignored before; whatever num_missing_variables says, the model takes none)
        with pytest.raises(ValueError, match="tp06_generalized_rush_larsen"):
            solver(tp06.generalized_rush_larsen, tp06.init_state_values(), tp06.init_parameter_values(), missing_variables=np.zeros((1, n)),
                   num_missing_variables=count)
    with pytest.raises(ValueError, match="small_cell"):
        solver(X.whole(), X.whole().init_state_values(), missing_variables=np.zeros((1, n)))
    mem = X.membrane()
    with pytest.raises(ValueError, match="num_missing_variables"):
        solver(mem, mem.init_state_values(), missing_variables=np.zeros((1, n)), num_missing_variables=2)
    with pytest.raises(ValueError, match="num_missing_variables"):
        solver(mem, mem.init_state_values(), missing_variables=np.zeros((1, n)))
    with pytest.raises(ValueError, match="shape"):
        solver(mem, mem.init_state_values(), missing_variables=np.zeros((2, n)), num_missing_variables=1)
    markers = g.Function(V)
    markers.x.array[:] = np.where(x < 7.1, 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="missing variables"):
        beat.odesolver.DolfinMultiODESolver(
            v_ode=g.Function(V), v_pde=g.Function(V), markers=markers, num_states={k: 4 for k in (0, 1)}, fun={k: mem for k in (0, 1)},
            init_states={k: mem.init_state_values() for k in (0, 1)}, parameters={k: mem.init_parameter_values() for k in (0, 1)},
            v_index={k: 0 for k in (0, 1)})
    ok = solver(mem, mem.init_state_values(), missing_variables=np.zeros((1, n)), num_missing_variables=1)
    with pytest.raises(KeyError):
        ok.missing_function("V")
    small = g.Function(g.functionspace(g.create_interval(g.COMM_WORLD, 8, [0.0, 2.0]), ("P", 1)))
    with pytest.raises(ValueError, match="values"):  # (a device copy is as long as its destination: sizes must agree)
        ok.set_missing("ca", small)
    with pytest.raises(ValueError, match="values"):
        ok.state_to_function("V", small)
    with pytest.raises(ValueError):
        solver(X.whole(), X.whole().init_state_values()).missing_function("ca")


# ---------------------------------------------------------------------------------------------------- 15. the demo
def test_split_cell_demo(hip_ctx, capsys):
    """demos/split_cell.py at its smallest size -- the two coupled halves against the whole model on the 364 nodes of a slab, the
    same 40 steps and the same spread of initial potentials as the interval's -- prints a difference under the bound of
    test_two_coupled_solvers_against_the_monolithic_one: 8 times what the twins differ by there, 3.80e-9 of a state's range.
    Measured on an MI355X: 1.68e-10."""
    diff, w, (whole, mem, cal) = _demo().main(["--dx", "0.5", "--steps", "40"])
    out = capsys.readouterr().out
    assert "status OK" in out and f"largest difference {diff:.3e}" in out
    print(f"demo: {diff:.3e}; bound {8.0 * _twins_on_the_interval():.3e}")
    assert w.shape[1] == 364 and diff <= 8.0 * _twins_on_the_interval(), diff
