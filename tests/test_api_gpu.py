"""GPU tests of the reference-shaped Python API.  They restate the reference's own tests
(tests/test_monodomain.py, tests/test_stimulation.py, tests/test_odesolver.py,
tests/test_monodomain_solver.py) and the Niederer table (demos/niederer_benchmark.py:315-319)
against the HIP backend, with the reference's thresholds."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _ctx(hip_ctx):
    return hip_ctx


def _l2_error(mesh, vh, exact):
    from oracle import fem

    om = fem.BoxMesh(mesh.n, tuple(u - l for l, u in zip(mesh.lower, mesh.upper)), origin=mesh.lower)
    return fem.l2_error(om, np.asarray(vh), exact)


# ---- tests/test_monodomain.py:11-64 ---------------------------------------------------------------
@pytest.mark.parametrize(
    "M, amp, err",
    [
        (0.0, lambda g, t: g.cos(t), 1e-4),
        (1.0, lambda g, t: g.cos(t) + 8 * g.pi**2 * g.sin(t), 2e-4),
        (2.0, lambda g, t: g.cos(t) + 16 * g.pi**2 * g.sin(t), 2e-4),
    ],
)
def test_monodomain_analytic(M, amp, err):
    import beat
    from beat import grid as g

    N, theta, dt = 15, 0.5, 0.001
    T = 10 * dt
    mesh = g.create_unit_square(g.COMM_WORLD, N, N, g.CellType.triangle)
    time = g.Constant(mesh, g.default_scalar_type(0.0))
    x = g.SpatialCoordinate(mesh)
    t_var = g.variable(time)
    I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * amp(g, t_var)
    model = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, params=dict(theta=theta, linear_solver_type="direct"))
    res = model.solve((0, T), dt=dt)
    e = _l2_error(mesh, res.state.x.array, lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(T))
    assert e < err


# ---- tests/test_monodomain.py:67-104 --------------------------------------------------------------
def test_monodomain_spatial_convergence():
    import beat
    from beat import grid as g

    errors = []
    dt = 0.001
    T = 10 * dt
    for N in (4, 8, 16, 32):
        mesh = g.create_unit_square(g.COMM_WORLD, N, N)
        time = g.Constant(mesh, 0.0)
        x = g.SpatialCoordinate(mesh)
        I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * (g.cos(time) + 8 * g.pi**2 * g.sin(time))
        model = beat.MonodomainModel(time=time, mesh=mesh, M=1.0, I_s=I_s, params=dict(theta=0.5))
        res = model.solve((0, T), dt=dt)
        errors.append(_l2_error(mesh, res.state.x.array,
                                lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(T)))
    rates = [np.log(e1 / e2) / np.log(2) for e1, e2 in zip(errors[:-1], errors[1:])]
    assert all(rate >= 2.0 for rate in rates), rates


# ---- tests/test_monodomain.py:107-147 (coarser N to keep it quick; same criterion) ------------------
def test_monodomain_temporal_convergence():
    import beat
    from beat import grid as g

    T, N = 1.0, 100
    mesh = g.create_unit_square(g.COMM_WORLD, N, N)
    x = g.SpatialCoordinate(mesh)
    errors = []
    for dt in (1.0, 0.5, 0.25, 0.125):
        time = g.Constant(mesh, 0.0)
        I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * (g.cos(time) + 8 * g.pi**2 * g.sin(time))
        model = beat.MonodomainModel(time=time, mesh=mesh, M=1.0, I_s=I_s, params=dict(theta=0.5))
        res = model.solve((0, T), dt=dt)
        errors.append(_l2_error(mesh, res.state.x.array,
                                lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(T)))
    rates = [np.log(e1 / e2) / np.log(2) for e1, e2 in zip(errors[:-1], errors[1:])]
    assert all(rate >= 2.0 for rate in rates), rates


# ---- tests/test_stimulation.py:12-48 ---------------------------------------------------------------
def test_single_stimulation():
    import beat
    from beat import grid as g

    mesh = g.create_unit_interval(g.COMM_WORLD, 10)
    value, end, start, dt = 2.0, 1.0, 0.5, 0.01
    time = g.Constant(mesh, 0.0)
    expr = g.conditional(g.And(g.ge(time, start), g.le(time, end)), value, 0.0)
    I_s = beat.stimulation.Stimulus(dZ=g.dx(domain=mesh), expr=expr)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=g.Constant(mesh, 0.0), I_s=I_s)
    pde.step((0.0, 0.4))
    assert np.allclose(pde.state.x.array, 0.0)
    t0 = 0.9
    pde.solve((0.4, t0), dt=dt)
    assert np.allclose(pde.state.x.array, value * (t0 - start))
    pde.solve((t0, end + dt), dt=dt)
    # solve() does not assign_previous() after its final step: hence the "- dt"
    assert np.allclose(pde.state.x.array, (end - start - dt) * value)
    pde.solve((end + dt, 2 * end), dt=dt)
    assert np.allclose(pde.state.x.array, (end - start - dt) * value)


# ---- tests/test_stimulation.py:51-107 --------------------------------------------------------------
def test_double_stimulation():
    import beat
    from beat import grid as g

    mesh = g.create_unit_interval(g.COMM_WORLD, 10)
    dt, value1, value2 = 0.01, 2.0, 3.0
    start1, end1, start2, end2 = 0.5, 1.0, 0.9, 1.5
    time = g.Constant(mesh, 0.0)
    expr1 = g.conditional(g.And(g.ge(time, start1), g.le(time, end1)), value1, 0.0)
    expr2 = g.conditional(g.And(g.ge(time, start2), g.le(time, end2)), value2, 0.0)
    dx = g.dx(domain=mesh)
    I_s = [beat.stimulation.Stimulus(dZ=dx, expr=expr1), beat.stimulation.Stimulus(dZ=dx, expr=expr2)]
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=g.Constant(mesh, 0.0), I_s=I_s)
    pde.step((0.0, 0.4))
    assert np.allclose(pde.state.x.array, 0.0)
    t0 = 0.9
    pde.solve((0.4, t0), dt=dt)
    assert np.allclose(pde.state.x.array, value1 * (t0 - start1))
    pde.solve((t0, end1 + dt), dt=dt)
    assert np.allclose(pde.state.x.array, (end1 - start1 - dt) * value1 + (end1 + dt - start2) * value2)
    pde.solve((end1 + dt, end2 + dt), dt=dt)
    assert np.allclose(pde.state.x.array, (end1 - start1 - dt) * value1 + (end2 - start2 - dt) * value2)
    pde.solve((end2 + dt, 2 * end2), dt=dt)
    assert np.allclose(pde.state.x.array, (end1 - start1 - dt) * value1 + (end2 - start2 - dt) * value2)


# ---- tests/test_stimulation.py:253-304: integral of define_stimulus over the marked region -----------
def test_define_stimulus_integral():
    import beat
    from beat import grid as g

    mesh = g.create_unit_cube(g.COMM_WORLD, 4, 4, 4)
    time = g.Constant(mesh, 0.0)
    cells = g.locate_entities(mesh, 3, lambda x: x[0] <= 0.5 + 1e-12)
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    chi, amplitude = 1400.0, 50000.0
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=chi * beat.units.ureg("cm**-1"), time=time,
                                           subdomain_data=tags, marker=1, mesh_unit="mm", amplitude=amplitude,
                                           duration=2.0, start=1.0)
    expected = (amplitude * beat.units.ureg("uA/cm**3") / (chi * beat.units.ureg("cm**-1"))).to("uA/mm**2").magnitude
    w = beat.stimulation.assemble_weights(mesh, I_s.dz.cells(), None)
    for t, on in ((0.5, False), (1.0, True), (2.0, True), (3.0, True), (3.1, False)):
        time.value = t
        assert np.isclose(float(I_s.expr.evaluate()) * w.sum(), (expected * 0.5) if on else 0.0)


# ---- tests/test_odesolver.py:52-117 ----------------------------------------------------------------
def _simple_ode_forward_euler(states, t, dt, parameters):
    v, s = states
    a, b = parameters
    values = np.zeros_like(states)
    values[0] = v - a * s * dt
    values[1] = s + b * v * dt
    return values


@pytest.mark.parametrize("device_model", [False, True])
def test_DolfinODESolver_data_movement(device_model):
    import beat
    from beat import grid as g
    from beat.odesolver import DolfinODESolver

    mesh = g.create_unit_square(g.COMM_WORLD, 5, 5)
    v_pde = g.Function(g.functionspace(mesh, ("P", 1)))
    v_ode = g.Function(g.functionspace(mesh, ("P", 1)))
    N_ode = 36
    v0, s0 = 1.0, 2.0
    fun = beat.models.simple.forward_euler if device_model else _simple_ode_forward_euler
    ode = DolfinODESolver(v_ode=v_ode, v_pde=v_pde, init_states=np.array([v0, s0]), parameters=np.array([1, 1]),
                          fun=fun, num_states=2, v_index=0)
    assert ode.on_device == device_model
    assert ode.full_values.shape == (2, N_ode) and ode.values.shape == (2, N_ode)
    assert np.allclose(ode.values[0, :], v0) and np.allclose(ode.values[1, :], s0)
    dt = 0.1
    ode.step(0.0, dt)
    assert np.allclose(ode.values[0, :], v0 - s0 * dt)
    assert np.allclose(ode.values[1, :], s0 + v0 * dt)
    assert np.allclose(v_ode.x.array, 0.0)
    ode.to_dolfin()
    assert np.allclose(v_ode.x.array, v0 - s0 * dt)
    assert np.allclose(v_pde.x.array, 0.0)
    ode.ode_to_pde()
    assert np.allclose(v_pde.x.array, v0 - s0 * dt)
    v_pde.x.array[:] = 1.0
    ode.pde_to_ode()
    assert np.allclose(v_ode.x.array, 1.0)
    ode.from_dolfin()
    assert np.allclose(ode.values[0, :], 1.0)
    assert np.allclose(ode.values[1, :], s0 + v0 * dt)
    states = ode.states_to_dolfin()
    assert len(states) == 2
    assert np.allclose(states[0].x.array, 1.0)
    assert np.allclose(states[1].x.array, s0 + v0 * dt)


# ---- tests/test_odesolver.py:120-215 (two markers, per-marker parameters) ---------------------------
@pytest.mark.parametrize("device_model", [False, True])
def test_DolfinMultiODESolver(device_model):
    import beat
    from beat import grid as g
    from beat.odesolver import DolfinMultiODESolver

    mesh = g.create_unit_square(g.COMM_WORLD, 5, 5)
    V = g.functionspace(mesh, ("P", 1))
    v_pde, v_ode, markers = g.Function(V), g.Function(V), g.Function(V)
    marr = np.zeros(36)
    marr[:10] = 1
    markers.x.array[:] = marr
    fun = beat.models.simple.forward_euler if device_model else _simple_ode_forward_euler
    init = {0: np.array([1.0, 2.0]), 1: np.array([3.0, 4.0])}
    par = {0: np.array([1.0, 1.0]), 1: np.array([2.0, 0.5])}
    ode = DolfinMultiODESolver(v_ode=v_ode, v_pde=v_pde, markers=markers, init_states=init, parameters=par,
                               fun={0: fun, 1: fun}, num_states={0: 2, 1: 2}, v_index={0: 0, 1: 0})
    assert ode.values(0).shape == (2, 26) and ode.values(1).shape == (2, 10)
    dt = 0.1
    ode.step(0.0, dt)
    assert np.allclose(ode.values(0)[0], 1.0 - 1.0 * 2.0 * dt) and np.allclose(ode.values(0)[1], 2.0 + 1.0 * 1.0 * dt)
    assert np.allclose(ode.values(1)[0], 3.0 - 2.0 * 4.0 * dt) and np.allclose(ode.values(1)[1], 4.0 + 0.5 * 3.0 * dt)
    assert np.allclose(v_ode.x.array, 0.0)
    ode.to_dolfin()
    expect = np.where(marr == 1, 3.0 - 2.0 * 4.0 * dt, 1.0 - 2.0 * dt)
    assert np.allclose(v_ode.x.array, expect)
    ode.ode_to_pde()
    assert np.allclose(v_pde.x.array, expect)
    v_pde.x.array[:] = np.arange(36.0)
    ode.pde_to_ode()
    ode.from_dolfin()
    assert np.allclose(ode.values(1)[0], np.arange(10.0)) and np.allclose(ode.values(0)[0], np.arange(10.0, 36.0))
    fv = ode.full_values
    assert fv.shape == (2, 36) and np.allclose(fv[0], np.arange(36.0))


# ---- tests/test_monodomain_solver.py:33-87 (P1 ODE space) -------------------------------------------
@pytest.mark.parametrize("mode", ["device_fused", "device_unfused", "host_callable"])
def test_monodomain_splitting_analytic(mode):
    import beat
    from beat import grid as g

    N, M, dt, T, t0 = 50, 1.0, 0.01, 1.0, 0.0
    mesh = g.create_unit_square(g.COMM_WORLD, N, N)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    I_s = 8 * g.pi**2 * g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * g.sin(time)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s)
    V_ode = beat.utils.space_from_string("P_1", mesh, dim=1)
    v_ode = g.Function(V_ode)
    s = g.Function(V_ode)
    s.interpolate(lambda p: -np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.cos(0.0))
    init_states = np.zeros((2, s.x.array.size))
    init_states[1, :] = np.asarray(s.x.array)

    def simple(states, t, dt, parameters):
        v, s_ = states
        values = np.zeros_like(states)
        values[0] = v - s_ * dt
        values[1] = s_ + v * dt
        return values

    fun = simple if mode == "host_callable" else beat.models.simple.forward_euler
    ode = beat.odesolver.DolfinODESolver(v_ode=v_ode, v_pde=pde.state, fun=fun, init_states=init_states,
                                         parameters=None, num_states=2, v_index=0)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, fused=(mode != "device_unfused"))
    solver.solve((t0, T), dt=dt)
    E = _l2_error(mesh, pde.state.x.array,
                  lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(float(time)))
    assert E < 0.002
    # every N-vector the reference keeps in sync is in sync
    assert np.array_equal(np.asarray(pde.v_.x.array), np.asarray(pde.state.x.array))
    assert np.array_equal(np.asarray(ode.v_ode.x.array), np.asarray(pde.state.x.array))
    assert np.array_equal(ode.values[0], np.asarray(pde.state.x.array))


def _split_error(N, dt, theta=1.0, T=1.0, odespace="CG_1"):
    """L2 error at t = T of the split system of tests/test_monodomain_solver.py (v = cos cos sin t, s = -cos cos cos t,
    forward-Euler ODE on the device; ODE space CG_1, CG_2 or DG_1 as the reference parametrises it)."""
    import beat
    from beat import grid as g

    mesh = g.create_unit_square(g.COMM_WORLD, N, N)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    I_s = 8 * g.pi**2 * g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * g.sin(time)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=1.0, I_s=I_s)
    V_ode = beat.utils.space_from_string(odespace, mesh, dim=1)
    s = g.Function(V_ode)
    s.interpolate(lambda p: -np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]))
    init_states = np.zeros((2, s.x.array.size))
    init_states[1, :] = np.asarray(s.x.array)
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V_ode), v_pde=pde.state, fun=beat.models.simple.forward_euler,
                                         init_states=init_states, parameters=None, num_states=2, v_index=0)
    assert ode.num_points == V_ode.num_dofs
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=theta)
    solver.solve((0.0, T), dt=dt)
    return _l2_error(mesh, pde.state.x.array,
                     lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(float(time)))


@pytest.mark.parametrize("odespace", ["CG_1", "CG_2", "DG_1"])
def test_monodomain_splitting_analytic_other_ode_spaces(odespace):
    """tests/test_monodomain_solver.py:33-87 with the ODE on a P2 / DG1 space (transfers by interpolation,
    utils.local_project): N = 50, dt = 0.01 -> error < 0.002 as for the P1 ODE space."""
    if odespace == "CG_1":
        pytest.skip("covered by test_monodomain_splitting_analytic")
    assert _split_error(50, 0.01, odespace=odespace) < 0.002


@pytest.mark.parametrize("odespace", ["CG_1", "CG_2", "DG_1"])
def test_monodomain_splitting_spatial_convergence(odespace):
    """tests/test_monodomain_solver.py:90-149: N = 8, 16, 32 at dt = 0.001 -> average rate > 1.85."""
    errors = [_split_error(2**level, 0.001, odespace=odespace) for level in range(3, 6)]
    rates = [np.log2(e1 / e2) for e1, e2 in zip(errors[:-1], errors[1:])]
    assert sum(rates) / len(rates) > 1.85, (errors, rates)


@pytest.mark.parametrize("odespace", ["CG_1", "CG_2", "DG_1"])
def test_monodomain_splitting_temporal_convergence(odespace):
    """tests/test_monodomain_solver.py:152-216 (theta = 1): N = 150, dt = 1/8, 1/16, 1/32 -> average rate > 1."""
    errors = [_split_error(150, 1.0 / 2**level, odespace=odespace) for level in range(3, 6)]
    rates = [np.log2(e1 / e2) for e1, e2 in zip(errors[:-1], errors[1:])]
    assert sum(rates) / len(rates) > 1.0, (errors, rates)


def _tp06_slab(fused, theta=1.0, nsteps=40, stim=True, ksp_rtol=None, model=None, v_name="V", model_stimulus="stim_amplitude"):
    import beat
    from beat import grid as g
    from beat.models import tp06

    tp06 = tp06 if model is None else model  # (any built-in cell model with the same module interface)

    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=4.0, Ly=2.0, Lz=1.0, dx=0.25)
    mesh = geo.mesh
    time = g.Constant(mesh, 0.0)
    cond = beat.conductivities.default_conductivities("Niederer")
    cells = g.locate_entities(mesh, 3, lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                           mesh_unit="mm", amplitude=50_000.0 if stim else 0.0)
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
    params = None if ksp_rtol is None else {"petsc_options": {"ksp_type": "cg", "ksp_rtol": ksp_rtol}}
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ, params=params)
    ode = beat.odesolver.DolfinODESolver(
        v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
        init_states=tp06.init_state_values(), parameters=tp06.init_parameter_values(**{model_stimulus: 0.0}),
        num_states=len(tp06.init_state_values()), v_index=tp06.state_index(v_name))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=theta, fused=fused)
    dt = 0.05
    for i in range(nsteps):
        solver.step((i * dt, (i + 1) * dt))
    return solver


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_fused_step_equals_reference_sequence(theta):
    """The fused route (in-place solve on the V row, aliased functions; for theta < 1 the corrective ionic kernel
    after the solve) gives the same numbers as the literal reference sequence (monodomain_solver.py:53-116)."""
    a, b = _tp06_slab(True, theta=theta), _tp06_slab(False, theta=theta)
    va, vb = np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array)
    assert va.max() > 0.0  # the stimulated corner fired
    np.testing.assert_allclose(va, vb, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a.ode.values, b.ode.values, rtol=1e-12, atol=1e-14)
    for s in (a, b):
        assert np.array_equal(np.asarray(s.pde.v_.x.array), np.asarray(s.pde.state.x.array))
        assert np.array_equal(s.ode.values[17], np.asarray(s.pde.state.x.array))


def test_fused_aliases_materialise_when_values_diverge():
    s = _tp06_slab(True, nsteps=3)
    before = np.asarray(s.pde.state.x.array).copy()
    s.ode.step(0.15, 0.05)  # manual sub-step: the V row changes, pde.state must not
    assert np.array_equal(np.asarray(s.pde.state.x.array), before)
    assert not np.array_equal(s.ode.values[17], before)
    s.pde.state.x.array[:] = 1.0  # writing one function must not leak into the others
    assert np.array_equal(np.asarray(s.pde.v_.x.array), before)


def test_strang_splitting_against_oracle():
    """theta = 0.5 (corrective ODE half-step, monodomain_solver.py:98-113) against the oracle (sparse-LU
    diffusion solves).  PCG is run to rtol 1e-13 here so that what is compared is the arithmetic, not
    the linear-solver tolerance; the stimulated corner is in its upstroke, which amplifies rounding
    differences (libm exp/log) by ~1e3, hence 1e-7."""
    from oracle import fem, ionic

    s = _tp06_slab(False, theta=0.5, nsteps=10, ksp_rtol=1e-13)
    mesh = fem.BoxMesh((16, 8, 4), (4.0, 2.0, 1.0))
    M = np.diag([0.0009529837251356239, 0.00012575841147269718, 0.00012575841147269718])
    cells = mesh.locate_cells(lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
    w = fem.stimulus_weights(mesh, cells)
    amp = 50000.0 / 1400.0 / 100.0
    model = fem.OracleMonodomainModel(mesh, M, [fem.OracleStimulus(fem.window(0.0, 2.0, amp), w)], C_m=0.01, theta=0.5)
    S = np.repeat(ionic.tp06_init_state_values()[:, None], mesh.num_nodes, axis=1)
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    dt = 0.05
    for i in range(10):
        t0 = i * dt
        S = ionic.tp06_generalized_rush_larsen(S, t0, 0.5 * dt, P)
        model.state[:] = S[17]
        model.assign_previous()
        model.step((t0, t0 + dt))
        S[17] = model.state
        S = ionic.tp06_generalized_rush_larsen(S, t0 + 0.5 * dt, 0.5 * dt, P)
    out = s.ode.values
    err = np.abs(out - S) / np.maximum(np.abs(S), 1e-3)
    assert err.max() < 1e-7, err.max()


def test_isotropic_slab_tp06_trajectory_against_oracle():
    """BASELINE.json configs[2] in small: the benchmark's own isotropic set-up (bench.py --iso: M = 9.5301e-4 I, h = 0.1 mm,
    C_m = 0.01, theta_pde = 0.5, Godunov splitting, dt = 0.01, TP06 GRL1 at the Niederer initial values, a 60 mV Gaussian
    bump on V and 1 % noise on the other states, no stimulus) through the public API -- fused split step, default
    adaptive initial guess -- against the oracle (NumPy TP06 + literally assembled P1 matrices + sparse LU) over 40
    steps: every state of every node to 1e-8 relative."""
    import beat
    from beat import grid as g
    from beat.models import tp06
    from oracle import fem, ionic

    cells, h, dt, nsteps = (20, 16, 12), 0.1, 0.01, 40
    L = tuple(c * h for c in cells)
    M = 9.5301e-4 * np.eye(3)
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(L)], list(cells))
    time = g.Constant(mesh, 0.0)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, C_m=0.01, params={"theta": 0.5, "petsc_options": {"ksp_rtol": 1e-13, "ksp_atol": 1e-50}})
    ic = tp06.init_state_values()
    vi = tp06.state_index("V")
    om = fem.BoxMesh(cells, L)
    rng = np.random.default_rng(1234)
    S0 = np.repeat(ic[:, None], om.num_nodes, axis=1) * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, (19, om.num_nodes)))
    S0[vi] = ic[vi] + 60.0 * np.exp(-((om.x - 0.5 * np.array(L)) ** 2).sum(axis=1) / (2.0 * 0.4**2))
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state,
                                         fun=tp06.generalized_rush_larsen, init_states=S0,
                                         parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=19, v_index=vi)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    model = fem.OracleMonodomainModel(om, M, [], C_m=0.01, theta=0.5)
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    S = S0.copy()
    its = []
    for i in range(nsteps):
        t0 = i * dt
        solver.step((t0, t0 + dt))
        its.append(pde.ksp.getIterationNumber())
        S = ionic.tp06_generalized_rush_larsen(S, t0, dt, P)
        model.state[:] = S[vi]
        model.assign_previous()
        model.step((t0, t0 + dt))
        S[vi] = model.state
    out = np.asarray(ode.values)
    err = np.abs(out - S) / np.maximum(np.abs(S), 1e-3)
    assert err.max() < 1e-8, err.max()
    assert out[vi].max() > -40.0 and out[vi].min() < -80.0  # the bump is still up, the far field at rest
    assert all(k <= 40 for k in its) and np.mean(its[10:]) < np.mean(its[:3])  # the extrapolated guess took over


@pytest.mark.parametrize("fused", [True, False])
def test_land_cell_model_in_the_split_step_against_oracle(fused):
    """The 52-state ToR-ORd + Land model (beat.models.torord_land, odes/torord/ToRORd_dynCl_endo_Land.ode) as ``fun`` of
    the splitting solver on the slab of the tests above: 40 steps of 0.05 ms with a corner stimulus against the oracle
    (oracle/torord.py ionic step + sparse-LU diffusion), PCG at rtol 1e-13 so that the arithmetic is compared; the
    potential lives in row 41 and calcium in row 44 of this model."""
    from beat.models import torord_land as tl
    from oracle import fem
    from oracle import torord as otor

    nsteps, dt = 40, 0.05
    s = _tp06_slab(fused, nsteps=nsteps, ksp_rtol=1e-13, model=tl, v_name="v", model_stimulus="i_Stim_Amplitude")
    mesh = fem.BoxMesh((16, 8, 4), (4.0, 2.0, 1.0))
    M = np.diag([0.0009529837251356239, 0.00012575841147269718, 0.00012575841147269718])
    cells = mesh.locate_cells(lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
    w = fem.stimulus_weights(mesh, cells)
    amp = 50000.0 / 1400.0 / 100.0
    model = fem.OracleMonodomainModel(mesh, M, [fem.OracleStimulus(fem.window(0.0, 2.0, amp), w)], C_m=0.01, theta=0.5)
    S = np.repeat(otor.torord_land_init_state_values()[:, None], mesh.num_nodes, axis=1)
    P = otor.torord_land_init_parameter_values(i_Stim_Amplitude=0.0)
    vi = otor.TORORD_LAND_STATES.index("v")
    assert vi == tl.state_index("v") == 41
    for i in range(nsteps):
        t0 = i * dt
        S = otor.torord_land_generalized_rush_larsen(S, t0, dt, P)
        model.state[:] = S[vi]
        model.assign_previous()
        model.step((t0, t0 + dt))
        S[vi] = model.state
    out = s.ode.values
    assert S[vi].max() > 0.0 and np.array_equal(out[vi], np.asarray(s.pde.state.x.array))
    err = np.abs(out - S) / np.maximum(np.abs(S), 1e-6 * np.abs(S[:, :1]) + 1e-12)
    assert err.max() < 1e-7, (err.max(), otor.TORORD_LAND_STATES[np.unravel_index(err.argmax(), err.shape)[0]])


_POINTS = ("P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8", "P9")
NIEDERER_TABLE = {  # demos/niederer_benchmark.py:315-325: (dx, dt) -> activation times at P1..P9 in ms
    (0.5, 0.05): (1.25, 51.1, 34.9, 58.9, 14.1, 49.5, 34.0, 56.65, 26.05),
    (0.5, 0.01): (1.22, 50.85, 33.96, 58.05, 13.98, 49.36, 33.07, 55.91, 25.64),
    (0.5, 0.005): (1.215, 50.775, 33.825, 57.96, 13.97, 49.345, 32.945, 55.825, 25.595),
    (0.2, 0.05): (1.25, 29.7, 32.9, 40.2, 9.55, 30.0, 32.95, 39.9, 18.9),
    (0.2, 0.01): (1.24, 29.09, 31.25, 38.66, 9.34, 29.4, 31.29, 38.42, 18.14),
    (0.2, 0.005): (1.235, 29.015, 31.05, 38.475, 9.315, 29.32, 31.08, 38.235, 18.045),
    (0.1, 0.05): (1.25, 26.85, 33.3, 40.35, 8.4, 27.5, 33.85, 40.55, 18.95),
    (0.1, 0.01): (1.23, 25.64, 31.46, 38.08, 8.03, 26.24, 31.94, 38.21, 17.95),
    (0.1, 0.005): (1.225, 25.5, 31.26, 37.81, 7.99, 26.09, 31.72, 37.93, 17.835),
}
NIEDERER = {dt: dict(zip(_POINTS, NIEDERER_TABLE[(0.5, dt)])) for dt in (0.05, 0.01)}


def _niederer_activation_times(dx, dt, T=70.0):
    """demos/niederer_benchmark.py written against this package: activation time = start of the first step after
    which v > 0 at the probe point (the demo's own convention, :283-289)."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    Lx, Ly, Lz = 20.0, 7.0, 3.0
    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=Lx, Ly=Ly, Lz=Lz, dx=dx)
    mesh = geo.mesh
    cond = beat.conductivities.default_conductivities("Niederer")
    C_m = 1.0 * beat.units.ureg("uF/cm**2")
    time = g.Constant(mesh, 0.0)
    L, tol = 1.5, 1.0e-10
    cells = g.locate_entities(mesh, 3, lambda x: np.logical_and(np.logical_and(x[0] <= L + tol, x[1] <= L + tol), x[2] <= L + tol))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                           mesh_unit="mm", amplitude=50_000.0)
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s,
                               params={"petsc_options": {"ksp_type": "cg", "pc_type": "hypre"}},
                               C_m=C_m.to("uF/mm**2").magnitude, dx=I_s.dZ)
    ic = tp06.init_state_values(V=-85.23, Xr1=0.00621, Xr2=0.4712, Xs=0.0095, m=0.00172, h=0.7444, j=0.7045,
                                d=3.373e-05, f=0.7888, f2=0.9755, fCass=0.9953, s=0.999998, r=2.42e-08,
                                Ca_i=0.000126, R_prime=0.9073, Ca_SR=3.64, Ca_ss=0.00036, Na_i=8.604, K_i=136.89)
    ode = beat.odesolver.DolfinODESolver(
        v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
        init_states=ic, parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(ic),
        v_index=tp06.state_index("V"))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    points = {"P1": (0, 0, 0), "P2": (0.0, Ly, 0.0), "P3": (Lx, 0.0, 0.0), "P4": (Lx, Ly, 0.0), "P5": (0.0, 0.0, Lz),
              "P6": (0.0, Ly, Lz), "P7": (Lx, 0.0, Lz), "P8": (Lx, Ly, Lz), "P9": (Lx / 2, Ly / 2, Lz / 2)}
    plist = np.array(list(points.values()), dtype=float)
    at = {p: -1.0 for p in points}
    t = 0.0
    while t < T + 1e-12 and any(a < 0.0 for a in at.values()):
        solver.step((t, t + dt))
        vals = g.evaluate_function(solver.pde.state, plist).ravel()
        for p, value in zip(points, vals):
            if value > 0.0 and at[p] < 0.0:
                at[p] = t
        t += dt
    return at


@pytest.mark.parametrize("dt", [0.05, 0.01])
def test_niederer_activation_times(dt):
    """Niederer 2011 benchmark, dx = 0.5 mm: activation times (first t with v > 0) at P1..P9 against
    the table committed in the reference demo.  Gate: |delta| <= max(2 dt, 0.1 % of the tabulated time)
    -- the table was produced with CG + BoomerAMG at PETSc's default rtol 1e-5 and is printed to two
    decimals; here the linear systems are solved to 1e-10."""
    at = _niederer_activation_times(0.5, dt)
    for p, ref in NIEDERER[dt].items():
        assert abs(at[p] - ref) <= max(2 * dt, 1e-3 * ref) + 1e-9, (p, at[p], ref, at)


@pytest.mark.parametrize("dx,dt", [k for k in NIEDERER_TABLE if k not in ((0.5, 0.05), (0.5, 0.01))])
def test_niederer_table_all_resolutions(dx, dt):
    """The remaining seven rows of the reference's table (dx = 0.5 / 0.2 / 0.1 mm x dt = 0.05 / 0.01 / 0.005 ms,
    up to 442 k nodes and 11.6 k steps): every one of the 63 activation times within max(4 dt, 0.2 %) of the
    tabulated value (measured: all within 3 dt or 0.17 %; most within one step)."""
    at = _niederer_activation_times(dx, dt)
    for p, ref in zip(_POINTS, NIEDERER_TABLE[(dx, dt)]):
        assert abs(at[p] - ref) <= max(4 * dt, 2e-3 * ref) + 1e-9, (dx, dt, p, at[p], ref)


def test_readme_fitzhugh_nagumo_32x32_matches_oracle():
    """BASELINE config 1: the README script (README.md:40-199; 32x32 unit square, FHN forward Euler with
    11 parameters, M = 0.001, stimulus 600 on [0, 0.5]^2 for t in [0, 0.5], dt = 0.01) for 1000 steps:
    HIP path (PCG to rtol 1e-13) vs CPU oracle (sparse LU), difference <= 1e-10 relative to the 125 mV
    amplitude (all-fp64, no transcendental functions; what is left is the linear-solver tolerance
    accumulated over 1000 steps)."""
    import beat
    from beat import grid as g
    from oracle import fem, ionic

    mesh = g.create_unit_square(g.COMM_WORLD, 32, 32, g.CellType.triangle)
    time = g.Constant(mesh, g.default_scalar_type(0.0))
    a, b, c1, c2, c3, v_peak, v_rest = 0.13, 0.013, 0.26, 0.1, 1.0, 40.0, -85.0
    parameters = np.array([c1, c2, c3, a, b, v_peak - v_rest, v_rest, v_peak, 100.0, 1, 0.0], dtype=np.float64)
    init_states = np.array([0.0, -85], dtype=np.float64)
    parameters[-3] = 0.0
    stim_expr = g.conditional(g.And(g.ge(time, 0.0), g.le(time, 0.5)), 600.0, 0.0)
    cells = g.locate_entities(mesh, mesh.topology.dim, lambda x: np.logical_and(x[0] <= 0.5, x[1] <= 0.5))
    tags = g.meshtags(mesh, mesh.topology.dim, cells, np.full(len(cells), 1, dtype=np.int32))
    dx = g.Measure("dx", domain=mesh, subdomain_data=tags)
    I_s = beat.Stimulus(expr=stim_expr, dZ=dx, marker=1)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=0.001, I_s=I_s, dx=dx,
                               params={"petsc_options": {"ksp_rtol": 1e-13}})
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state,
                                         fun=beat.models.fhn.forward_euler_readme, init_states=init_states,
                                         parameters=parameters, num_states=2, v_index=1)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)

    om = fem.BoxMesh((32, 32), (1.0, 1.0))
    w = fem.stimulus_weights(om, om.locate_cells(lambda x: np.logical_and(x[0] <= 0.5, x[1] <= 0.5)))
    model = fem.OracleMonodomainModel(om, 0.001, [fem.OracleStimulus(fem.window(0.0, 0.5, 600.0), w)], theta=0.5)
    S = np.zeros((2, om.num_nodes))
    S.T[:] = init_states
    t, dt = 0.0, 0.01
    vmin, vmax = [], []
    for i in range(1000):
        solver.step((t, t + dt))
        S = ionic.fhn_readme_forward_euler(S, t, dt, parameters)
        model.state[:] = S[1]
        model.assign_previous()
        model.step((t, t + dt))
        S[1] = model.state
        t += dt
        if i % 100 == 0:
            v = solver.pde.state.x.array
            vmin.append(v.min())
            vmax.append(v.max())
    assert np.isfinite(vmin).all() and np.isfinite(vmax).all() and max(vmax) > -80.0
    assert np.abs(ode.values - S).max() <= 1e-10 * 125.0


def test_dg0_stimulus_function_updated_by_the_caller():
    """I_s given as a DG0 function that the caller re-interpolates from generate_random_activation every step
    (demos/ukb_atlas.py:327-356, 440-445): the PDE steps equal the oracle's with the same per-cell current,
    rhs_i = dt * sum_cells s_c |T|/(d+1) (sparse LU), to 1e-9."""
    import beat
    from beat import grid as g
    from oracle import fem

    cells, L = (12, 10, 8), (3.0, 2.5, 2.0)
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(L)], list(cells))
    time = g.Constant(mesh, 0.0)
    pts = np.array([[0.5, 0.5, 0.5], [2.5, 2.0, 1.5], [1.5, 1.25, 1.0]])
    delays = np.array([0.0, 0.1, 0.25])
    e = beat.stimulation.generate_random_activation(mesh, time, pts, delays, stim_start=0.0, stim_duration=0.2,
                                                    stim_amplitude=3.0, tol=0.4)
    stim = g.Function(g.functionspace(mesh, ("DG", 0)))
    M = np.diag([1e-3, 5e-4, 2e-4])
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=stim, C_m=0.01, params={"petsc_options": {"ksp_rtol": 1e-13}})
    omesh = fem.BoxMesh(cells, L)
    vol, _ = fem._cell_geometry(omesh)

    class CellStim:  # oracle stimulus with per-cell values re-evaluated at the model's time
        def __init__(self):
            self.weights = np.zeros(omesh.num_nodes)

        def amp(self, t):
            time.value = t
            vals = e.evaluate(g.cell_midpoints(mesh, mesh.all_cells()).T)
            w = np.zeros(omesh.num_nodes)
            np.add.at(w, omesh.cells.ravel(), np.repeat(vals * vol / 4.0, 4))
            self.weights = w
            return 1.0 if vals.any() else 0.0

    model = fem.OracleMonodomainModel(omesh, M, [CellStim()], C_m=0.01, theta=0.5)
    pde.state.x.array[:] = -80.0
    model.state[:] = -80.0
    dt = 0.05
    fired = 0
    for i in range(10):
        t0 = i * dt
        time.value = t0 + 0.5 * dt  # the caller evaluates the current at the time the PDE step uses
        stim.interpolate(e)
        fired += int(stim.x.array.any())
        pde.assign_previous()
        pde.step((t0, t0 + dt))
        model.assign_previous()
        model.step((t0, t0 + dt))
        assert np.abs(np.asarray(pde.state.x.array) - model.state).max() < 1e-9 * 80.0
    assert fired >= 6 and np.asarray(pde.state.x.array).max() > -79.0


def test_ecg_recovery():
    """beat.ECGRecovery: the reference's own test (tests/test_ecg.py:13-49: zero field -> zero lead, symmetry about
    x = 0.5, decay with distance) plus the numbers against the oracle: Im = -(1/C_m) Mass^-1 K v by sparse LU and
    the lead integral by quadrature of Im_h / (4 pi sigma_b |x - p|), to 1e-7 relative (PCG at 1e-8/1e-8... the
    recovery is run at rtol 1e-12 for this comparison)."""
    import scipy.sparse.linalg as spla

    import beat
    from beat import grid as g
    from oracle import fem

    N = 5
    mesh = g.create_unit_square(g.COMM_WORLD, N, N, g.CellType.triangle)
    V = g.functionspace(mesh, ("P", 1))
    v = g.Function(V)
    X = g.SpatialCoordinate(mesh)
    v_expr = (X[0] - 0.5) ** 2
    ecg = beat.ECGRecovery(v=v, M=1.0, C_m=1.0, sigma_b=1.0)
    p1, p2, p3 = (1.5, 0.5), (10.0, 0.5), (-0.5, 0.5)
    f1, f2, f3 = ecg.eval(p1), ecg.eval(p2), ecg.eval(p3)
    ecg.solve()
    assert np.isclose(beat.ecg.assemble_scalar(f1), 0.0)
    v.interpolate(g.Expression(v_expr, beat.utils.interpolation_points(V)))
    ecg.solve()
    v1, v2, v3 = (beat.ecg.assemble_scalar(f) for f in (f1, f2, f3))
    assert np.isclose(v1, v3) and abs(v2) < abs(v1) and abs(v1) > 1e-6

    # numbers: anisotropic tensor, C_m != 1, 3-D
    cells, L = (8, 6, 5), (2.0, 1.5, 1.0)
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(L)], list(cells))
    V = g.functionspace(mesh, ("P", 1))
    v = g.Function(V)
    v.interpolate(lambda x: -80.0 + 100.0 * np.exp(-((x[0] - 0.6) ** 2 + (x[1] - 0.5) ** 2 + (x[2] - 0.4) ** 2) / 0.2))
    M = np.array([[2.0e-3, 3.0e-4, 0.0], [3.0e-4, 1.0e-3, 0.0], [0.0, 0.0, 5.0e-4]])
    ecg = beat.ECGRecovery(v=v, M=M, C_m=0.01, sigma_b=2.0, petsc_options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    leads = {"a": (3.0, 0.5, 0.5), "b": (-1.0, 2.0, 1.5)}
    forms = {k: ecg.eval(p) for k, p in leads.items()}
    ecg.solve()
    omesh = fem.BoxMesh(cells, L)
    Mass, K = fem.assemble_mass(omesh), fem.assemble_stiffness(omesh, M)
    Im = spla.spsolve((-0.01 * Mass).tocsc(), K @ np.asarray(v.x.array))
    np.testing.assert_allclose(np.asarray(ecg.sol.x.array), Im, rtol=0, atol=1e-9 * np.abs(Im).max())
    for k, p in leads.items():
        w = fem.load_vector(omesh, lambda x, p=p: 1.0 / (4 * np.pi * 2.0) / np.sqrt(sum((x[a] - p[a]) ** 2 for a in range(3))))
        assert np.isclose(beat.ecg.assemble_scalar(forms[k]), w @ Im, rtol=1e-7)


def test_checkpoint_roundtrip(tmp_path):
    """beat.io: write_function / read_timestamps / read_function (the io4dolfinx calls of the demos)."""
    import beat
    from beat import grid as g

    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.ones(3)], [5, 4, 3])
    V = g.functionspace(mesh, ("P", 1))
    v = g.Function(V, name="v")
    fname = tmp_path / "chk.bp"
    beat.io.write_mesh(fname, mesh)
    snaps = {}
    for t in (0.0, 0.5, 1.0):
        v.interpolate(lambda x, t=t: np.sin(3 * x[0] + t) + x[1] * x[2])
        snaps[t] = np.asarray(v.x.array).copy()
        beat.io.write_function(fname, v, time=t, name="v")
    np.testing.assert_array_equal(beat.io.read_timestamps(comm=mesh.comm, filename=fname, function_name="v"), [0.0, 0.5, 1.0])
    w = g.Function(V)
    for t in (1.0, 0.0, 0.5):
        beat.io.read_function(fname, w, time=t, name="v")
        np.testing.assert_array_equal(np.asarray(w.x.array), snaps[t])
    with pytest.raises(KeyError):
        beat.io.read_function(fname, w, time=0.25, name="v")
    # a second run into the same path starts a NEW checkpoint (write_mesh opens in write mode): no time stamp or slab
    # of the first run survives, and a time stamp written twice within a run reads back the later write
    beat.io.write_mesh(fname, mesh)
    assert not list(fname.glob("*_r*.npy"))
    v.interpolate(lambda x: 7.0 + x[0])
    beat.io.write_function(fname, v, time=0.5, name="v")
    v.interpolate(lambda x: 9.0 - x[1])
    beat.io.write_function(fname, v, time=0.5, name="v")
    np.testing.assert_array_equal(beat.io.read_timestamps(comm=mesh.comm, filename=fname, function_name="v"), [0.5, 0.5])
    beat.io.read_function(fname, w, time=0.5, name="v")
    np.testing.assert_array_equal(np.asarray(w.x.array), np.asarray(v.x.array))
    with pytest.raises(KeyError):
        beat.io.read_function(fname, w, time=1.0, name="v")


def test_deferred_potential_update_is_bit_identical():
    """The fused split step leaves the last x += sum alpha_j p_j of the diffusion solve to the next ionic kernel
    (beat_ode_step_pending).  A run that never looks at the potential between steps (update always applied inside
    the kernel) equals, bit for bit, a run that reads it after every step (update always applied by the flush
    pass), and reading through any alias (pde.state, pde.v_, ode.v_ode, ode.values) sees the complete value."""
    runs = {}
    for peek in (False, True):
        s = _tp06_slab(True, nsteps=0)
        ops = s.pde._ops
        ops.set_small(False)  # (765 nodes: the one-launch solve would leave nothing to defer)
        deferred = 0
        for i in range(12):
            s.step((i * 0.05, (i + 1) * 0.05))
            deferred += int(ops.pending is not None or ops.open_x is not None)  # (left pending, or the solve still open: round 5)
            if peek:
                v = np.asarray(s.pde.state.x.array)
                assert ops.pending is None
                np.testing.assert_array_equal(v, np.asarray(s.ode.v_ode.x.array))
                np.testing.assert_array_equal(v, s.ode.values[17])
        assert deferred >= 10  # the solve does leave its update pending
        if not peek:
            # ... and the next ionic kernel consumes it: size queries on the aliased vectors (what _can_fuse asks at
            # every step) are not reads of the potential and must not cost a flush pass
            assert s.pde.state.x.array.size == s.ode.num_points == len(s.pde.v_.x.array)
            assert s.pde.state.x.array.shape == (s.ode.num_points,)
            assert ops.flushes == 0 and (ops.pending is not None or ops.open_x is not None)
        runs[peek] = s.ode.values.copy()
        assert ops.pending is None
        np.testing.assert_array_equal(np.asarray(s.pde.v_.x.array), runs[peek][17])
    np.testing.assert_array_equal(runs[False], runs[True])


@pytest.mark.parametrize("lazy", ["open", "pending"])
@pytest.mark.parametrize("why", ["another field", "not the model's potential row", "a node map into another field"])
def test_an_update_the_ionic_launch_may_not_claim_is_flushed_bit_identically(why, lazy, monkeypatch):
    """The three ways the claim of a deferred update (beat._deferred.DeferredUpdate.claim) can fail, each behind a solve that is
    still open and with the update pending (BEAT_LAZY_KSP=0): the ionic launch must leave the update alone -- the open solve is
    finished, the update applied in a pass of its own -- and 4 steps on a 17 x 9 x 7 box end on the bits of the same run with
    the update flushed after every solve.  "another field": two splitting solvers on ONE diffusion model take turns, so each
    finds the other's solve; "not the model's potential row": the PDE is coupled to another row of the states than TP06's V;
    "a node map into another field": a compact state array whose potential is at home in a field of its own.

    Why these: counted over the whole GPU suite, the claim met only an idle owner, a matching open solve (ring of six; ring of
    twelve with and without the class kernel) and a matching pending update -- no test reached a refusal for any of the three
    reasons, in either state.  No public route refuses today: the fused step always solves on the launch's own row.  So each case
    builds the nearest configuration that does.  Two solvers on one model meet each other's solve from the third step on (the
    second solver's first step has no operator yet and its solve flushes through the start of a solve); the node map is pointed at
    a field made here, through the private ``_dev.node_map``, which no public route does.  What they hold: a launch that took an
    update it must refuse would add one row's directions to another row or home, and the bits would differ from the flushed run;
    ``flushes`` tells a refused claim (a pass of its own) from a taken one (none)."""
    import beat
    from beat import grid as g
    from beat._engine import HipOps
    from beat.models import tp06

    monkeypatch.setattr(HipOps, "default_small", False)  # (1071 nodes: the one-launch solve would leave nothing to defer)
    monkeypatch.setenv("BEAT_LAZY_KSP", "1" if lazy == "open" else "0")
    monkeypatch.setenv("BEAT_MULTI_COMPACT", "1")
    row_v = tp06.state_index("V")

    def run(flush):
        mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([4.0, 2.0, 1.5])], [16, 8, 6])
        time = g.Constant(mesh, 0.0)
        cells = g.locate_entities(mesh, 3, lambda x: x[0] <= 1.0 + 1e-10)
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        chi = beat.conductivities.default_conductivities("Niederer")["chi"]
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=chi, time=time, subdomain_data=tags, marker=1, mesh_unit="mm",
                                               amplitude=50_000.0, duration=1.0)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([9.5e-4, 1.3e-4, 1.3e-4]), I_s=I_s, C_m=0.01, dx=I_s.dZ)
        V = g.functionspace(mesh, ("P", 1))
        assert pde.state.x.array.size == 17 * 9 * 7 and not pde._ops.small_active()

        def single(v_index):
            ode = beat.odesolver.DolfinODESolver(
                v_ode=g.Function(V), v_pde=pde.state, fun=tp06.generalized_rush_larsen, init_states=tp06.init_state_values(),
                parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=19, v_index=v_index)
            return beat.MonodomainSplittingSolver(pde=pde, ode=ode)

        if why == "another field":
            solvers = [single(row_v), single(row_v)]
        elif why == "not the model's potential row":
            solvers = [single((row_v + 1) % 19)]
        else:
            markers = g.Function(V)
            markers.x.array[:] = np.where(mesh.node_coordinates(pad3=True)[:, 0] < 2.0, 0.0, 1.0)
            v_ode = g.Function(V)
            v_ode.x.array[:] = -80.0
            ode = beat.odesolver.DolfinMultiODESolver(
                v_ode=v_ode, v_pde=pde.state, markers=markers, num_states={0: 19, 1: 19}, v_index={0: row_v, 1: row_v},
                fun={k: tp06.generalized_rush_larsen for k in (0, 1)}, init_states={k: tp06.init_state_values() for k in (0, 1)},
                parameters={0: tp06.init_parameter_values(stim_amplitude=0.0), 1: tp06.init_parameter_values(stim_amplitude=0.0, g_Ks=0.098)})
            assert ode._marked and ode._node_idx is not None
            home = pde._ctx.field(ode._v_row.n, mesh.plane)  # the potential the cells see lives here ...
            home.copy_from(ode._v_row)
            ode._dev.node_map = (ode._dev.node_map[0], home)  # ... while the diffusion solve works on ode._v_row
            solvers = [beat.MonodomainSplittingSolver(pde=pde, ode=ode)]
        assert all(s._can_fuse() for s in solvers)
        ops, left = pde._ops, 0
        for i in range(4):
            solvers[i % len(solvers)].step((i * 0.05, (i + 1) * 0.05))
            left += int(ops.open_x is not None if lazy == "open" else ops.pending is not None)
            if flush:
                ops.flush_pending()
        # the steps left their solves open / updates pending (a solve that ends on a full ring cycle with no guess increment due
        # leaves nothing): the state the claims under test meet
        assert left == 4 if lazy == "open" else left >= 2
        if not flush:  # ... and no launch took one: passes of their own applied them (the last step's may still be owed)
            assert 1 <= ops.flushes <= 3
        out = [np.asarray(pde.state.x.array).copy()]
        for s in solvers:
            ode = s.ode
            out.append(np.asarray(ode._v_row.numpy()).copy())
            out.append(np.asarray(ode._dev.states.numpy()).copy())
        assert ops.pending is None and ops.open_x is None
        return out

    a, b = run(False), run(True)
    assert np.abs(a[0] - a[0][0]).max() > 0.0  # (the stimulus acts: the potential is no constant)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_fused_multi_celltype_step_equals_reference_sequence(theta, monkeypatch):
    """DolfinMultiODESolver whose markers share one device model, four ways: (a) ONE state array with a class byte per
    node, one ionic launch per step (beat_ode_step_classes) and the single-model fused route -- in-place solve on the V
    row, the deferred potential update applied by the next ionic launch; (b) the same array driven through the literal
    reference sequence; (c) per-marker arrays (the reference's data layout, BEAT_MULTI_ONE_LAUNCH=0) through the fused
    multi route (potentials scattered into the PDE unknown, solved in place, gathered back); (d) per-marker arrays, literal
    sequence.  Bit-identical states everywhere; v_ / v_ode / state agree.  A strip of nodes carries a marker no model is
    defined for: it only diffuses (its potential still receives the deferred update)."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    out = []
    # (compact: the state array holds only the nodes of the tissue and reaches the potential through a node map -- what a
    # voxelised wall gets by itself; forced here on a full box, where the map is the identity)
    for one_launch, fused, compact in ((True, True, "0"), (True, True, "1"), (True, False, "0"), (True, False, "1"),
                                       (False, True, "0"), (False, False, "0")):
        monkeypatch.setenv("BEAT_MULTI_ONE_LAUNCH", "1" if one_launch else "0")
        monkeypatch.setenv("BEAT_MULTI_COMPACT", compact)
        mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([3.0, 2.0, 1.0])], [12, 8, 4])
        time = g.Constant(mesh, 0.0)
        cells = g.locate_entities(mesh, 3, lambda x: x[0] <= 0.75 + 1e-10)
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        chi = beat.conductivities.default_conductivities("Niederer")["chi"]
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=chi, time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, duration=1.0)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([9.5e-4, 1.3e-4, 1.3e-4]), I_s=I_s, C_m=0.01, dx=I_s.dZ)
        V = g.functionspace(mesh, ("P", 1))
        markers = g.Function(V)
        xs = mesh.node_coordinates(pad3=True)[:, 0]
        markers.x.array[:] = np.where(xs < 1.0, 0.0, np.where(xs < 2.0, 1.0, np.where(xs < 2.7, 2.0, 7.0)))
        v_ode = g.Function(V)
        v_ode.x.array[:] = -80.0  # what the strip without a model starts from
        keys = (0, 1, 2)
        params = {0: tp06.init_parameter_values(stim_amplitude=0.0), 1: tp06.init_parameter_values(stim_amplitude=0.0, g_Ks=0.098),
                  2: tp06.init_parameter_values(stim_amplitude=0.0, g_to=0.073)}
        ode = beat.odesolver.DolfinMultiODESolver(
            v_ode=v_ode, v_pde=pde.state, markers=markers, num_states={k: 19 for k in keys},
            fun={k: tp06.generalized_rush_larsen for k in keys}, init_states={k: tp06.init_state_values() for k in keys},
            parameters=params, v_index={k: tp06.state_index("V") for k in keys})
        assert ode._marked == one_launch and (not one_launch or (ode._node_idx is not None) == (compact == "1"))
        solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=theta, fused=fused)
        assert solver._can_fuse() == (fused and one_launch) and solver._can_fuse_multi() == fused
        for i in range(25):
            if i == 12:  # an edit of a live parameter array between steps reaches the kernels (odesolver.py:70-76)
                params[1][tp06.parameter_index("g_Kr")] *= 0.5
            solver.step((i * 0.05, (i + 1) * 0.05))
        if one_launch and fused:
            assert pde._ops.flushes == 0  # no separate pass ever applied the potential's update
        v = np.asarray(pde.state.x.array).copy()
        np.testing.assert_array_equal(v, np.asarray(pde.v_.x.array))
        np.testing.assert_array_equal(v, np.asarray(ode.v_ode.x.array))
        per_marker = {k: ode.values(k).copy() for k in keys}
        assert all(per_marker[k].shape == (19, int((np.asarray(markers.x.array) == k).sum())) for k in keys)
        out.append((v, ode.full_values.copy(), per_marker))
        assert v.max() > -60.0 and v[xs >= 2.7].max() < -60.0 and not np.array_equal(v[xs >= 2.7], np.full((xs >= 2.7).sum(), -80.0))
    for other in out[1:]:
        np.testing.assert_array_equal(out[0][0], other[0])
        np.testing.assert_array_equal(out[0][1], other[1])
        for k in (0, 1, 2):
            np.testing.assert_array_equal(out[0][2][k], other[2][k])


def test_piecewise_constant_per_node_parameters_run_as_classes():
    """(P, N) per-node parameters of which two rows are piecewise constant -- demos/pace_train.py:133-167: g_Kr and g_Ks
    zeroed in the right half of the cable -- are recognised as two uniform parameter sets and run through the class
    kernel (scalar-register parameters, no per-node rows loaded), as NumPy array and as resident DeviceParameters handle,
    with edits seen; the states equal those of the per-node kernel (BEAT_PARAM_CLASSES=0) to rounding of the per-launch
    constants and the oracle's to 1e-11.  A smoothly varying row is left to the per-node kernel."""
    import os

    import beat
    from beat import grid as g
    from beat.models import tp06
    from beat.odesolver import DeviceParameters
    from oracle import ionic

    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([4.0, 1.0, 1.0])], [32, 8, 8])
    V = g.functionspace(mesh, ("P", 1))
    n = V.dofmap.index_map.size_local
    xs = mesh.node_coordinates(pad3=True)[:, 0]
    P0 = tp06.init_parameter_values(stim_amplitude=0.0)
    P = np.zeros((len(P0), n))
    P.T[:] = P0
    for name in ("g_Kr", "g_Ks"):
        P[tp06.parameter_index(name)] = np.where(xs >= 2.0, 0.0, P0[tp06.parameter_index(name)])
    rng = np.random.default_rng(2)
    S0 = np.repeat(tp06.init_state_values()[:, None], n, axis=1)
    S0[tp06.state_index("V")] = rng.uniform(-90.0, 30.0, n)

    def run(parameters, steps=6, classes_env="1", sparse_env="1", jit_env="1"):
        os.environ["BEAT_PARAM_CLASSES"] = classes_env
        os.environ["BEAT_PARAM_SPARSE"] = sparse_env
        os.environ["BEAT_JIT"] = jit_env  # "0": the run-time-index kernel (same arithmetic as the all-rows kernel, bit for bit)
        try:
            ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=tp06.generalized_rush_larsen,
                                                 init_states=S0, parameters=parameters, num_states=19, v_index=tp06.state_index("V"))
            for i in range(steps):
                ode.step(0.02 * i, 0.02)
            return ode, np.asarray(ode.values).copy()
        finally:
            os.environ.pop("BEAT_PARAM_CLASSES", None)
            os.environ.pop("BEAT_PARAM_SPARSE", None)
            os.environ.pop("BEAT_JIT", None)

    ode_c, out_c = run(P)
    assert ode_c._dev.classes is not None and ode_c._dev.classes[2] == 2
    ode_h, out_h = run(DeviceParameters(P))
    assert ode_h._dev.classes is not None and ode_h._dev.classes[2] == 2
    ode_n, out_n = run(P, classes_env="0", sparse_env="0")
    assert ode_n._dev.classes is None and ode_n._dev._sparse is None
    np.testing.assert_array_equal(out_c, out_h)
    np.testing.assert_allclose(out_c, out_n, rtol=1e-13, atol=1e-300)
    ref = S0.copy()
    for i in range(6):
        ref = ionic.tp06_generalized_rush_larsen(ref, 0.02 * i, 0.02, P)
    err = np.abs(out_c - ref) / np.maximum(np.abs(ref), 1e-3)
    assert err.max() < 1e-10
    # an edit of the live array is seen: a third class appears
    P[tp06.parameter_index("g_to"), xs < 1.0] *= 0.3
    ode_c.step(0.12, 0.02)
    assert ode_c._dev.classes[2] == 3
    ref = ionic.tp06_generalized_rush_larsen(ref, 0.12, 0.02, P)
    err = np.abs(np.asarray(ode_c.values) - ref) / np.maximum(np.abs(ref), 1e-3)
    assert err.max() < 1e-10
    # a smooth field has as many distinct columns as nodes: per-node kernel
    Pg = np.repeat(P0[:, None], n, axis=1)
    Pg[tp06.parameter_index("g_Na")] *= np.linspace(0.8, 1.2, n)
    # ... but only ONE row of it varies: that row alone is kept on the device next to the uniform vector (round 4:
    # beat_ode_step_rows -- 8 B per node of parameter traffic instead of 424), same arithmetic as with all 53 rows
    Pg[tp06.parameter_index("g_CaL")] *= 1.0 + 0.2 * np.sin(3.0 * xs)
    ode_g, out_g = run(Pg, jit_env="0")
    assert ode_g._dev.classes is None and ode_g._dev._sparse is not None
    assert sorted(ode_g._dev._sparse[1].tolist()) == sorted([tp06.parameter_index("g_Na"), tp06.parameter_index("g_CaL")])
    ode_d, out_d = run(Pg, sparse_env="0")
    assert ode_d._dev._sparse is None
    np.testing.assert_array_equal(out_g, out_d)
    ode_h2, out_h2 = run(DeviceParameters(Pg), jit_env="0")
    assert ode_h2._dev._sparse is not None
    np.testing.assert_array_equal(out_h2, out_d)
    # the default route: the instance compiled for these two indices (csrc/beat_ode_jit.h) -- the constants the two
    # conductances do not enter come from the host there: last-bit differences
    ode_j, out_j = run(Pg)
    assert ode_j._dev._sparse is not None
    np.testing.assert_allclose(out_j, out_d, rtol=1e-12, atol=1e-300)
    ref = S0.copy()
    for i in range(6):
        ref = ionic.tp06_generalized_rush_larsen(ref, 0.02 * i, 0.02, Pg)
    assert (np.abs(out_g - ref) / np.maximum(np.abs(ref), 1e-3)).max() < 1e-10
    # an edit of the live array that makes a fifth row vary: without run-time compilation (the shipped kernel takes four rows)
    # back to all rows; with it (round 5: a compiled instance takes up to sixteen) the five rows stay the only ones on the device
    for k, name in enumerate(("g_Kr", "g_Ks", "g_to")):
        Pg[tp06.parameter_index(name)] *= 1.0 + 0.01 * (k + 1) * np.cos(xs)
    os.environ["BEAT_JIT"] = "0"
    try:
        ode_g.step(0.12, 0.02)
    finally:
        os.environ.pop("BEAT_JIT", None)
    assert ode_g._dev._sparse is None and ode_g._dev.classes is None
    ref = ionic.tp06_generalized_rush_larsen(ref, 0.12, 0.02, Pg)
    assert (np.abs(np.asarray(ode_g.values) - ref) / np.maximum(np.abs(ref), 1e-3)).max() < 1e-10
    Pg[tp06.parameter_index("g_to")] *= 1.0 + 1e-3 * np.sin(xs)  # (another edit: the route is looked at again)
    ode_g.step(0.14, 0.02)
    assert ode_g._dev._sparse is not None and len(ode_g._dev._sparse[1]) == 5 and ode_g._dev.classes is None
    ref = ionic.tp06_generalized_rush_larsen(ref, 0.14, 0.02, Pg)
    assert (np.abs(np.asarray(ode_g.values) - ref) / np.maximum(np.abs(ref), 1e-3)).max() < 1e-10


def test_one_solver_through_every_parameter_route_equals_fresh_solvers(monkeypatch):
    """One TP06 solver of 640 nodes (two and a half 256-node tiles) whose parameters change kind every two steps -- vector, two-column
    array (the class boundary inside a wavefront, at node 430), vector, the same array, an array with two smooth rows, a resident
    handle of it, ``set_row`` on the handle: after each pair of steps the states equal, bit for bit, those of a fresh solver started
    from the states before the pair with the same parameters (no route outlives the input it was derived from), and ``classes`` /
    ``_sparse`` read as tests/test_param_route_cpu.py says the kinds are.  BEAT_JIT=0: the shipped kernels, nothing is compiled."""
    import beat
    from beat import grid as g
    from beat.models import tp06
    from beat.odesolver import DeviceParameters

    monkeypatch.setenv("BEAT_JIT", "0")
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([3.9, 0.3, 0.3])], [39, 3, 3])
    V = g.functionspace(mesh, ("P", 1))
    n = V.dofmap.index_map.size_local
    assert n == 640
    vi, dt = tp06.state_index("V"), 0.02
    P0 = tp06.init_parameter_values(stim_amplitude=0.0)
    A = np.repeat(P0[:, None], n, axis=1)
    A[tp06.parameter_index("g_Kr"), 430:] = 0.0
    A[tp06.parameter_index("g_Ks"), 430:] *= 0.5
    G = np.repeat(P0[:, None], n, axis=1)
    G[tp06.parameter_index("g_Na")] *= np.linspace(0.8, 1.2, n)
    G[tp06.parameter_index("g_CaL")] *= 1.0 + 0.2 * np.sin(np.linspace(0.0, 3.0, n))
    two = sorted([tp06.parameter_index("g_Na"), tp06.parameter_index("g_CaL")])
    S0 = np.repeat(tp06.init_state_values()[:, None], n, axis=1)
    S0[vi] = np.random.default_rng(5).uniform(-90.0, 30.0, n)

    def solver(states, parameters):
        return beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=tp06.generalized_rush_larsen,
                                              init_states=states, parameters=parameters, num_states=19, v_index=vi)

    def kind(dev):
        return (None if dev.classes is None else dev.classes[2]), (None if dev._sparse is None else sorted(dev._sparse[1].tolist()))

    ode = solver(S0, P0)
    handle = DeviceParameters(G)

    def more_rows():
        handle.set_row(tp06.parameter_index("g_to"), P0[tp06.parameter_index("g_to")] * np.linspace(1.0, 0.7, n))
        return handle

    stages = [("vector", lambda: P0, (None, None)), ("two columns", lambda: A, (2, None)), ("vector again", lambda: P0.copy(), (None, None)),
              ("the same array", lambda: A, (2, None)), ("two smooth rows", lambda: G, (None, two)), ("handle", lambda: handle, (None, two)),
              ("set_row", more_rows, (None, sorted(two + [tp06.parameter_index("g_to")])))]
    for k, (what, parameters, want) in enumerate(stages):
        before = np.asarray(ode.values).copy()
        ode.parameters = parameters()
        for j in range(2):
            ode.step(dt * (2 * k + j), dt)
        assert kind(ode._dev) == want, what
        p = ode.parameters
        other = solver(before, p.numpy() if isinstance(p, DeviceParameters) else np.array(p))
        for j in range(2):
            other.step(dt * (2 * k + j), dt)
        assert kind(other._dev) == want, what
        got = np.asarray(ode.values)
        assert np.isfinite(got).all() and not np.array_equal(got, before)
        np.testing.assert_array_equal(got, np.asarray(other.values), err_msg=what)


def test_split_step_with_a_smooth_per_node_parameter_runs_on_sparse_rows():
    """A smooth gradient in one conductance over a slab, through the public API and the fused split step (the ionic kernel
    applies the previous solve's pending update): the sparse-rows route (one parameter row on the device) against all 53
    rows (BEAT_PARAM_SPARSE=0), bit for bit after 12 steps, for TP06 and for ToR-ORd-dynCl (the per-node route itself is held against
    the oracle by the tests above).  Reference: parameters per node, src/beat/odesolver.py:67-79, demos/pace_train.py:133-167."""
    import os

    import beat
    from beat import grid as g
    from beat.models import torord, tp06

    def run(model, vname, pname, sparse):
        os.environ["BEAT_PARAM_SPARSE"] = sparse
        os.environ["BEAT_JIT"] = "0"  # the run-time-index kernel: same arithmetic as the all-rows kernel (the compiled instance: next test)
        try:
            mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([2.0, 1.0, 0.6])], [20, 10, 6])
            V = g.functionspace(mesh, ("P", 1))
            n = V.dofmap.index_map.size_local
            xs = mesh.node_coordinates(pad3=True)
            P0 = model.init_parameter_values()
            P = np.repeat(P0[:, None], n, axis=1)
            P[model.parameter_index(pname)] *= 1.0 - 0.2 * xs[:, 0] - 0.1 * xs[:, 1] - 0.07 * xs[:, 2]  # distinct at every node
            time = g.Constant(mesh, 0.0)
            pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([1e-3, 3e-4, 3e-4]), C_m=0.01,
                                       params={"petsc_options": {"ksp_rtol": 1e-10}})
            S0 = np.repeat(model.init_state_values()[:, None], n, axis=1)
            S0[model.state_index(vname)] += 60.0 * np.exp(-((xs - np.array([0.4, 0.5, 0.3])) ** 2).sum(axis=1) / 0.05)
            ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=pde.state, fun=model.generalized_rush_larsen, init_states=S0,
                                                 parameters=P, num_states=S0.shape[0], v_index=model.state_index(vname))
            solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
            for k in range(12):
                solver.step((0.02 * k, 0.02 * (k + 1)))
            return np.asarray(ode.values).copy(), ode._dev._sparse is not None, (mesh, P, S0)
        finally:
            os.environ.pop("BEAT_PARAM_SPARSE", None)
            os.environ.pop("BEAT_JIT", None)

    for model, vname, pname in ((tp06, "V", "g_CaL"), (torord, "v", "GKr_b")):
        a, sparse_a, info = run(model, vname, pname, "1")
        b, sparse_b, _ = run(model, vname, pname, "0")
        assert sparse_a and not sparse_b
        np.testing.assert_array_equal(a, b)
        assert np.isfinite(a).all() and a[model.state_index(vname)].max() > -80.0  # (the bump is still there)



def test_sparse_rows_run_on_an_instance_compiled_for_their_indices():
    """The kernel instance with the varying parameter indices as compile-time constants, written and compiled by hipcc at first
    use (csrc/beat_ode_jit.h): through the public API's fused split step against the all-rows kernel -- same values to 1e-12 (the
    derived constants the varying parameter does not enter are the host's there and the device's here: last-bit differences) --
    for one smooth conductance (TP06, ToR-ORd), for two varying rows at once, and for a DISCRETE parameter pushed through the
    sparse route with the class analysis off (the cell type of ToR-ORd: derive() branches on it, so the numerically found
    dependency mask has to catch every constant it switches).  The library's counters say the instances were compiled and
    loaded, and a second solver with the same index set compiles nothing.  Reference: src/beat/odesolver.py:67-79."""
    import ctypes as C
    import os

    import beat
    from beat import _hip
    from beat import grid as g
    from beat.models import torord, torord_land, tp06

    lib = _hip.load()
    stats = (C.c_longlong * 4)()
    assert lib.beat_ode_jit_stats(stats) == 1, lib.beat_last_error().decode(errors="replace")  # (says what is missing)

    def run(model, vname, fields, route):
        env = {"rows": {"BEAT_PARAM_SPARSE": "0"}, "jit": {}}[route]
        env = dict(env, BEAT_PARAM_CLASSES="0")
        os.environ.update(env)
        try:
            mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([2.0, 1.0, 0.6])], [20, 10, 6])
            V = g.functionspace(mesh, ("P", 1))
            n = V.dofmap.index_map.size_local
            xs = mesh.node_coordinates(pad3=True)
            P = np.repeat(model.init_parameter_values()[:, None], n, axis=1)
            for pname, field in fields.items():
                P[model.parameter_index(pname)] = field(P[model.parameter_index(pname)], xs)
            time = g.Constant(mesh, 0.0)
            pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([1e-3, 3e-4, 3e-4]), C_m=0.01,
                                       params={"petsc_options": {"ksp_rtol": 1e-10}})
            S0 = np.repeat(model.init_state_values()[:, None], n, axis=1)
            S0[model.state_index(vname)] += 60.0 * np.exp(-((xs - np.array([0.4, 0.5, 0.3])) ** 2).sum(axis=1) / 0.05)
            ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=pde.state, fun=model.generalized_rush_larsen, init_states=S0,
                                                 parameters=P, num_states=S0.shape[0], v_index=model.state_index(vname))
            solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
            for k in range(12):
                solver.step((0.02 * k, 0.02 * (k + 1)))
            return np.asarray(ode.values).copy(), ode._dev._sparse is not None
        finally:
            for k in env:
                os.environ.pop(k, None)

    smooth = lambda p, xs: p * (1.0 - 0.2 * xs[:, 0] - 0.1 * xs[:, 1] - 0.07 * xs[:, 2])  # noqa: E731
    other = lambda p, xs: p * (0.7 + 0.25 * np.sin(3.0 * xs[:, 0]) * np.cos(2.0 * xs[:, 1]))  # noqa: E731
    layers = lambda p, xs: np.floor(3.0 * xs[:, 2] / 0.6001)  # noqa: E731  -- 0, 1, 2 through the wall
    # eight smooth rows (round 5: the compiled instance takes up to 16 indices; the shipped run-time-index kernel four)
    eight_tp06 = {nm: (smooth if k % 2 == 0 else other) for k, nm in enumerate(("g_CaL", "g_Kr", "g_Ks", "g_Na", "g_to", "g_K1", "g_bca", "g_pCa"))}
    eight_tor = {nm: (smooth if k % 2 == 0 else other) for k, nm in enumerate(("GKr_b", "GKs_b", "GNa", "Gto_b", "GK1_b", "PCa_b", "GNaL_b", "Gncx_b"))}
    cases = [(tp06, "V", {"g_CaL": smooth}), (torord, "v", {"GKr_b": smooth}), (tp06, "V", {"g_CaL": smooth, "g_Kr": other}),
             (torord, "v", {"celltype": layers, "GKs_b": other}), (torord_land, "v", {"Tref": smooth, "GKr_b": other}),
             (tp06, "V", eight_tp06), (torord, "v", eight_tor)]
    loaded_before = stats[0]
    for model, vname, fields in cases:
        a, sparse_a = run(model, vname, fields, "jit")
        b, sparse_b = run(model, vname, fields, "rows")
        assert sparse_a and not sparse_b
        scale = np.maximum(np.abs(b), 1e-9 * np.abs(b).max(axis=1, keepdims=True) + 1e-300)
        assert (np.abs(a - b) / scale).max() < 1e-10, (sorted(fields), (np.abs(a - b) / scale).max())
        assert np.isfinite(a).all()
    assert lib.beat_ode_jit_stats(stats) == 1
    loaded, compiled, from_disk, failures = (int(v) for v in stats)
    # every case steps the plain kernel once (the first ionic step has no pending update) and the pending-update form after
    # (counted over the process: another test may have loaded some of these instances before)
    assert failures == 0 and loaded >= max(len(cases), loaded_before) and compiled + from_disk >= loaded
    run(tp06, "V", {"g_CaL": smooth}, "jit")
    lib.beat_ode_jit_stats(stats)
    assert int(stats[0]) == loaded and int(stats[3]) == 0  # same index set: nothing new compiled or loaded


def test_sparse_rows_without_a_compiler_run_on_the_run_time_index_kernel(tmp_path):
    """BEAT_HIPCC pointing nowhere (a machine with the library but no hipcc): the step on sparse rows runs on the shipped
    run-time-index kernel -- the all-rows kernel's bits --, the failure is counted (beat_ode_jit_stats) and reported once on stderr;
    nothing falls back to the host (tests/_jit_fallback_script.py, its own process: the compiler is looked up once per process)."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, BEAT_HIPCC=str(tmp_path / "no-such-hipcc"), BEAT_JIT_CACHE=str(tmp_path / "cache"))
    env.pop("BEAT_JIT", None)
    run = subprocess.run([sys.executable, str(root / "tests" / "_jit_fallback_script.py")], capture_output=True, text=True, timeout=300,
                         cwd=root, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "jit-fallback ok" in run.stdout
    assert run.stderr.count("run-time compilation unavailable") == 1 and "using the run-time-index kernel" in run.stderr


def test_three_processes_compile_the_same_instance_into_one_cache_directory(tmp_path):
    """What the ranks of a decomposed run do at their first step with per-node parameters: three processes, one empty cache directory,
    the same kernel instance wanted by all at once (tests/_jit_race_script.py).  Each compiles under a name of its own and renames the
    object into place -- or finds the one another process put there -- and every one ends with a loaded instance, no failure, and the
    all-rows kernel's values; the directory holds one code object afterwards and no leftovers."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    cache = tmp_path / "cache"
    env = dict(os.environ, BEAT_JIT_CACHE=str(cache))
    for k in ("BEAT_JIT", "BEAT_PARAM_SPARSE", "BEAT_PARAM_CLASSES"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, str(root / "tests" / "_jit_race_script.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=root, env=env) for _ in range(3)]
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, so[-1500:] + se[-3000:]
        assert "jit-race ok" in so
    files = sorted(f.name for f in cache.iterdir())
    assert sum(f.endswith(".hsaco") for f in files) == 1 and not any(f.endswith((".tmp", ".hip")) for f in files), files


def test_parameter_route_follows_the_parameters_through_every_change_of_kind():
    """(round-3 review) The route a step takes -- uniform vector, per-node rows, parameter classes -- is re-derived whenever
    the KIND of ``parameters`` changes: a classified (P, N) array, then a vector, then the SAME array again must classify
    again (the vector branch cleared the classes, a cached "use the classes" must not survive it), likewise for a resident
    DeviceParameters handle of one version, and for NumPy array <-> handle in either order.  Every step is checked against
    the oracle with the parameters that were current; a mirror row other than the potential sends class-routed parameters
    back to the per-node kernel; the library refuses a launch without any parameters."""
    import ctypes as C

    import beat
    from beat import _hip
    from beat import grid as g
    from beat.models import tp06
    from beat.odesolver import DeviceParameters
    from oracle import ionic

    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([4.0, 1.0, 1.0])], [16, 4, 4])
    V = g.functionspace(mesh, ("P", 1))
    n = V.dofmap.index_map.size_local
    xs = mesh.node_coordinates(pad3=True)[:, 0]
    P0 = tp06.init_parameter_values(stim_amplitude=0.0)
    Pn = np.zeros((len(P0), n))
    Pn.T[:] = P0
    Pn[tp06.parameter_index("g_Kr")] = np.where(xs >= 2.0, 0.0, P0[tp06.parameter_index("g_Kr")])
    Pv = tp06.init_parameter_values(stim_amplitude=0.0, g_Na=9.0)
    handle = DeviceParameters(Pn)
    rng = np.random.default_rng(8)
    S0 = np.repeat(tp06.init_state_values()[:, None], n, axis=1)
    S0[tp06.state_index("V")] = rng.uniform(-90.0, 30.0, n)
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=tp06.generalized_rush_larsen,
                                         init_states=S0, parameters=Pn, num_states=19, v_index=tp06.state_index("V"))
    ref, t, dt = S0.copy(), 0.0, 0.02
    sequence = [("rows", Pn, 2), ("vector", Pv, None), ("rows", Pn, 2), ("handle", handle, 2), ("vector", Pv, None),
                ("handle", handle, 2), ("rows", Pn, 2), ("handle", handle, 2), ("vector", Pv, None), ("rows", Pn, 2)]
    for kind, prm, ncls in sequence:
        ode.parameters = prm
        ode.step(t, dt)
        ref = ionic.tp06_generalized_rush_larsen(ref, t, dt, Pv if kind == "vector" else Pn)
        t += dt
        cls = ode._dev.classes
        assert (cls is None) if ncls is None else (cls is not None and cls[2] == ncls), (kind, cls)
        err = np.abs(np.asarray(ode.values) - ref) / np.maximum(np.abs(ref), 1e-3)
        assert err.max() < 1e-10, (kind, err.max())
    # a mirror of another row than the potential: the class kernel does not write it, the per-node kernel does
    dev = ode._dev
    mirror = dev.ctx.zeros(n)

    class _Row:
        ptr = C.c_void_p(mirror.data_ptr())

    k = 3  # the m gate
    dev.parameters = Pn
    dev.step(t, dt, v_index=k, v_copy=_Row)
    ref = ionic.tp06_generalized_rush_larsen(ref, t, dt, Pn)
    dev.ctx.synchronize()
    np.testing.assert_allclose(mirror.cpu().numpy(), ref[k], rtol=1e-10)
    np.testing.assert_array_equal(mirror.cpu().numpy(), np.asarray(ode.values)[k])
    # no parameters at all for a model that has 53: refused, not run with every parameter at 1.0
    rc = dev.ctx.lib.beat_ode_step(dev.ctx.handle, _hip.MODEL_TP06_GRL1, dev.states.ptr, n, dev.states.ld, None, 53, None, 0,
                                   0.0, dt, tp06.state_index("V"), None)
    assert rc != 0 and b"no parameters" in dev.ctx.lib.beat_last_error()


@pytest.mark.parametrize("dim,theta_split,theta_pde", [(2, 1.0, 0.5), (2, 0.5, 1.0), (3, 1.0, 1.0), (3, 0.5, 0.5), (3, 1.0, 0.75)])
def test_fused_route_equals_literal_route_over_options(dim, theta_split, theta_pde):
    """Fused vs literal stepping (the reference's sequence of copies) over what the other tests hold fixed: 2-D and 3-D
    meshes, backward-Euler / Crank-Nicolson / theta = 0.75 diffusion, Godunov and Strang splitting, and a time step
    that changes twice during the run (base_model.py:225-230: matrices are rebuilt when dt changes) with a stimulus that
    switches off in between.  Same values to 1e-12."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    def run(fused):
        if dim == 3:
            geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=3.0, Ly=2.0, Lz=1.0, dx=0.25)
        else:
            geo = beat.geometry.get_2D_slab_geometry(comm=g.COMM_WORLD, Lx=4.0, Ly=3.0, dx=0.25)
        mesh = geo.mesh
        time = g.Constant(mesh, 0.0)
        cond = beat.conductivities.default_conductivities("Niederer")
        cells = g.locate_entities(mesh, dim, lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
        tags = g.meshtags(mesh, dim, cells, np.full(len(cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, start=0.0, duration=1.0)
        M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01, dx=I_s.dZ,
                                   params={"theta": theta_pde, "petsc_options": {"ksp_rtol": 1e-12}})
        ode = beat.odesolver.DolfinODESolver(
            v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
            init_states=tp06.init_state_values(), parameters=tp06.init_parameter_values(stim_amplitude=0.0),
            num_states=19, v_index=tp06.state_index("V"))
        solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=theta_split, fused=fused)
        t = 0.0
        for dt, n in ((0.05, 12), (0.02, 15), (0.1, 8)):  # stimulus ends at 1 ms, inside the second block
            for _ in range(n):
                solver.step((t, t + dt))
                t += dt
        return solver

    a, b = run(True), run(False)
    va, vb = np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array)
    assert va.max() > 0.0 and np.isfinite(va).all()
    np.testing.assert_allclose(va, vb, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a.ode.values, b.ode.values, rtol=1e-12, atol=1e-14)


# ---- per-node parameters: in-place edits by the caller must reach the kernel (demos/pace_train.py:133-167) -------
def test_per_node_parameter_edits_are_seen_and_device_handle():
    """The reference hands the live ``parameters`` array to ``fun`` every step.  A (P, N) NumPy array edited in place
    between steps -- here a pacing patch MOVED to another site of equal size, which keeps the array's sum and absolute
    sum -- must be picked up; a resident ``DeviceParameters`` handle gives the same values with nothing checked or
    moved per step, and changes through ``set_row``."""
    from beat import grid as g
    from beat.models import tp06
    from beat.odesolver import DeviceParameters, DolfinODESolver
    from oracle import ionic

    mesh = g.create_unit_square(g.COMM_WORLD, 9, 9)
    V = g.functionspace(mesh, ("P", 1))
    n = 100
    ic = tp06.init_state_values()
    ia = tp06.parameter_index("stim_amplitude")
    base = tp06.init_parameter_values(stim_start=0.0, stim_duration=5.0, stim_amplitude=0.0)
    P = np.repeat(base[:, None], n, axis=1)
    P[ia, :10] = -52.0
    dt = 0.05

    def solver(params):
        return DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=tp06.generalized_rush_larsen, init_states=ic,
                               parameters=params, num_states=len(ic), v_index=tp06.state_index("V"))

    ode = solver(P)
    ref = np.repeat(ionic.tp06_init_state_values()[:, None], n, axis=1)
    Pr = P.copy()
    for i in range(4):
        if i == 2:  # move the patch: same sum, same absolute sum, different nodes
            P[ia, :10] = 0.0
            P[ia, 50:60] = -52.0
            Pr = P.copy()
        ode.step(i * dt, dt)
        ref = ionic.tp06_generalized_rush_larsen(ref, i * dt, dt, Pr)
    out = ode.values
    err = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-3)
    assert err.max() < 1e-10, err.max()
    vi = tp06.state_index("V")
    assert out[vi, 55] > out[vi, 80] + 1.0 and out[vi, 5] > out[vi, 80] + 1.0  # both sites were paced, in turn

    P0 = np.repeat(base[:, None], n, axis=1)
    P0[ia, :10] = -52.0
    handle = DeviceParameters(P0)
    assert handle.shape == (53, n) and len(handle) == 53 and handle.version == 1
    ode2 = solver(handle)
    for i in range(4):
        if i == 2:
            row = np.zeros(n)
            row[50:60] = -52.0
            handle.set_row(ia, row)
            assert handle.version == 2
        ode2.step(i * dt, dt)
    np.testing.assert_array_equal(ode2.values, out)
    np.testing.assert_array_equal(handle.numpy(), P)


def test_field_extrema_propagate_nan():
    """``v.min()`` / ``v.max()`` of a device function (beat_field_minmax) behave as numpy's on a blown-up state: one
    NaN node, or an all-NaN field, gives NaN for both; infinities are ordinary values."""
    from beat._device import Context

    ctx = Context.default()
    n = 70_001
    f = ctx.field(n, 0)
    vals = np.linspace(-3.0, 5.0, n)
    f.set(vals)
    assert f.minmax() == (-3.0, 5.0)
    for bad in (0, 12_345, n - 1):
        v = vals.copy()
        v[bad] = np.nan
        f.set(v)
        lo, hi = f.minmax()
        assert np.isnan(lo) and np.isnan(hi), (bad, lo, hi)
    f.set(np.full(n, np.nan))
    lo, hi = f.minmax()
    assert np.isnan(lo) and np.isnan(hi)
    v = vals.copy()
    v[7] = np.inf
    v[9] = -np.inf
    f.set(v)
    assert f.minmax() == (-np.inf, np.inf)


def test_pde_solve_reports_non_convergence_as_status():
    """base_model.py:23-30: ``solve`` returns Results(state, status); a linear solve that runs out of iterations gives
    Status.NOT_CONVERGING and a negative ``getConvergedReason()`` seen by the monitor (telemetry.py:67-76) instead of
    an exception; ``ksp_error_if_not_converged`` raises, as PETSc's option of that name."""
    import beat
    from beat import grid as g
    from beat.base_model import Status
    from beat.telemetry import PerformanceMonitor

    mesh = g.create_unit_square(g.COMM_WORLD, 24, 24)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    stim = g.cos(2 * g.pi * x[0]) * g.cos(3 * g.pi * x[1])
    mon = PerformanceMonitor()
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=1.0, I_s=stim, monitor=mon,
                               params={"petsc_options": {"ksp_rtol": 1e-14, "ksp_max_it": 2}})
    res = pde.solve((0.0, 0.3), dt=0.1)
    assert res.status == Status.NOT_CONVERGING and pde.ksp.getConvergedReason() < 0
    assert mon.ksp_last_converged_reason < 0 and mon.ksp_last_iterations == 2
    assert np.isfinite(np.asarray(res.state.x.array)).all()
    ok = beat.MonodomainModel(time=time, mesh=mesh, M=1.0, I_s=stim, params={"petsc_options": {"ksp_rtol": 1e-10}})
    assert ok.solve((0.0, 0.3), dt=0.1).status == Status.OK
    strict = beat.MonodomainModel(time=time, mesh=mesh, M=1.0, I_s=stim,
                                  params={"petsc_options": {"ksp_rtol": 1e-14, "ksp_max_it": 2, "ksp_error_if_not_converged": True}})
    with pytest.raises(RuntimeError, match="did not converge"):
        strict.step((0.0, 0.1))


@pytest.mark.parametrize("order", [3, "auto"])
def test_batched_solve_equals_the_step_loop(order):
    """MonodomainSplittingSolver.solve on a grid small enough for the one-launch diffusion solve hands its steps to the
    library in one call (beat_split_steps: no host round trip between steps).  Same kernels in the same order as the
    step() loop: with a fixed guess order the states are identical bit for bit, the recorded probe values are the
    values evaluate_function returns after each step, the last KSP record is the last step's; with the adaptive order
    (frozen through a batch) the trajectories agree to the solver tolerance.  A monitor or a non-uniform parameter set
    keeps solve() on the step loop."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    pts = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.5], [4.0, 2.0, 1.0]])

    def build(monitor=None):
        geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=4.0, Ly=2.0, Lz=1.0, dx=0.25)
        mesh = geo.mesh
        time = g.Constant(mesh, 0.0)
        cond = beat.conductivities.default_conductivities("Niederer")
        cells = g.locate_entities(mesh, 3, lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, duration=1.0)
        M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
        C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ,
                                   params={"petsc_options": {"ksp_type": "cg", "ksp_rtol": 1e-10, "ksp_guess_order": order}})
        ode = beat.odesolver.DolfinODESolver(
            v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
            init_states=tp06.init_state_values(), parameters=tp06.init_parameter_values(stim_amplitude=0.0),
            num_states=19, v_index=tp06.state_index("V"))
        kw = {} if monitor is None else {"monitor": monitor}
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode, **kw)

    dt, nsteps = 0.05, 45  # the stimulus switches off at t = 1 ms, inside the run
    a = build()
    assert a._can_batch(None)
    rec = g.ProbeRecorder(a.pde.state, pts, capacity=32)  # smaller than the run: the record spills to the host once
    a.solve((0.0, nsteps * dt), dt, recorder=rec)
    b = build()
    vals, t0 = [], 0.0
    for i in range(nsteps):  # the intervals solve() generates (t1 = t0 + dt, accumulated)
        b.step((t0, t0 + dt))
        t0 = t0 + dt
        vals.append(g.evaluate_function(b.pde.state, pts).ravel())
    assert b.ode.values[17].max() > 0.0
    if order == 3:
        np.testing.assert_array_equal(a.ode.values, b.ode.values)
        np.testing.assert_array_equal(rec.values(), np.array(vals))
        assert a.pde.ksp.iterations == b.pde.ksp.iterations and a.pde.ksp.converged_reason > 0
    else:
        # (different guess orders leave different rtol-sized errors, which the upstroke amplifies)
        np.testing.assert_allclose(a.ode.values, b.ode.values, rtol=2e-6, atol=1e-8)
        np.testing.assert_allclose(rec.values(), np.array(vals), rtol=0, atol=1e-5)
    assert len(rec) == nsteps
    np.testing.assert_array_equal(np.asarray(a.pde.state.x.array), a.ode.values[17])
    np.testing.assert_array_equal(np.asarray(a.pde.v_.x.array), a.ode.values[17])
    # a second call continues where the first one ended (the step loop too)
    a.solve((t0, t0 + 5 * dt), dt)
    for i in range(5):
        b.step((t0, t0 + dt))
        t0 = t0 + dt
    if order == 3:
        np.testing.assert_array_equal(a.ode.values, b.ode.values)
    # with a monitor attached the caller wants per-step records: no batching
    assert not build(beat.telemetry.PerformanceMonitor())._can_batch(None)


@pytest.mark.parametrize("order", [2, "auto"])
def test_batched_solve_of_a_big_grid_equals_the_step_loop(order, monkeypatch):
    """A grid too big for the one-launch solve (28 611 nodes): MonodomainSplittingSolver.solve hands its steps to the library's own
    loop (beat_split_steps_big: per step the ionic launch that applies what the previous solve deferred, and the solve in place)
    -- what step() does without Python between the steps.  Same kernels, same arguments: the states after 40 steps, a second call
    that continues, the potential seen through pde.state (the deferred update applied on access) and the last KSP record are
    those of the step() loop BIT FOR BIT, with a fixed guess order and with the adaptive one (chosen per solve in both); the
    durations of the ionic launches are handed out on request; BEAT_BATCH_BIG=0, a probe recorder or a monitor keep the step loop."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    def build(monitor=None):
        geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=8.0, Ly=4.0, Lz=2.0, dx=0.2)
        mesh = geo.mesh
        time = g.Constant(mesh, 0.0)
        cond = beat.conductivities.default_conductivities("Niederer")
        cells = g.locate_entities(mesh, 3, lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, duration=1.0)
        M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
        C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ,
                                   params={"petsc_options": {"ksp_type": "cg", "ksp_rtol": 1e-10, "ksp_guess_order": order}})
        ode = beat.odesolver.DolfinODESolver(
            v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
            init_states=tp06.init_state_values(), parameters=tp06.init_parameter_values(stim_amplitude=0.0),
            num_states=19, v_index=tp06.state_index("V"))
        kw = {} if monitor is None else {"monitor": monitor}
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode, **kw)

    dt, nsteps = 0.05, 40  # the stimulus switches off at t = 1 ms, inside the run
    a = build()
    assert a.pde.state.x.array.size > 8192 and not a.pde._ops.small_active() and a._can_batch(None)
    a.batch_ode_ms = []
    a.solve((0.0, nsteps * dt), dt)
    assert len(a.batch_ode_ms) == nsteps and all(ms > 0.0 for ms in a.batch_ode_ms)
    b = build()
    t0 = 0.0
    for i in range(nsteps):
        b.step((t0, t0 + dt))
        t0 = t0 + dt
    assert b.ode.values[17].max() > 0.0
    np.testing.assert_array_equal(np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array))  # (applies the deferred update)
    np.testing.assert_array_equal(a.ode.values, b.ode.values)
    assert a.pde.ksp.iterations == b.pde.ksp.iterations and a.pde.ksp.converged_reason > 0
    a.solve((t0, t0 + 7 * dt), dt)  # continues: the update the last solve deferred is applied by the batch's first ionic launch
    for i in range(7):
        b.step((t0, t0 + dt))
        t0 = t0 + dt
    np.testing.assert_array_equal(a.ode.values, b.ode.values)
    b.step((t0, t0 + dt))  # and a step() after a batch
    a.step((t0, t0 + dt))
    np.testing.assert_array_equal(a.ode.values, b.ode.values)
    # solve() after step() / solve() WITHOUT a read in between (a driver that calls solve() per output interval): what the last
    # solve deferred -- here the solve step() left open -- is handed to the library loop's first ionic launch (pending_in), not
    # flushed in a pass of its own; twice in a row; same bits as the step() loop
    t0 = t0 + dt
    ops = a.pde._ops
    for span in (5, 3):
        a.step((t0, t0 + dt))
        b.step((t0, t0 + dt))
        t0 = t0 + dt
        assert ops.open_x is not None
        flushes, real_flush = [], ops.flush_pending
        ops.flush_pending = lambda: (flushes.append(1) if (ops.pending is not None or ops.open_x is not None) else None, real_flush())[1]  # (a call with nothing pending does nothing)
        try:
            a.solve((t0, t0 + span * dt), dt)
            a.solve((t0 + span * dt, t0 + 2 * span * dt), dt)
        finally:
            del ops.flush_pending
        assert not flushes
        for i in range(2 * span):
            b.step((t0, t0 + dt))
            t0 = t0 + dt
        np.testing.assert_array_equal(a.ode.values, b.ode.values)
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.5]])
    assert not a._can_batch(g.ProbeRecorder(a.pde.state, pts, capacity=8))
    assert not build(beat.telemetry.PerformanceMonitor())._can_batch(None)
    monkeypatch.setenv("BEAT_BATCH_BIG", "0")
    assert not a._can_batch(None)


@pytest.mark.parametrize("case", ["slab", "shell"])
def test_step_leaves_its_solve_open_and_the_next_ionic_launch_goes_behind_it(case, monkeypatch):
    """Round 5: ``MonodomainSplittingSolver.step`` does not wait for its diffusion solve (beat_pde_solve_begin); the next step's
    ionic launch is enqueued behind the open solve, reads what is pending from the solve's state on the device, does nothing if the
    solve has not latched -- the host then enqueues the missing iterations and launches again (beat_ode_step_* with pending = -1).
    Values, KSP records and status are those of the waiting step (BEAT_LAZY_KSP=0) BIT FOR BIT: on a TP06 slab whose iteration
    counts jump by more than the one iteration enqueued on spec when the stimulated corner fires (the relaunch path) and on a
    voxel shell with per-node rows, two parameter classes and the ring of 12 (the class kernel behind the solve);
    ``pde.ksp`` and ``pde.state.x.array`` finish an open solve on access.  (The two cases are those of bench.py's multi-rank
    parity block, bench_parity.py, on one rank, with this test's own step loop.)"""
    import sys
    from pathlib import Path

    from beat import grid as g

    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import bench_parity

    nsteps = 30

    def run(lazy, touch):
        monkeypatch.setenv("BEAT_LAZY_KSP", "1" if lazy else "0")
        out = {}

        def loop(solver, pde, steps, dt):
            extra, opens, t, log = [], 0, 0.0, []
            pde._ops.ksp_log = log
            for i in range(nsteps):
                solver.step((t, t + dt))
                opens += int(pde._ops.open_x is not None)
                if touch and i == 11:
                    extra.append(("ksp", pde.ksp.iterations))  # finishes the open solve
                    assert pde._ops.open_x is None
                if touch and i == 17:
                    extra.append(("v", float(np.asarray(pde.state.x.array).max())))  # flushes (and finishes) on access
                t += dt
            v = np.asarray(pde.state.x.array, dtype=np.float64).copy()
            out.update(v=v, opens=opens, its=[r.iterations for r in log], reasons=[r.converged_reason for r in log], extra=extra,
                       last=pde.ksp.iterations, status=pde.status)
            return v, out["its"]

        monkeypatch.setattr(bench_parity, "_run", loop)
        if case == "slab":
            bench_parity.slab_case(g.COMM_SELF, 24, nxy=48)
        else:
            bench_parity.shell_case(g.COMM_SELF, 32, n_xy=48)
        return out

    a = run(False, False)
    b = run(True, False)
    c = run(True, True)
    assert a["opens"] == 0 and b["opens"] == nsteps and c["opens"] == nsteps
    assert len(a["its"]) == nsteps and a["its"] == b["its"] == c["its"] and all(r > 0 for r in b["reasons"])
    # (the relaunch path is taken: the first solve needs more than the 8 iterations enqueued for a solve without a predecessor,
    # or some solve needs two more than the one before it -- the speculative chunk is the previous count + 1)
    assert a["its"][0] >= 9 or max(j - i for i, j in zip(a["its"][:-1], a["its"][1:])) >= 2
    np.testing.assert_array_equal(b["v"], a["v"])
    np.testing.assert_array_equal(c["v"], a["v"])
    assert b["last"] == a["last"] and c["extra"][0] == ("ksp", a["its"][11]) and a["status"] == b["status"]


@pytest.mark.parametrize("max_it", [0, 2])
def test_open_solve_that_may_not_iterate_still_takes_its_ionic_steps_and_reports_the_last_step(max_it, monkeypatch):
    """ADVICE round 5, two findings on the open solve.  (1) ``ksp_max_it = 0``: pcg_begin does not latch and no iteration is
    enqueued, so the ionic launch behind the solve saw an unlatched solve and did nothing -- and beat_solve_end, whose loop is
    skipped with nothing left to enqueue, used to report "no more iterations were needed": every ionic step after the first was
    silently dropped.  Now the first look at the latch decides, and the step is launched again with the host's count.  With
    x0 = v_ (guess order 0) and no iteration the diffusion changes nothing, so n steps must equal n steps of the cell model alone,
    bit for bit; with ``ksp_max_it = 2`` and an unreachable tolerance the values must be the waiting loop's.  (2) ``pde.status``
    of the LAST step: it is a property that finishes the open solve, as ``pde.ksp`` is."""
    import beat
    from beat import grid as g
    from beat.base_model import Status
    from beat.models import tp06

    def build(lazy):
        monkeypatch.setenv("BEAT_LAZY_KSP", "1" if lazy else "0")
        geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=8.0, Ly=4.0, Lz=2.0, dx=0.2)  # 9 471 nodes: not the one-launch solve
        mesh = geo.mesh
        time = g.Constant(mesh, 0.0)
        cond = beat.conductivities.default_conductivities("Niederer")
        M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, C_m=0.01,
                                   params={"petsc_options": {"ksp_rtol": 1e-14, "ksp_max_it": max_it, "ksp_guess_order": 0}})
        ic = tp06.init_state_values()
        init = np.repeat(ic[:, None], pde.state.x.array.shape[0], axis=1)
        x = mesh.geometry.x
        init[tp06.state_index("V")] += 60.0 * np.exp(-((x[:, 0] - 4.0) ** 2 + (x[:, 1] - 2.0) ** 2) / 2.0)  # something to diffuse
        ode = beat.odesolver.DolfinODESolver(
            v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
            init_states=init, parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=19, v_index=tp06.state_index("V"))
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode), init

    dt, nsteps = 0.05, 6
    a, init = build(True)
    opens = 0
    for i in range(nsteps):
        a.step((i * dt, (i + 1) * dt))
        opens += int(a.pde._ops.open_x is not None)
    assert opens == nsteps  # every solve was left open: the path under test
    assert a.pde.status == Status.NOT_CONVERGING  # (read BEFORE anything else finishes the last solve)
    assert a.pde._ops.open_x is None and a.pde.ksp.converged_reason < 0 and a.pde.ksp.iterations == max_it
    b, _ = build(False)
    for i in range(nsteps):
        b.step((i * dt, (i + 1) * dt))
    assert b.pde.status == Status.NOT_CONVERGING
    np.testing.assert_array_equal(a.ode.values, b.ode.values)
    if max_it == 0:  # no iteration from x0 = v_: the cell model alone
        y = init.copy()
        p = tp06.init_parameter_values(stim_amplitude=0.0)
        for i in range(nsteps):
            y = tp06.generalized_rush_larsen(states=y, t=i * dt, parameters=p, dt=dt)
        # (the fused step and the model's __call__ are two instances of one kernel template; with the step's fma contraction they
        # may differ in the last bit -- a dropped step differs by 1e-3)
        np.testing.assert_allclose(a.ode.values, y, rtol=1e-11, atol=1e-300)


def test_batched_solve_of_a_big_grid_stops_at_the_first_solve_that_does_not_converge():
    """the library's step loop used to run on after a solve had hit ksp_max_it -- up to a thousand steps on the bad
    iterate before Python saw it.  Now the batch ends AT that solve: with ``ksp_error_if_not_converged`` the exception comes with
    the state the failing step left (equal to the step() loop's, bit for bit), without it ``solve`` goes on from that iterate as the
    reference's loop does (src/beat/base_model.py:236-239 records and continues) and every step is still taken."""
    import beat
    from beat import grid as g
    from beat.base_model import Status
    from beat.models import tp06

    def build(strict, max_it):
        geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=8.0, Ly=4.0, Lz=2.0, dx=0.2)
        mesh = geo.mesh
        time = g.Constant(mesh, 0.0)
        cond = beat.conductivities.default_conductivities("Niederer")
        cells = g.locate_entities(mesh, 3, lambda x: np.logical_and(x[0] <= 1.0 + 1e-10, x[1] <= 1.0 + 1e-10))
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, start=0.2, duration=1.0)
        M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01, dx=I_s.dZ,
                                   params={"petsc_options": {"ksp_rtol": 1e-10, "ksp_max_it": max_it, "ksp_guess_order": 0,
                                                             "ksp_error_if_not_converged": strict}})
        ode = beat.odesolver.DolfinODESolver(
            v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
            init_states=tp06.init_state_values(), parameters=tp06.init_parameter_values(stim_amplitude=0.0),
            num_states=19, v_index=tp06.state_index("V"))
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode)

    dt = 0.05
    # resting tissue: the solves need next to nothing until the stimulus starts at t = 0.2 (step 4), whose solve needs more
    # than three iterations
    a = build(True, 3)
    assert a._can_batch(None)
    with pytest.raises(RuntimeError, match="did not converge"):
        a.solve((0.0, 20 * dt), dt)
    b = build(False, 3)
    failed_at = None
    ivs, t0 = [], 0.0  # the intervals as solve() forms them (t1 = t0 + dt accumulated: i * dt differs in the last bit)
    for i in range(20):
        ivs.append((t0, t0 + dt))
        t0 = t0 + dt
    for i in range(20):
        b.step(ivs[i])
        if b.pde.ksp.converged_reason < 0:
            failed_at = i
            break
    assert failed_at is not None and 2 <= failed_at <= 6
    np.testing.assert_array_equal(np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array))
    np.testing.assert_array_equal(a.ode.values, b.ode.values)
    assert a.pde.ksp.converged_reason < 0 and a.pde.ksp.iterations == 3
    # without the option: all 20 steps are taken, the status says what happened, the values are the step() loop's
    c = build(False, 3)
    c.solve((0.0, 20 * dt), dt)
    for i in range(failed_at + 1, 20):
        b.step(ivs[i])
    assert c.pde.status == Status.NOT_CONVERGING
    np.testing.assert_array_equal(c.ode.values, b.ode.values)


def test_split_steps_entry_refuses_what_it_does_not_cover(hip_ctx):
    """beat_split_steps is for grids the one-launch solve takes: a larger grid, an operator switched to the multi-launch
    kernels or more steps than BEAT_MAX_BATCH are refused with an error text (and MonodomainSplittingSolver.solve
    falls back to its step loop for them: _can_batch)."""
    import ctypes as C

    from beat import _hip, _stencil
    from beat._device import StateArray
    from beat._engine import HipOps
    from beat.models import tp06

    lib = hip_ctx.lib
    ic = tp06.init_state_values()
    p = np.ascontiguousarray(tp06.init_parameter_values(stim_amplitude=0.0))
    vi = tp06.state_index("V")

    def call(nn, nsteps, small=True):
        n = int(np.prod(nn))
        ops = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_tables(3, (0.1,) * 3, 1e-3))
        ops.set_small(small)
        ops.set_timestep(0.01, 0.5, 0.05)
        states = StateArray(hip_ctx, len(ic), n, nn[0] * nn[1])
        states.set(np.repeat(ic[:, None], n, axis=1))
        t0 = np.arange(nsteps, dtype=np.float64) * 0.05
        dts = np.full(nsteps, 0.05)
        infos = (_hip.KspInfo * max(1, nsteps))()
        rc = lib.beat_split_steps(hip_ctx.handle, _hip.MODEL_TP06_GRL1, states.ptr, n, states.ld, p.ctypes.data_as(C.c_void_p), len(p),
                                  vi, ops.handle, nsteps, t0.ctypes.data_as(C.c_void_p), dts.ctypes.data_as(C.c_void_p), None, None, 0,
                                  1e-10, 1e-50, 100, None, None, 0, None, infos)
        return rc, lib.beat_last_error().decode(), infos, states

    rc, _, infos, states = call((12, 10, 8), 5)
    assert rc == 0 and all(infos[k].converged_reason > 0 for k in range(5))
    assert np.isfinite(states.numpy()).all()
    rc, msg, _, _ = call((40, 40, 40), 2)
    assert rc != 0 and "one-launch" in msg
    rc, msg, _, _ = call((12, 10, 8), 2, small=False)
    assert rc != 0 and "one-launch" in msg
    rc, msg, _, _ = call((12, 10, 8), _hip.MAX_BATCH + 1)
    assert rc != 0 and "steps per call" in msg
