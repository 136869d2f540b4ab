"""GPU tests of the implicit Runge-Kutta monodomain model (beat.IrksomeMonodomainModel, csrc/beat_pde_rk.hip): one step
against a dense / sparse coupled solve of the stage system (tests/_rk_oracle.py), the complex COCG solve against SciPy, the
reference's tests/test_irksome_monodomain.py and tests/test_monodomain_solver.py:227-298 with their thresholds, temporal
order against the exact semi-discrete solution, and agreement with the theta-rule."""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

TABLEAUX = ["BackwardEuler()", "GaussLegendre(1)", "GaussLegendre(2)", "RadauIIA(2)", "RadauIIA(3)", "LobattoIIIA(2)",
            "LobattoIIIA(3)", "LobattoIIIC(2)", "LobattoIIIC(3)", "Alexander()"]
TIGHT = {"petsc_options": {"ksp_rtol": 1e-14, "ksp_atol": 1e-50}}


@pytest.fixture(autouse=True)
def _ctx(hip_ctx):
    return hip_ctx


def _tableau(expr):
    from beat import butcher

    return eval(expr, vars(butcher))


def _oracle_mesh(mesh):
    from oracle import fem

    return fem.BoxMesh(mesh.n, tuple(u - l for l, u in zip(mesh.lower, mesh.upper)), origin=mesh.lower)


def _sparse_coupled_step(Mm, K, C_m, A, b, c, dt, v, G, t0):
    s = len(b)
    S = sp.kron(sp.identity(s), C_m * Mm) + dt * sp.kron(sp.csr_matrix(np.asarray(A)), K)
    rhs = np.concatenate([G(t0 + c[i] * dt) - K @ v for i in range(s)])
    k = spla.spsolve(S.tocsc(), rhs).reshape(s, v.size)
    return v + dt * (np.asarray(b) @ k)


def _setup(dim):
    from beat import grid as g

    if dim == 2:
        mesh = g.create_unit_square(g.COMM_WORLD, 12, 12)
        Mten, C_m, dt = 1.0, 1.0, 0.05
    else:
        mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([1.5, 1.2, 0.9])], [15, 13, 11])
        Mten, C_m, dt = np.diag([1.0, 0.4, 0.15]), 0.5, 0.1
    return mesh, Mten, C_m, dt


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("expr", TABLEAUX)
def test_one_step_parity_with_coupled_stage_solve(expr, dim):
    _one_step_parity(expr, *_setup(dim))


def _setup_more(case):
    """Meshes beyond _setup's: a 1-D interval (all y / z rows collapsed), a 2-D box with nx > 64 and an off-diagonal
    tensor, a 3-D box with nx > 64, an off-diagonal tensor and C_m != 1."""
    from beat import grid as g

    if case == "interval300":
        return g.create_interval(g.COMM_WORLD, 300, [0.0, 3.0]), 1.0, 1.0, 0.05
    if case == "rect130x33":
        mesh = g.create_rectangle(g.COMM_WORLD, [np.zeros(2), np.array([2.6, 0.66])], [130, 33])
        return mesh, np.array([[2.0, 0.3], [0.3, 1.0]]), 1.0, 0.01
    f0 = np.array([np.cos(np.pi / 6), np.sin(np.pi / 6), 0.0])
    aniso3 = 9.5e-4 * np.outer(f0, f0) + 1.25e-4 * (np.eye(3) - np.outer(f0, f0))
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([1.4, 0.18, 0.1])], [70, 9, 5])
    return mesh, aniso3, 0.01, 0.05


@pytest.mark.parametrize("case", ["interval300", "rect130x33", "box70x9x5"])
@pytest.mark.parametrize("expr", TABLEAUX)
def test_one_step_parity_on_more_meshes(expr, case):
    _one_step_parity(expr, *_setup_more(case))


def _one_step_parity(expr, mesh, Mten, C_m, dt):
    """Two steps of the model against the sparse coupled stage solve: <= 1e-9 relative."""
    import beat
    from beat import grid as g
    from oracle import fem

    dim = mesh.dim
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    if dim == 1:
        I_s = (1.0 + x[0]) * (g.cos(3 * time) + 2.0)
        spatial = lambda p: 1.0 + p[0]  # noqa: E731
        v0 = lambda p: np.cos(np.pi * p[0])  # noqa: E731
    else:
        I_s = (1.0 + x[0] + 0.5 * x[1]) * (g.cos(3 * time) + 2.0)
        spatial = lambda p: 1.0 + p[0] + 0.5 * p[1]  # noqa: E731
        v0 = lambda p: np.cos(np.pi * p[0]) * (1.0 + p[1])  # noqa: E731
    t = _tableau(expr)
    model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=Mten, butcher_tableau=t, I_s=I_s, params=TIGHT, C_m=C_m)
    model.state.interpolate(v0)
    om = _oracle_mesh(mesh)
    Mm = fem.assemble_mass(om)
    K = fem.assemble_stiffness(om, Mten if np.ndim(Mten) else Mten * np.eye(dim))
    w = fem.load_vector(om, spatial)
    G = lambda tt: (np.cos(3 * tt) + 2.0) * w  # noqa: E731
    v = v0(om.x.T)
    t0 = 0.2
    for _ in range(2):
        model.step((t0, t0 + dt))
        assert float(time) == pytest.approx(t0 + dt, abs=1e-15)
        v = _sparse_coupled_step(Mm, K, C_m, t.A, t.b, t.c, dt, v, G, t0)
        t0 += dt
    got = np.asarray(model.state.x.array)
    assert np.abs(got - v).max() / np.abs(v).max() < 1e-9
    assert model.ksp.converged_reason > 0 and model.ksp.iterations > 0


def _moving_pulse(g, x, time, shift):
    """A stimulus that mixes x and t (no separable form): re-integrated at every stage time."""
    return g.exp(-((x[0] - shift - 0.5 * time) ** 2) / 0.05)


@pytest.mark.parametrize("mixed", [False, True], ids=["alone", "with_separable"])
@pytest.mark.parametrize("expr", ["Alexander()", "LobattoIIIA(2)", "RadauIIA(3)", "GaussLegendre(2)"])
def test_non_separable_stimulus_against_coupled_stage_solve(expr, mixed):
    """A stimulus that is not a product f(x) g(t) goes through _CompiledStimulus.general: its weights are integrated again
    at every stage time into per-stage load fields.  Alone and next to a separable stimulus (both kinds in one _merge),
    on the lower-triangular and the diagonalised paths, against the coupled stage solve with G(t) = int f(x, t) phi_i
    by the same quadrature (5 Gauss points per collapsed axis, stimulation.assemble_weights)."""
    import beat
    from beat import grid as g
    from beat.stimulation import Stimulus
    from oracle import fem

    mesh = g.create_rectangle(g.COMM_WORLD, [np.zeros(2), np.array([1.2, 0.6])], [48, 24])
    Mten, C_m, dt = np.array([[2.0, 0.3], [0.3, 1.0]]) * 0.1, 1.0, 0.05
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    dx = g.dx(domain=mesh)
    I_s = [Stimulus(expr=_moving_pulse(g, x, time, 0.3), dZ=dx)]
    if mixed:
        I_s.append(Stimulus(expr=(1.0 + x[0]) * (g.cos(3 * time) + 2.0), dZ=dx))
    t = _tableau(expr)
    model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=Mten, butcher_tableau=t, I_s=I_s, params=TIGHT, C_m=C_m)
    assert model._stimuli[0].general is not None
    assert not mixed or model._stimuli[1].general is None
    v0 = lambda p: np.cos(np.pi * p[0]) * (1.0 + p[1])  # noqa: E731
    model.state.interpolate(v0)
    om = _oracle_mesh(mesh)
    Mm = fem.assemble_mass(om)
    K = fem.assemble_stiffness(om, Mten)
    w_sep = fem.load_vector(om, lambda p: 1.0 + p[0], m=5)

    def G(tt):
        out = fem.load_vector(om, lambda p: np.exp(-((p[0] - 0.3 - 0.5 * tt) ** 2) / 0.05), m=5)
        return out + (np.cos(3 * tt) + 2.0) * w_sep if mixed else out

    v = v0(om.x.T)
    t0 = 0.1
    for _ in range(2):
        model.step((t0, t0 + dt))
        v = _sparse_coupled_step(Mm, K, C_m, t.A, t.b, t.c, dt, v, G, t0)
        t0 += dt
    got = np.asarray(model.state.x.array)
    assert np.abs(got - v).max() / np.abs(v).max() < 1e-9
    assert model.ksp.converged_reason > 0


def test_too_many_load_fields_are_refused():
    """RadauIIA(3) with three non-separable stimuli needs 3 x 3 = 9 load fields in a stage right-hand side, one more than
    the kernel takes: NotImplementedError, and the state is left as it was."""
    import beat
    from beat import grid as g
    from beat.stimulation import Stimulus

    mesh = g.create_unit_square(g.COMM_WORLD, 12, 12)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    dx = g.dx(domain=mesh)
    I_s = [Stimulus(expr=_moving_pulse(g, x, time, s), dZ=dx) for s in (0.2, 0.4, 0.6)]
    model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=1.0, butcher_tableau=_tableau("RadauIIA(3)"), I_s=I_s,
                                        params=TIGHT)
    model.state.interpolate(lambda p: np.cos(np.pi * p[0]))
    before = np.asarray(model.state.x.array).copy()
    with pytest.raises(NotImplementedError):
        model.step((0.0, 0.05))
    assert np.array_equal(np.asarray(model.state.x.array), before)
    # two of them fit (6 fields)
    time.value = 0.0
    model2 = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=1.0, butcher_tableau=_tableau("RadauIIA(3)"),
                                         I_s=I_s[:2], params=TIGHT)
    model2.step((0.0, 0.05))
    assert model2.ksp.converged_reason > 0


def test_complex_solve_against_scipy():
    import ctypes as C

    import beat
    from beat import _hip, grid as g
    from oracle import fem

    mesh, Mten, C_m, dt = _setup(3)
    model = beat.IrksomeMonodomainModel(time=g.Constant(mesh, 0.0), mesh=mesh, M=Mten, butcher_tableau=_tableau("RadauIIA(2)"))
    ops = model._ops
    om = _oracle_mesh(mesh)
    Mm = fem.assemble_mass(om)
    K = fem.assemble_stiffness(om, Mten)
    rng = np.random.default_rng(7)
    n = om.num_nodes
    b_re, b_im = rng.standard_normal(n), rng.standard_normal(n)
    a, lam = 0.5, complex(1 / 3, np.sqrt(2) / 6) * 0.1
    S = (a * Mm + lam * K).tocsc()
    ref = spla.spsolve(S, b_re + 1j * b_im)
    fr, fi, xr, xi = (ops.field(k) for k in ("t_br", "t_bi", "t_xr", "t_xi"))
    fr.set(b_re)
    fi.set(b_im)
    res = ops.solve(a, lam, fr, fi, xr, xi, 1e-13, 1e-50, 1000)
    got = xr.numpy() + 1j * xi.numpy()
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-9
    assert res.converged_reason > 0 and 1 < res.iterations < 1000
    print(f"COCG iterations: {res.iterations}")
    # the complex apply
    yr, yi = ops.field("t_yr"), ops.field("t_yi")
    _hip.check(ops.lib.beat_pde_zapply(ops.handle, a, lam.real, lam.imag, fr.ptr, fi.ptr, yr.ptr, yi.ptr))
    y = yr.numpy() + 1j * yi.numpy()
    yref = S @ (b_re + 1j * b_im)
    assert np.abs(y - yref).max() / np.abs(yref).max() < 1e-13
    # a real shift through the real instantiation
    res = ops.solve(a, 0.1, fr, None, xr, None, 1e-13, 1e-50, 1000)
    ref = spla.spsolve((a * Mm + 0.1 * K).tocsc(), b_re)
    assert np.abs(xr.numpy() - ref).max() / np.abs(ref).max() < 1e-9 and res.converged_reason > 0
    # max_it = 2 is reported, not raised
    res = ops.solve(a, lam, fr, fi, xr, xi, 1e-13, 1e-50, 2)
    assert res.converged_reason == -3 and res.iterations == 2
    assert C.sizeof(_hip.KspInfo) == 24


def test_max_it_reports_not_converging():
    import beat
    from beat import grid as g
    from beat.base_model import Status

    mesh = g.create_unit_square(g.COMM_WORLD, 15, 15)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * (g.cos(time) + 8 * g.pi**2 * g.sin(time))
    model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=1.0, butcher_tableau=_tableau("RadauIIA(2)"), I_s=I_s,
                                        params={"petsc_options": {"ksp_max_it": 2}})
    res = model.solve((0, 0.003), dt=0.001)
    assert res.status == Status.NOT_CONVERGING
    assert model.ksp.converged_reason < 0


def test_per_node_operators_are_refused():
    import beat
    from beat import grid as g

    mesh = g.create_unit_square(g.COMM_WORLD, 4, 4)
    per_cell = np.repeat(np.eye(2)[None], mesh.num_cells_global, axis=0)
    with pytest.raises(NotImplementedError):
        beat.IrksomeMonodomainModel(time=g.Constant(mesh, 0.0), mesh=mesh, M=per_cell, butcher_tableau=_tableau("RadauIIA(2)"))


# ---- the reference's tests/test_irksome_monodomain.py ---------------------------------------------------------------
def _l2_error(mesh, vh, exact):
    from oracle import fem

    return fem.l2_error(_oracle_mesh(mesh), np.asarray(vh), exact)


@pytest.mark.parametrize("M, w, err", [(0.0, 0.0, 1e-4), (1.0, 8.0, 2e-4), (2.0, 16.0, 2e-4)])
def test_irksome_monodomain_analytic(M, w, err):
    import beat
    from beat import grid as g
    from beat.base_model import Status

    N, dt = 15, 0.001
    T = 10 * dt
    mesh = g.create_unit_square(g.COMM_WORLD, N, N, g.CellType.triangle)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    t_var = g.variable(time)
    I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * (g.cos(t_var) + w * g.pi**2 * g.sin(t_var))
    model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=M, butcher_tableau=_tableau("RadauIIA(2)"), I_s=I_s,
                                        params=dict(petsc_options={"ksp_type": "preonly", "pc_type": "lu"}))
    res = model.solve((0, T), dt=dt)
    assert res.status == Status.OK
    assert float(time) == pytest.approx(T, abs=1e-12)
    e = _l2_error(mesh, res.state.x.array, lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(T))
    assert e < err


def test_irksome_monodomain_spatial_convergence():
    import beat
    from beat import grid as g

    dt = 0.001
    T = 10 * dt
    errors = []
    for N in (4, 8, 16, 32):
        mesh = g.create_unit_square(g.COMM_WORLD, N, N)
        time = g.Constant(mesh, 0.0)
        x = g.SpatialCoordinate(mesh)
        I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * (g.cos(time) + 8 * g.pi**2 * g.sin(time))
        model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=1.0, butcher_tableau=_tableau("RadauIIA(2)"), I_s=I_s)
        res = model.solve((0, T), dt=dt)
        errors.append(_l2_error(mesh, res.state.x.array,
                                lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(T)))
    rates = [np.log(e1 / e2) / np.log(2) for e1, e2 in zip(errors[:-1], errors[1:])]
    assert all(rate >= 2.0 for rate in rates), rates


@pytest.mark.parametrize("expr, check", [("GaussLegendre(1)", ("last", 1.9)), ("GaussLegendre(2)", ("last", 3.8)),
                                         ("RadauIIA(2)", ("all", 2.2))])
def test_temporal_order_against_semidiscrete_exact(expr, check):
    """P1 only here: the temporal error is measured against the exact solution of the semi-discrete system C_m M v' + K v
    = G(t) (generalised eigendecomposition), in the M-norm, over dt = 1, 1/2, 1/4, 1/8 to T = 1."""
    import beat
    from beat import grid as g
    from oracle import fem

    from _rk_oracle import semidiscrete_exact

    N, T = 16, 1.0
    mesh = g.create_unit_square(g.COMM_WORLD, N, N)
    om = _oracle_mesh(mesh)
    Mm = fem.assemble_mass(om).toarray()
    K = fem.assemble_stiffness(om, np.eye(2)).toarray()
    errors = []
    for dt in (1.0, 0.5, 0.25, 0.125):
        time = g.Constant(mesh, 0.0)
        x = g.SpatialCoordinate(mesh)
        I_s = g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * (g.cos(time) + 8 * g.pi**2 * g.sin(time))
        model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=1.0, butcher_tableau=_tableau(expr), I_s=I_s,
                                            params={"petsc_options": {"ksp_rtol": 1e-14, "ksp_atol": 1e-50}})
        # the load of the model itself: G(t) = (cos t + 8 pi^2 sin t) f
        stim = model._stimuli[0]
        time.value = 0.3
        f = stim.field.numpy() * stim.amplitude() / (np.cos(0.3) + 8 * np.pi**2 * np.sin(0.3))
        time.value = 0.0
        exact = semidiscrete_exact(Mm, K, 1.0, np.zeros(om.num_nodes), f, T)
        res = model.solve((0, T), dt=dt)
        e = np.asarray(res.state.x.array) - exact
        errors.append(np.sqrt(e @ Mm @ e))
    rates = [np.log(e1 / e2) / np.log(2) for e1, e2 in zip(errors[:-1], errors[1:])]
    kind, bound = check
    if kind == "last":
        assert rates[-1] >= bound, rates
    else:
        assert all(r >= bound for r in rates), rates


def test_backward_euler_agrees_with_theta_rule():
    import beat
    from beat import grid as g

    mesh, Mten, C_m, dt = _setup(3)
    out = []
    for kind in ("rk", "theta"):
        time = g.Constant(mesh, 0.0)
        x = g.SpatialCoordinate(mesh)
        I_s = (1.0 + x[0]) * g.sin(2 * time + 0.3)
        if kind == "rk":
            model = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=Mten, butcher_tableau=_tableau("BackwardEuler()"),
                                                I_s=I_s, C_m=C_m, params=TIGHT)
        else:
            model = beat.MonodomainModel(time=time, mesh=mesh, M=Mten, I_s=I_s, C_m=C_m, params=dict(theta=1.0, **TIGHT))
        model.state.interpolate(lambda p: np.exp(-((p[0] - 0.7) ** 2 + (p[1] - 0.5) ** 2) / 0.1))
        if kind == "theta":
            model.assign_previous()
        model.solve((0.0, 5 * dt), dt=dt)
        out.append(np.asarray(model.state.x.array).copy())
    assert np.abs(out[0] - out[1]).max() / np.abs(out[1]).max() < 1e-10


def test_irksome_monodomain_splitting_analytic(monkeypatch):
    """tests/test_monodomain_solver.py:227-298 (BackwardEuler, N = 50, dt = 0.01, T = 1, E < 0.002) through
    MonodomainSplittingSolver: the literal sequence, never a fused or batched route."""
    import beat
    from beat import grid as g

    for name in ("_fused_step", "_fused_multi_step", "_batched_steps", "_batched_steps_big"):
        def boom(*a, _name=name, **k):
            raise AssertionError(f"{_name} entered with an IrksomeMonodomainModel")

        monkeypatch.setattr(beat.MonodomainSplittingSolver, name, boom)
    N, M, dt, T, t0 = 50, 1.0, 0.01, 1.0, 0.0
    mesh = g.create_unit_square(g.COMM_WORLD, N, N)
    time = g.Constant(mesh, 0.0)
    x = g.SpatialCoordinate(mesh)
    I_s = 8 * g.pi**2 * g.cos(2 * g.pi * x[0]) * g.cos(2 * g.pi * x[1]) * g.sin(time)
    pde = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=M, butcher_tableau=_tableau("BackwardEuler()"), I_s=I_s,
                                      params=dict(petsc_options={"ksp_type": "preonly", "pc_type": "lu"}))
    V_ode = beat.utils.space_from_string("P_1", mesh, dim=1)
    v_ode = g.Function(V_ode)
    s = g.Function(V_ode)
    s.interpolate(lambda p: -np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.cos(0.0))
    init_states = np.zeros((2, s.x.array.size))
    init_states[1, :] = np.asarray(s.x.array)
    ode = beat.odesolver.DolfinODESolver(v_ode=v_ode, v_pde=pde.state, fun=beat.models.simple.forward_euler,
                                         init_states=init_states, parameters=None, num_states=2, v_index=0)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    assert not solver._can_fuse() and not solver._can_fuse_multi() and not solver._can_batch(None)
    solver.solve((t0, T), dt=dt)
    E = _l2_error(mesh, pde.state.x.array,
                  lambda p: np.cos(2 * np.pi * p[0]) * np.cos(2 * np.pi * p[1]) * np.sin(float(time)))
    assert E < 0.002
    assert np.array_equal(ode.values[0], np.asarray(pde.state.x.array))
