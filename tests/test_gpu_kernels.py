"""GPU parity tests proper: every HIP kernel called through the C-ABI (ctypes) and compared
with the CPU oracle on the same seeded inputs.  Floating-point tolerances are stated per test
(all arithmetic is fp64; exp/log come from different libms on the two sides)."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["one-launch", "multi-launch"])
def small_grid_path(request):
    """Grids of a few thousand nodes are solved by one workgroup in one launch (csrc/beat_pde_small.hip) unless the
    operator is told otherwise: every test of this module runs on both paths."""
    from beat._engine import HipOps

    old = HipOps.default_small
    HipOps.default_small = request.param == "one-launch"
    yield request.param
    HipOps.default_small = old


def _ptr_array(ptrs):
    arr = (C.c_void_p * max(1, len(ptrs)))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def _dbl_array(vals):
    arr = (C.c_double * max(1, len(vals)))()
    for i, v in enumerate(vals):
        arr[i] = v
    return arr


def _ode_step(ctx, model_id, states, params, t, dt, v_index=0, v_copy=None, ppn=None):
    from beat import _hip
    from beat._device import StateArray

    S, n = states.shape
    sa = StateArray(ctx, S, n)
    sa.set(states)
    hp = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    npar = 0 if hp is None else len(hp)
    ppn_t = None
    if ppn is not None:
        ppn_t = ctx.from_numpy(np.ascontiguousarray(ppn, dtype=np.float64))
        npar = ppn.shape[0]
    _hip.check(
        ctx.lib.beat_ode_step(
            ctx.handle, model_id, sa.ptr, n, sa.ld,
            None if hp is None or ppn is not None else hp.ctypes.data_as(C.c_void_p), npar,
            None if ppn_t is None else C.c_void_p(ppn_t.data_ptr()), 0 if ppn is None else ppn.shape[1],
            float(t), float(dt), v_index, None if v_copy is None else v_copy.ptr,
        )
    )
    ctx.synchronize()
    return sa.numpy()


def _random_tp06_states(n, seed):
    from oracle import ionic

    rng = np.random.default_rng(seed)
    S = np.repeat(ionic.tp06_init_state_values()[:, None], n, axis=1)
    idx = ionic.tp06_state_index
    S[idx("V")] = rng.uniform(-95, 50, n)
    for g in ["Xr1", "Xr2", "Xs", "m", "h", "j", "d", "f", "f2", "fCass", "s", "r", "R_prime"]:
        S[idx(g)] = rng.uniform(0, 1, n)
    S[idx("Ca_i")] = 10 ** rng.uniform(-4.2, -2.8, n)
    S[idx("Ca_ss")] = 10 ** rng.uniform(-4, -2, n)
    S[idx("Ca_SR")] = rng.uniform(1, 4.5, n)
    S[idx("Na_i")] = rng.uniform(6, 12, n)
    S[idx("K_i")] = rng.uniform(125, 145, n)
    return S


def test_simple_ode_and_fhn_match_oracle(hip_ctx):
    from beat import _hip
    from oracle import ionic

    rng = np.random.default_rng(1)
    n = 10007
    st = rng.standard_normal((2, n))
    out = _ode_step(hip_ctx, _hip.MODEL_SIMPLE_ODE, st, np.array([1.5, 0.5]), 0.0, 0.1)
    ref = ionic.simple_ode_forward_euler(st, 0.0, 0.1, np.array([1.5, 0.5]))
    np.testing.assert_allclose(out, ref, rtol=1e-15, atol=1e-15)
    out = _ode_step(hip_ctx, _hip.MODEL_SIMPLE_ODE, st, None, 0.0, 0.1)
    np.testing.assert_allclose(out, ionic.simple_ode_forward_euler(st, 0.0, 0.1), rtol=1e-15, atol=1e-15)

    st = np.stack([rng.uniform(-0.5, 2, n), rng.uniform(-90, 45, n)])
    p_demo = np.array([40.0, -85.0, 0.13, 0.013, 0.26, 0.1, 1.0, 100.0, 1.0, 0.0])
    for t in (0.5, 3.0):
        out = _ode_step(hip_ctx, _hip.MODEL_FHN_DEMO, st, p_demo, t, 0.01)
        np.testing.assert_allclose(out, ionic.fhn_demo_forward_euler(st, t, 0.01, p_demo), rtol=1e-14, atol=1e-14)
    p_readme = np.array([0.26, 0.1, 1.0, 0.13, 0.013, 125.0, -85.0, 40.0, 100.0, 1.0, 0.0])
    for t in (0.5, 1.0, 3.0):
        out = _ode_step(hip_ctx, _hip.MODEL_FHN_README, st, p_readme, t, 0.01)
        np.testing.assert_allclose(out, ionic.fhn_readme_forward_euler(st, t, 0.01, p_readme), rtol=1e-14, atol=1e-14)


def test_tp06_grl1_one_step_matches_oracle(hip_ctx):
    """One GRL1 step on 20k random physiological states: |HIP - oracle| <= 1e-11 relative to the
    state scale (different exp/log implementations; the update multiplies rounding by <= dt*|J|).
    i_CaL = ... / (exp(2 (V-15) F/RT) - 1) has a removable singularity at V = 15 mV where the
    reference's own formula loses digits; nodes within 0.05 mV of it get 1e-8."""
    from beat import _hip
    from oracle import ionic

    n = 20011
    S = _random_tp06_states(n, 11)
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    for dt in (0.05, 0.01):
        out = _ode_step(hip_ctx, _hip.MODEL_TP06_GRL1, S, P, 1.0, dt)
        ref = ionic.tp06_generalized_rush_larsen(S, 1.0, dt, P)
        scale = np.maximum(np.abs(ref), 1e-3)
        err = np.abs(out - ref) / scale
        assert np.isfinite(out).all()
        near = np.abs(S[17] - 15.0) < 0.05
        assert err[:, ~near].max() < 1e-11, (err[:, ~near].max(), np.unravel_index(err.argmax(), err.shape))
        assert err[:, near].max() < 1e-8


def test_tp06_grl1_increment_matches_oracle_on_both_sides_of_the_polynomial_window(hip_ctx):
    """Round 6: the GRL1 increment of TP06's seven non-gate states is ``f dt phi(J dt)`` with phi by its Taylor polynomial when
    |J dt| <= 1/16 and the scheme's literal ``f (exp(J dt) - 1) / J`` outside (csrc/ionic_models.h: advance).  Random physiological
    states stepped with time steps from 0.001 to 1 ms put |J_V dt| from 1e-4 to beyond 10 -- both branches of every state and
    lanes of one wavefront on either side; each dt against the NumPy oracle (the literal expression throughout) to 1e-11 of the
    state scale, as the one-step test asks of dt = 0.01 / 0.05."""
    from beat import _hip
    from oracle import ionic

    n = 8192
    S = _random_tp06_states(n, 23)
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    near = np.abs(S[17] - 15.0) < 0.05  # (the i_CaL singularity: see test_tp06_grl1_one_step_matches_oracle)
    for dt in (0.001, 0.02, 0.1, 0.3, 1.0):
        out = _ode_step(hip_ctx, _hip.MODEL_TP06_GRL1, S, P, 1.0, dt)
        ref = ionic.tp06_generalized_rush_larsen(S, 1.0, dt, P)
        ok = np.isfinite(ref).all(axis=0) & ~near
        scale = np.maximum(np.abs(ref), 1e-3)
        err = (np.abs(out - ref) / scale)[:, ok]
        assert np.isfinite(out[:, ok]).all() and err.max() < 1e-11, (dt, err.max())
    # the window is really straddled: the potential's own J dt = -dt dI/dV lies on both sides at dt = 0.1
    out1, out2 = (_ode_step(hip_ctx, _hip.MODEL_TP06_GRL1, S, P, 1.0, d)[17] for d in (0.1, 0.1 * (1 + 1e-9)))
    assert np.isfinite(out1).all() and np.abs(out1 - out2).max() < 1e-6  # (continuous across the switch)


def test_state_array_keeps_the_best_of_three_placements(hip_ctx, monkeypatch):
    """Round 6: where the driver puts a large state array decides how fast its rows stream (profiles/r06_placement.md);
    ``StateArray`` allocates up to BEAT_STATE_PLACE candidates, times the library's streaming probe of the ionic kernels' access
    pattern on each and keeps the best.  With the size threshold lowered for the test (the product: 1 GB): the record names three
    rates and the index of the largest, the array is zero-filled and of the layout an unplaced one has, a TP06 step on it equals the
    step on an unplaced array bit for bit, and BEAT_STATE_PLACE=1 switches the choice off."""
    from beat import _hip
    from beat._device import StateArray
    from oracle import ionic

    n, S = 1 << 18, 19
    monkeypatch.setenv("BEAT_STATE_PLACE_MIN_BYTES", str(1 << 20))
    a = StateArray(hip_ctx, S, n, 4096)
    rec = a.placement
    assert rec is not None and len(rec["candidates"]) == 3 and rec["rows_probed"] == 19
    assert rec["chosen"] == int(np.argmax(rec["candidates"])) and min(rec["candidates"]) > 0.0
    assert float(a.buf.abs().max()) == 0.0
    monkeypatch.setenv("BEAT_STATE_PLACE", "1")
    b = StateArray(hip_ctx, S, n, 4096)
    assert b.placement is None and (b.ld, b.base, tuple(b.rows.shape)) == (a.ld, a.base, tuple(a.rows.shape))
    st = _random_tp06_states(n, 5)
    P = np.ascontiguousarray(ionic.tp06_init_parameter_values(stim_amplitude=0.0))
    outs = []
    for sa in (a, b):
        sa.set(st)
        _hip.check(hip_ctx.lib.beat_ode_step(hip_ctx.handle, _hip.MODEL_TP06_GRL1, sa.ptr, n, sa.ld, P.ctypes.data_as(C.c_void_p), len(P),
                                             None, 0, 1.0, 0.02, 17, None))
        hip_ctx.synchronize()
        outs.append(sa.numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    # a row count the probe has no instance for takes the largest it has; an odd plane (rows not 16-byte aligned) is not probed
    monkeypatch.setenv("BEAT_STATE_PLACE", "2")
    c = StateArray(hip_ctx, 7, n, 0)
    assert c.placement is not None and c.placement["rows_probed"] == 4 and len(c.placement["candidates"]) == 2
    d = StateArray(hip_ctx, 7, n + 1, 3)
    assert float(d.buf.abs().max()) == 0.0  # (placed or not: a usable array either way)
    assert list(d.placement) == ["skipped"] and "16-byte" in d.placement["skipped"]


def test_work_fields_keep_the_best_of_three_placements(hip_ctx, monkeypatch):
    """The PCG's work fields (r, q, z, the ring) are placed by the state array's routine with the 4-row probe.  With the size
    threshold lowered for the test: the record names three rates and the index of the largest, the buffer is zero-filled and of the
    layout an unplaced one has, and a solve on it equals the solve on an unplaced buffer (BEAT_WORK_PLACE=1) bit for bit."""
    from beat import _stencil
    from beat._engine import DiffusionSolver, HipOps, Slab

    nn = (64, 64, 64)
    tabs = _stencil.stencil_tables(3, (0.1, 0.1, 0.1), 1e-3)
    monkeypatch.setenv("BEAT_STATE_PLACE_MIN_BYTES", str(1 << 20))
    placed = HipOps(hip_ctx, nn, True, True, *tabs)
    rec = placed.work_placement
    assert rec is not None and len(rec["candidates"]) == 3 and rec["rows_probed"] == 4
    assert rec["chosen"] == int(np.argmax(rec["candidates"])) and min(rec["candidates"]) > 0.0
    assert float(placed.work.abs().max()) == 0.0
    monkeypatch.setenv("BEAT_WORK_PLACE", "1")
    plain = HipOps(hip_ctx, nn, True, True, *tabs)
    assert plain.work_placement is None and plain.work.numel() == placed.work.numel()
    layout = lambda ops: [f.offset for f in (ops.r, ops.q, ops.z, *ops.ring)]  # noqa: E731
    assert layout(plain) == layout(placed)
    v = -85.0 + 30.0 * np.random.default_rng(5).random(placed.n)
    outs = []
    for ops in (placed, plain):
        ops.set_timestep(0.01, 0.5, 0.05)
        fv, fx = ops.new_field(), ops.new_field()
        fv.set(v)
        res = DiffusionSolver(ops, Slab(nn[2])).solve(fv, [], [], fx, rtol=1e-10, atol=1e-50, max_it=500)
        assert res.converged_reason > 0
        outs.append(fx.numpy())
    np.testing.assert_array_equal(outs[0], outs[1])


def test_tp06_many_steps_and_stimulus_window(hip_ctx):
    """2000 steps (20 ms at dt = 0.01) through an upstroke triggered by the model's own i_Stim:
    trajectories agree to 1e-7 relative (error growth through the stiff upstroke)."""
    from beat import _hip
    from beat._device import StateArray
    from oracle import ionic

    n = 257
    S0 = np.repeat(ionic.tp06_init_state_values()[:, None], n, axis=1)
    S0[ionic.tp06_state_index("V")] += np.linspace(0, 5, n)
    P = ionic.tp06_init_parameter_values(stim_start=1.0)
    sa = StateArray(hip_ctx, 19, n)
    sa.set(S0)
    ref = S0.copy()
    dt = 0.01
    t = 0.0
    for _ in range(2000):
        _hip.check(hip_ctx.lib.beat_ode_step(hip_ctx.handle, _hip.MODEL_TP06_GRL1, sa.ptr, n, sa.ld,
                                              P.ctypes.data_as(C.c_void_p), 53, None, 0, t, dt, 17, None))
        ref = ionic.tp06_generalized_rush_larsen(ref, t, dt, P)
        t += dt
    out = sa.numpy()
    assert ref[17].max() > 0.0  # the cells fired
    err = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-3)
    assert err.max() < 1e-7, err.max()


def test_tp06_per_node_parameters_and_v_copy(hip_ctx):
    from beat import _hip
    from beat._device import Field
    from oracle import ionic

    n = 1000
    S = _random_tp06_states(n, 5)
    P = np.repeat(ionic.tp06_init_parameter_values(stim_amplitude=0.0)[:, None], n, axis=1)
    rng = np.random.default_rng(2)
    P[ionic.tp06_parameter_index("g_Ks")] *= rng.uniform(0.5, 2.0, n)
    P[ionic.tp06_parameter_index("g_to")] *= rng.uniform(0.5, 2.0, n)
    vcopy = Field(hip_ctx, n, 0)
    out = _ode_step(hip_ctx, _hip.MODEL_TP06_GRL1, S, None, 0.0, 0.02, v_index=17, v_copy=vcopy, ppn=P)
    ref = ionic.tp06_generalized_rush_larsen(S, 0.0, 0.02, P)
    err = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-3)
    assert err.max() < 1e-11
    np.testing.assert_array_equal(vcopy.numpy(), out[17])


GRIDS = [
    # (cells per axis, box lengths, conductivity)
    ((70, 37, 9), (7.0, 3.7, 0.9), "aniso3"),
    ((40, 14, 6), (20.0, 7.0, 3.0), "niederer"),
    ((4, 1, 2), (2.0, 0.5, 1.0), "aniso3"),
    ((24, 20, 12), (2.4, 2.0, 1.2), "iso3"),  # BASELINE.json configs[2]: M = s I, h = 0.1 mm (7-point stiffness inside the 15-point row)
    ((130, 33), (1.0, 1.0), "aniso2"),
    ((10,), (1.0,), 1.0),
]


def _conductivity(kind, dim):
    if kind == "aniso3":
        f0 = np.array([np.cos(np.pi / 6), np.sin(np.pi / 6), 0.0])
        return 9.5e-4 * np.outer(f0, f0) + 1.25e-4 * (np.eye(3) - np.outer(f0, f0))
    if kind == "niederer":
        return np.diag([9.5301e-4, 1.2576e-4, 1.2576e-4])
    if kind == "iso3":
        return 9.5301e-4 * np.eye(3)
    if kind == "aniso2":
        return np.array([[2.0, 0.3], [0.3, 1.0]])
    return kind


def _make_pde(ctx, cells, L, Mk, z_lo_phys=1, z_hi_phys=1):
    from beat import _hip, _stencil

    dim = len(cells)
    h = tuple(l / c for l, c in zip(L, cells))
    mt, kt = _stencil.stencil_tables(dim, h, _conductivity(Mk, dim))
    nn = [c + 1 for c in cells] + [1] * (3 - dim)
    n3 = (C.c_int64 * 3)(*nn)
    handle = C.c_void_p()
    mt = np.ascontiguousarray(mt)
    kt = np.ascontiguousarray(kt)
    _hip.check(ctx.lib.beat_pde_create(ctx.handle, n3, z_lo_phys, z_hi_phys, mt.ctypes.data_as(C.c_void_p),
                                       kt.ctypes.data_as(C.c_void_p), C.byref(handle)))
    return handle, nn, mt, kt


# (C_m, theta, dt) of the diffusion operator: Crank-Nicolson, backward Euler, and a set in which C_m, theta dt, (1 - theta) dt and dt
# are four different numbers (tests/_pcg_ref.py says what each is for).  At theta = 1/2 A and B have the same factor of K.
OPSETS = {"cn": (0.01, 0.5, 0.05), "be": (0.01, 1.0, 0.05), "skew": (0.013, 0.25, 0.08)}


@pytest.mark.parametrize("cells,L,Mk", GRIDS)
def test_stencil_operators_match_assembled_matrices(hip_ctx, cells, L, Mk, opset="cn"):
    """y = Mass x, K x, A x, B x from the LDS-tiled stencil vs the oracle's literally assembled
    sparse matrices: <= 1e-13 relative to ||row||_1 * max|x| (15-term fp64 sums)."""
    from beat import _hip
    from beat._device import Field
    from oracle import fem

    ctx = hip_ctx
    dim = len(cells)
    mesh = fem.BoxMesh(cells, L)
    handle, nn, _, _ = _make_pde(ctx, cells, L, Mk)
    Mass = fem.assemble_mass(mesh)
    K = fem.assemble_stiffness(mesh, _conductivity(Mk, dim))
    C_m, theta, dt = OPSETS[opset]
    _hip.check(ctx.lib.beat_pde_set_timestep(handle, C_m, theta, dt))
    mats = {0: C_m * Mass + theta * dt * K, 1: C_m * Mass - (1 - theta) * dt * K, 2: Mass, 3: K}
    n = mesh.num_nodes
    plane = nn[0] * nn[1]
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n)
    fx, fy = Field(ctx, n, plane), Field(ctx, n, plane)
    fx.set(x)
    # poison the ghost planes: physical faces must ignore them
    fx.ghost_lo.fill_(float("nan"))
    fx.ghost_hi.fill_(float("nan"))
    for which, mat in mats.items():
        _hip.check(ctx.lib.beat_pde_apply(handle, which, fx.ptr, fy.ptr))
        ctx.synchronize()
        ref = mat @ x
        scale = (abs(mat) @ np.ones(n)).max() * np.abs(x).max()
        assert np.abs(fy.numpy() - ref).max() <= 1e-13 * scale, which
    _hip.check(ctx.lib.beat_pde_destroy(handle))


@pytest.mark.parametrize("opset", ("be", "skew"))
@pytest.mark.parametrize("cells,L,Mk", GRIDS)
def test_stencil_operators_match_assembled_matrices_off_theta_one_half(hip_ctx, cells, L, Mk, opset):
    """The test above with A and B two different matrices."""
    test_stencil_operators_match_assembled_matrices(hip_ctx, cells, L, Mk, opset)


def test_stencil_slab_ghost_planes(hip_ctx):
    """A z-slab with live ghost planes reproduces the rows of the undivided operator."""
    from beat import _hip
    from beat._device import Field
    from oracle import fem

    ctx = hip_ctx
    cells, L = (20, 9, 11), (2.0, 0.9, 1.1)
    mesh = fem.BoxMesh(cells, L)
    A = fem.assemble_mass(mesh) + 0.3 * fem.assemble_stiffness(mesh, _conductivity("aniso3", 3))
    nx, ny, nz = (c + 1 for c in cells)
    plane = nx * ny
    rng = np.random.default_rng(4)
    x = rng.standard_normal(mesh.num_nodes)
    ref = (A @ x).reshape(nz, plane)
    X = x.reshape(nz, plane)
    for z0, z1 in ((0, 4), (4, 9), (9, 12)):
        from beat import _stencil

        h = tuple(l / c for l, c in zip(L, cells))
        mt, kt = _stencil.stencil_tables(3, h, _conductivity("aniso3", 3))
        n3 = (C.c_int64 * 3)(nx, ny, z1 - z0)
        handle = C.c_void_p()
        _hip.check(ctx.lib.beat_pde_create(ctx.handle, n3, int(z0 == 0), int(z1 == nz),
                                           mt.ctypes.data_as(C.c_void_p), kt.ctypes.data_as(C.c_void_p),
                                           C.byref(handle)))
        _hip.check(ctx.lib.beat_pde_set_timestep(handle, 1.0, 1.0, 0.3))
        nloc = (z1 - z0) * plane
        fx, fy = Field(ctx, nloc, plane), Field(ctx, nloc, plane)
        fx.set(X[z0:z1].ravel())
        if z0 > 0:
            fx.ghost_lo.copy_(ctx.from_numpy(X[z0 - 1]))
        if z1 < nz:
            fx.ghost_hi.copy_(ctx.from_numpy(X[z1]))
        _hip.check(ctx.lib.beat_pde_apply(handle, 0, fx.ptr, fy.ptr))
        ctx.synchronize()
        np.testing.assert_allclose(fy.numpy().reshape(-1, plane), ref[z0:z1], rtol=0, atol=1e-12)
        _hip.check(ctx.lib.beat_pde_destroy(handle))


@pytest.mark.parametrize("cells,L,Mk", GRIDS[:2] + GRIDS[3:])  # (all but the 5 x 2 x 3-node grid)
def test_pde_solve_matches_direct_solve(hip_ctx, cells, L, Mk, opset="cn"):
    """One theta-step: rhs build + Jacobi-PCG (rtol 1e-12) vs the oracle's sparse-LU solve of
    (C_m Mass + theta dt K) v = (C_m Mass - (1-theta) dt K) v_ + dt b_stim: <= 1e-9 * max|v|."""
    from beat import _hip
    from beat._device import Field
    from oracle import fem

    ctx = hip_ctx
    dim = len(cells)
    mesh = fem.BoxMesh(cells, L)
    Mten = _conductivity(Mk, dim)
    C_m, theta, dt = OPSETS[opset]
    if Mk == "aniso2" or Mk == 1.0:
        C_m, dt = 1.0, 1e-3
    handle, nn, _, _ = _make_pde(ctx, cells, L, Mk)
    _hip.check(ctx.lib.beat_pde_set_timestep(handle, C_m, theta, dt))
    n = mesh.num_nodes
    plane = nn[0] * nn[1]
    rng = np.random.default_rng(8)
    v_prev = -85.0 + 100.0 * np.exp(-((mesh.x - 0.3 * np.array(L)) ** 2).sum(axis=1) / (0.05 * max(L) ** 2))
    v_prev += 0.01 * rng.standard_normal(n)
    cellsel = mesh.locate_cells(lambda x: x[0] <= 0.25 * L[0] + 1e-10)
    w = fem.stimulus_weights(mesh, cellsel)
    amp = 0.357
    model = fem.OracleMonodomainModel(mesh, Mten, [fem.OracleStimulus(lambda t: amp, w)], C_m=C_m, theta=theta,
                                      default_timestep=dt)
    model.state[:] = v_prev
    model.assign_previous()
    model.step((0.0, dt))
    fv, fx, fw = Field(ctx, n, plane), Field(ctx, n, plane), Field(ctx, n, plane)
    fv.set(v_prev)
    fw.set(w)
    work = ctx.zeros(ctx.lib.beat_pde_work_fields(handle) * ctx.lib.beat_pde_field_stride(handle))
    info = _hip.KspInfo()
    _hip.check(ctx.lib.beat_pde_solve(handle, fv.ptr, _ptr_array([fw.ptr.value]), _dbl_array([amp]), 1, fx.ptr,
                                      C.c_void_p(work.data_ptr()), 1e-12, 1e-50, 500, C.byref(info)))
    out = fx.numpy()
    assert info.converged_reason > 0 and 0 < info.iterations < 200
    assert np.abs(out - model.state).max() <= 1e-9 * np.abs(model.state).max()
    # the same iteration count as the oracle's restatement of the PCG (same algorithm, same x0)
    A = (C_m * fem.assemble_mass(mesh) + theta * dt * fem.assemble_stiffness(mesh, Mten)).tocsr()
    _, its, _ = fem.pcg_jacobi(A, model.rhs(theta * dt, dt), v_prev, rtol=1e-12)
    assert abs(its - info.iterations) <= 1
    _hip.check(ctx.lib.beat_pde_destroy(handle))


@pytest.mark.parametrize("opset", ("be", "skew"))
@pytest.mark.parametrize("cells,L,Mk", GRIDS[:2] + GRIDS[3:])
def test_pde_solve_matches_direct_solve_off_theta_one_half(hip_ctx, cells, L, Mk, opset):
    """The test above with theta = 1 and theta = 1/4: the right-hand side's factor of K is not the matrix's."""
    test_pde_solve_matches_direct_solve(hip_ctx, cells, L, Mk, opset)


def test_pde_solve_zero_rhs_and_latch(hip_ctx):
    """b = 0 (M = 0, no stimulus, v_ = 0) converges in 0 iterations with reason > 0."""
    from beat import _hip
    from beat._device import Field

    ctx = hip_ctx
    handle, nn, _, _ = _make_pde(ctx, (10,), (1.0,), 0.0)
    _hip.check(ctx.lib.beat_pde_set_timestep(handle, 1.0, 0.5, 0.4))
    n, plane = 11, 11
    fv, fx = Field(ctx, n, plane), Field(ctx, n, plane)
    work = ctx.zeros(ctx.lib.beat_pde_work_fields(handle) * ctx.lib.beat_pde_field_stride(handle))
    info = _hip.KspInfo()
    _hip.check(ctx.lib.beat_pde_solve(handle, fv.ptr, _ptr_array([]), _dbl_array([]), 0, fx.ptr,
                                      C.c_void_p(work.data_ptr()), 1e-10, 1e-50, 100, C.byref(info)))
    assert info.iterations == 0 and info.converged_reason > 0
    assert np.all(fx.numpy() == 0.0)


def test_field_utilities(hip_ctx):
    from beat import _hip
    from beat._device import Field

    ctx = hip_ctx
    rng = np.random.default_rng(0)
    n = 100003
    a, b = Field(ctx, n, 0), Field(ctx, n, 0)
    x = rng.standard_normal(n)
    a.set(x)
    b.copy_from(a)
    np.testing.assert_array_equal(b.numpy(), x)
    lo, hi = a.minmax()
    assert lo == x.min() and hi == x.max()
    b.fill(2.5)
    assert np.all(b.numpy() == 2.5)
    idx = rng.permutation(n)[: n // 3].astype(np.int64)
    didx = ctx.from_numpy(idx)
    g = Field(ctx, len(idx), 0)
    _hip.check(ctx.lib.beat_gather(ctx.handle, g.ptr, a.ptr, C.c_void_p(didx.data_ptr()), len(idx)))
    np.testing.assert_array_equal(g.numpy(), x[idx])
    _hip.check(ctx.lib.beat_scatter(ctx.handle, b.ptr, g.ptr, C.c_void_p(didx.data_ptr()), len(idx)))
    ref = np.full(n, 2.5)
    ref[idx] = x[idx]
    np.testing.assert_array_equal(b.numpy(), ref)
    # P1 point evaluation
    pidx = np.array([[0, 1, 2, 3], [5, 5, 5, 5]], dtype=np.int64)
    w = np.array([[0.1, 0.2, 0.3, 0.4], [1.0, 0.0, 0.0, 0.0]])
    out = np.zeros(2)
    _hip.check(ctx.lib.beat_field_probe(ctx.handle, a.ptr, pidx.ctypes.data_as(C.c_void_p),
                                        w.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p)))
    np.testing.assert_allclose(out, [w[0] @ x[:4], x[5]], rtol=1e-15)


def test_stream_probe_moves_the_bytes_it_claims(hip_ctx, small_grid_path):
    """beat_stream_probe (csrc/beat_probe.hip; bench.py's roofline.inplace_stream) touches what each mode says and nothing
    else: in place leaves every bit, copy reproduces the first half in the second, write only fills, read only and the row
    pattern leave the array as it was -- for every cache policy, global and raw-buffer instructions, 1 / 2 / 4 accesses in
    flight, looping and one-workgroup-per-chunk grids, and a length that is not a multiple of anything."""
    if small_grid_path != "one-launch":
        pytest.skip("independent of the solve path")
    from beat import _hip
    from beat._device import StateArray

    ctx = hip_ctx
    rng = np.random.default_rng(11)
    n = 2 * 50_021
    buf = ctx.from_numpy(rng.standard_normal(n))
    ref = buf.cpu().numpy().copy()
    ptr = C.c_void_p(buf.data_ptr())
    for policy in range(8):
        for unroll in (1, 2, 4):
            for blocks in (0, 7):
                _hip.check(ctx.lib.beat_stream_probe(ctx.handle, ptr, n, 0, policy, unroll, blocks, 0, 0))
                if not (policy & 2):
                    _hip.check(ctx.lib.beat_stream_probe(ctx.handle, ptr, n, 1, policy, unroll, blocks, 0, 0))
                assert np.array_equal(buf.cpu().numpy(), ref), (policy, unroll, blocks)
                cp = buf.clone()
                _hip.check(ctx.lib.beat_stream_probe(ctx.handle, C.c_void_p(cp.data_ptr()), n, 3, policy, unroll, blocks, 0, 0))
                out = cp.cpu().numpy()
                half = n // 4 * 2  # 16-byte elements: (n / 2) / 2 of them are copied
                assert np.array_equal(out[:half], ref[:half]) and np.array_equal(out[half:2 * half], ref[:half]), (policy, unroll, blocks)
                assert np.array_equal(out[2 * half:], ref[2 * half:])
                if not (policy & 1):
                    _hip.check(ctx.lib.beat_stream_probe(ctx.handle, C.c_void_p(cp.data_ptr()), n, 2, policy, unroll, blocks, 0, 0))
                    assert not cp.cpu().numpy().any()
    sa = StateArray(ctx, 19, 10_002, 0)
    vals = rng.standard_normal((19, 10_002))
    sa.set(vals)
    for policy in range(4):
        for blocks in (0, 5):
            _hip.check(ctx.lib.beat_stream_probe(ctx.handle, sa.ptr, sa.n, 4, policy, 1, blocks, 19, sa.ld))
    assert np.array_equal(sa.numpy(), vals)
    with pytest.raises(_hip.BeatHipError):
        _hip.check(ctx.lib.beat_stream_probe(ctx.handle, ptr, n, 9, 0, 1, 0, 0, 0))
    with pytest.raises(_hip.BeatHipError):
        _hip.check(ctx.lib.beat_stream_probe(ctx.handle, sa.ptr, sa.n, 4, 0, 1, 0, 7, sa.ld))


@pytest.mark.parametrize("lo_phys,hi_phys,nzl", [(0, 0, 5), (1, 0, 4), (0, 1, 3), (0, 0, 1), (0, 0, 2), (1, 1, 4)])
def test_spmv_in_two_parts_equals_whole(hip_ctx, lo_phys, hi_phys, nzl):
    """beat_pde_spmv_dot_part: interior planes (part 0, ghost planes POISONED while it runs) + boundary
    planes (part 1) give the same q and p.q as the one-shot SpMV."""
    from beat import _hip, _stencil
    from beat._device import Field

    ctx = hip_ctx
    nx, ny = 70, 21
    plane, n = nx * ny, nx * ny * nzl
    mt, kt = _stencil.stencil_tables(3, (0.1, 0.1, 0.1), _conductivity("aniso3", 3))
    n3 = (C.c_int64 * 3)(nx, ny, nzl)
    handle = C.c_void_p()
    _hip.check(ctx.lib.beat_pde_create(ctx.handle, n3, lo_phys, hi_phys, mt.ctypes.data_as(C.c_void_p),
                                       kt.ctypes.data_as(C.c_void_p), C.byref(handle)))
    _hip.check(ctx.lib.beat_pde_set_timestep(handle, 0.01, 0.5, 0.05))
    rng = np.random.default_rng(12)
    p, q1, q2 = Field(ctx, n, plane), Field(ctx, n, plane), Field(ctx, n, plane)
    p.set(rng.standard_normal(n))
    glo, ghi = rng.standard_normal(plane), rng.standard_normal(plane)
    p.ghost_lo.copy_(ctx.from_numpy(glo))
    p.ghost_hi.copy_(ctx.from_numpy(ghi))
    st = ctx.zeros(16)
    stp = C.c_void_p(st.data_ptr())
    _hip.check(ctx.lib.beat_pde_spmv_dot(handle, p.ptr, q1.ptr, stp))
    ctx.synchronize()
    pq_whole = float(st[3])
    q2.fill(float("nan"))
    p.ghost_lo.fill_(float("nan"))
    p.ghost_hi.fill_(float("nan"))
    _hip.check(ctx.lib.beat_pde_spmv_dot_part(handle, p.ptr, q2.ptr, stp, 0))
    ctx.synchronize()
    p.ghost_lo.copy_(ctx.from_numpy(glo))
    p.ghost_hi.copy_(ctx.from_numpy(ghi))
    _hip.check(ctx.lib.beat_pde_spmv_dot_part(handle, p.ptr, q2.ptr, stp, 1))
    ctx.synchronize()
    np.testing.assert_array_equal(q2.numpy(), q1.numpy())
    assert np.isclose(float(st[3]), pq_whole, rtol=1e-13)
    _hip.check(ctx.lib.beat_pde_destroy(handle))


@pytest.mark.parametrize("degree", [2, 3, 4])
def test_polynomial_preconditioned_pcg(hip_ctx, degree):
    """Chebyshev-polynomial preconditioned PCG: same solution as the sparse-LU solve (1e-9), fewer
    iterations than Jacobi, and the iteration count of the oracle's restatement with the same coefficients."""
    from beat import _stencil
    from beat._engine import DiffusionSolver, HipOps, Slab, chebyshev_coefficients, spectrum_bounds
    from oracle import fem

    ctx = hip_ctx
    cells, L = (40, 21, 12), (4.0, 2.1, 1.2)
    mesh = fem.BoxMesh(cells, L)
    Mten = _conductivity("aniso3", 3)
    C_m, theta, dt = 0.01, 0.5, 0.05
    nn = tuple(c + 1 for c in cells)
    mt, kt = _stencil.stencil_tables(3, tuple(l / c for l, c in zip(L, cells)), Mten)
    rng = np.random.default_rng(8)
    v_prev = -85.0 + 100.0 / (1.0 + np.exp((np.linalg.norm(mesh.x - 1.0, axis=1) - 0.8) / 0.05))
    v_prev += 0.01 * rng.standard_normal(mesh.num_nodes)
    w = fem.stimulus_weights(mesh, mesh.locate_cells(lambda x: x[0] <= 1.0 + 1e-10))
    amp = 0.357
    model = fem.OracleMonodomainModel(mesh, Mten, [fem.OracleStimulus(lambda t: amp, w)], C_m=C_m, theta=theta,
                                      default_timestep=dt)
    model.state[:] = v_prev
    model.assign_previous()
    model.step((0.0, dt))
    its = {}
    for deg in (1, degree):
        ops = HipOps(ctx, nn, True, True, mt, kt)
        ops.set_preconditioner(deg)
        ops.set_timestep(C_m, theta, dt)
        solver = DiffusionSolver(ops, Slab(nn[2]))
        fv, fx, fw = ops.new_field(), ops.new_field(), ops.new_field()
        fv.set(v_prev)
        fw.set(w)
        res = solver.solve(fv, [fw], [amp], fx, rtol=1e-11, atol=1e-50, max_it=300)
        assert res.converged_reason > 0
        assert np.abs(fx.numpy() - model.state).max() <= 1e-9 * np.abs(model.state).max()
        its[deg] = res.iterations
    assert its[degree] < its[1]
    A = (C_m * fem.assemble_mass(mesh) + theta * dt * fem.assemble_stiffness(mesh, Mten)).tocsr()
    lmin, lmax = spectrum_bounds(C_m * mt + theta * dt * kt)
    coef = chebyshev_coefficients(degree, lmin, lmax)
    np.testing.assert_allclose(coef, fem.chebyshev_coefficients(degree, lmin, lmax), rtol=1e-13)
    _, its_ref, _ = fem.pcg_polynomial(A, model.rhs(theta * dt, dt), v_prev, coef, rtol=1e-11)
    assert abs(its_ref - its[degree]) <= 1, (its_ref, its)


def test_deferred_x_ring_wrap_and_over_enqueue(hip_ctx):
    """Deferred-x PCG bookkeeping: (a) more iterations than the ring holds (wraps, in-loop flush),
    (b) a solve that converges long before the iterations enqueued ahead of time have run (the
    pre-enqueued flushes must stay no-ops): both give exactly what a fresh solver gives."""
    from beat import _stencil
    from beat._engine import DiffusionSolver, HipOps, Slab

    ctx = hip_ctx
    nn = (50, 23, 11)
    mt, kt = _stencil.stencil_tables(3, (0.1, 0.1, 0.1), _conductivity("aniso3", 3))
    rng = np.random.default_rng(21)
    v_hard = rng.standard_normal(nn[0] * nn[1] * nn[2]) * 50.0
    v_easy = -85.0 + 1e-3 * rng.standard_normal(v_hard.size)

    def make():
        ops = HipOps(ctx, nn, True, True, mt, kt)
        ops.set_timestep(0.01, 0.5, 0.5)  # large dt: stiffness matters, many iterations
        return ops, DiffusionSolver(ops, Slab(nn[2]))

    def solve(solver, ops, v, rtol):
        fv, fx = ops.new_field(), ops.new_field()
        fv.set(v)
        res = solver.solve(fv, [], [], fx, rtol=rtol, atol=1e-50, max_it=500)
        return fx.numpy(), res

    ops, solver = make()
    x_hard, r_hard = solve(solver, ops, v_hard, 1e-12)
    assert r_hard.iterations > 13  # wrapped the 6-deep ring at least twice
    x_easy, r_easy = solve(solver, ops, v_easy, 1e-6)  # same handle: r_hard.iterations get enqueued
    assert r_easy.iterations < 6
    ops2, solver2 = make()
    x_ref, r_ref = solve(solver2, ops2, v_easy, 1e-6)
    assert r_ref.iterations == r_easy.iterations
    np.testing.assert_array_equal(x_easy, x_ref)
    # and the hard one against the distributed-style classic recurrences (x updated every iteration)
    ops3 = HipOps(ctx, nn, True, True, mt, kt)
    ops3.set_timestep(0.01, 0.5, 0.5)
    x_cls, r_cls = solve(DiffusionSolver(ops3, Slab(nn[2]), force_distributed=False), ops3, v_hard, 1e-12)
    np.testing.assert_array_equal(x_cls, x_hard)


def test_tp06_step_is_regular_through_the_cal_singularity(hip_ctx):
    """i_CaL of the specification is 0/0 at V = 15 mV and its V-derivative loses all accuracy next to it (the
    literal expression gave |J_V| ~ 1e8 and V = inf at V = 15.000000000027 in a 256^3 run).  The kernel takes
    x/(e^x - 1) from its series inside |V - 15| < 0.13 mV: every state stays finite there, the update is smooth across
    the switch, and outside the window the kernel still agrees with the literal oracle."""
    from beat import _hip
    from beat.models import tp06
    from oracle import ionic

    # the plateau state of the node that blew up (V replaced below)
    base = np.array([0.26252164857130134, 0.01686034782909001, 0.019263565352823808, 0.999298678112656,
                     7.787943035125431e-11, 4.991947762659259e-10, 0.9550340372923384, 0.7192870635966016,
                     0.48840230274567625, 0.4037323643965525, 0.10531142458561057, 0.2803574590153299,
                     0.37626961261077424, 0.0006787249606944496, 2.892319135034567, 0.9153873040549239,
                     8.59497902253472, 15.0, 136.901828032133])
    iv = tp06.state_index("V")
    offsets = np.array([-0.4, -0.2, -0.14, -0.13, -1e-2, -1e-3, -1e-6, -1e-9, -2.7e-11, -1.8e-15, 0.0, 1.8e-15,
                        2.7367e-11, 1e-9, 1e-6, 1e-3, 1e-2, 0.13, 0.14, 0.2, 0.4])
    S = np.repeat(base[:, None], len(offsets), axis=1)
    S[iv] = 15.0 + offsets
    p = tp06.init_parameter_values(stim_amplitude=0.0)
    dt = 0.01
    out = _ode_step(hip_ctx, _hip.MODEL_TP06_GRL1, S, p, 0.0, dt, v_index=iv)
    assert np.isfinite(out).all()
    # outside the window: the literal oracle (same tolerance as the random-state parity test)
    far = np.abs(offsets) > 0.135
    ref = ionic.tp06_generalized_rush_larsen(S[:, far], 0.0, dt, p)
    np.testing.assert_allclose(out[:, far], ref, rtol=1e-9, atol=1e-12)
    # inside the window: the literal specification evaluated with 40 significant digits (mpmath through sympy's
    # lambdify) for the two states the L-type current drives, V and Ca_ss; V = 15 exactly is 0/0 there and is
    # checked against its neighbours instead
    import mpmath
    import sympy

    ys = sympy.symbols(" ".join(ionic.TP06_STATES), real=True)
    ps = sympy.symbols(" ".join("p_" + n for n in ionic.TP06_PARAMETERS), real=True)
    tt = sympy.Symbol("t", real=True)
    fs = ionic.tp06_rhs(ys, tt, ps, ns=ionic._sympy_ns())
    rows = [iv, tp06.state_index("Ca_ss")]
    fn = sympy.lambdify([*ys, tt, *ps], [(fs[k], sympy.diff(fs[k], ys[k])) for k in rows], modules="mpmath")
    mpmath.mp.dps = 40
    try:
        for c, off in enumerate(offsets):
            if off == 0.0:
                continue
            vals = fn(*[mpmath.mpf(float(x)) for x in S[:, c]], mpmath.mpf(0), *[mpmath.mpf(float(x)) for x in p])
            for k, (f, J) in zip(rows, vals):
                exact = float(mpmath.mpf(float(S[k, c])) + f * (mpmath.exp(J * dt) - 1) / J)
                assert abs(out[k, c] - exact) <= 1e-11 * max(abs(exact), 1e-3), (k, off, out[k, c], exact)
    finally:
        mpmath.mp.dps = 15
    mid = list(offsets).index(0.0)
    for k in rows:
        assert abs(out[k, mid] - 0.5 * (out[k, mid - 1] + out[k, mid + 1])) <= 1e-13 * max(abs(out[k, mid]), 1e-3)


def _sweep_shapes():
    """Seeded random grid shapes around every tile boundary of the stencil kernels (tiles are 64 x 16, 128 x 8 or
    256 x 4 nodes, chosen by nx; 16 planes per z-chunk), plus hand-picked edge cases."""
    rng = np.random.default_rng(20260101)
    shapes = [(255, 3, 2), (256, 4, 1), (257, 5, 3), (300, 9, 2), (513, 2, 2), (127, 8, 17), (128, 9, 16), (129, 7, 2),
              (63, 16, 3), (64, 17, 2), (65, 15, 33), (2, 2, 2), (1, 1, 40), (3, 40, 1), (600, 1, 1)]
    for _ in range(12):
        shapes.append((int(rng.integers(1, 330)), int(rng.integers(1, 20)), int(rng.integers(1, 8))))  # <= 50 k nodes
    return shapes


@pytest.mark.parametrize("cells", _sweep_shapes())
def test_operator_and_solve_sweep_over_grid_shapes(hip_ctx, cells):
    """A x and one theta-step on grids whose node counts straddle the tile and chunk sizes of the kernels, against the
    oracle's assembled matrices / sparse solve; then the same operators through the per-node path with a random voxel
    mask."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    from beat import _hip, _stencil
    from beat._device import Field
    from beat._engine import HipOps
    from oracle import fem

    ctx = hip_ctx
    L = tuple(0.1 * c for c in cells)
    mesh = fem.BoxMesh(cells, L)
    Mten = _conductivity("aniso3", 3)
    Mass, K = fem.assemble_mass(mesh), fem.assemble_stiffness(mesh, Mten)
    C_m, theta, dt = 0.01, 0.5, 0.05
    A = (C_m * Mass + theta * dt * K).tocsr()
    B = (C_m * Mass - (1 - theta) * dt * K).tocsr()
    n = mesh.num_nodes
    nn = tuple(c + 1 for c in cells)
    plane = nn[0] * nn[1]
    rng = np.random.default_rng(sum(cells))
    x = rng.standard_normal(n)
    ops = HipOps(ctx, nn, True, True, *_stencil.stencil_tables(3, (0.1, 0.1, 0.1), Mten))
    ops.set_timestep(C_m, theta, dt)
    fx, fy = ops.new_field(), ops.new_field()
    fx.set(x)
    fx.ghost_lo.fill_(float("nan"))
    fx.ghost_hi.fill_(float("nan"))
    ops.apply(0, fx, fy)
    ref = A @ x
    scale = (abs(A) @ np.ones(n)).max() * np.abs(x).max()
    assert np.abs(fy.numpy() - ref).max() <= 1e-13 * scale
    v_prev = -85.0 + 30.0 * rng.random(n)
    fv, fs = ops.new_field(), ops.new_field()
    fv.set(v_prev)
    res = ops.solve_single(fv, [], [], fs, 1e-12, 1e-50, 500)
    exact = spla.spsolve(A.tocsc(), B @ v_prev)
    assert res.converged_reason > 0
    np.testing.assert_allclose(fs.numpy(), exact, rtol=0, atol=1e-9 * np.abs(exact).max())
    # per-node rows on a random voxel mask of the same box
    active = rng.random(int(np.prod(cells))) < 0.6
    if not active.any():
        active[0] = True
    mf, kf = _stencil.stencil_fields(3, cells, (0.1, 0.1, 0.1), Mten, active)
    var = HipOps(ctx, nn, True, True, mf, kf, per_node=True)
    var.set_timestep(C_m, theta, dt)
    act_s = np.repeat(active, 6)  # six tetrahedra per box cell
    Mass_a = fem.assemble_mass(mesh, np.nonzero(act_s)[0])
    K_a = fem.assemble_stiffness(mesh, np.broadcast_to(Mten, (len(act_s), 3, 3)) * act_s[:, None, None])
    tissue = Mass_a.diagonal() > 0
    ident = sp.diags(np.where(tissue, 0.0, 1.0))
    A_a = (C_m * Mass_a + theta * dt * K_a + ident).tocsc()
    B_a = (C_m * Mass_a - (1 - theta) * dt * K_a + ident).tocsr()
    v2 = np.where(tissue, v_prev, 0.0)
    exact2 = spla.spsolve(A_a, B_a @ v2)
    gv, gs = var.new_field(), var.new_field()
    gv.set(v2)
    gs.set(v2)
    res2 = var.solve_single(gv, [], [], gs, 1e-12, 1e-50, 500)
    assert res2.converged_reason > 0
    np.testing.assert_allclose(gs.numpy()[tissue], exact2[tissue], rtol=0, atol=1e-9 * max(1.0, np.abs(exact2).max()))


@pytest.mark.parametrize("cells", [(255, 3), (256, 4), (257, 5), (1023, 1), (63, 17), (64, 16), (65, 15), (1, 1), (2, 300),
                                   (300,), (1,), (64,), (257,)])
def test_operator_and_solve_sweep_2d_1d(hip_ctx, cells):
    """The same sweep for 2-D and 1-D grids (one plane / one row of the 3-D kernels)."""
    import scipy.sparse.linalg as spla

    from beat import _stencil
    from beat._engine import HipOps
    from oracle import fem

    dim = len(cells)
    L = tuple(0.1 * c for c in cells)
    mesh = fem.BoxMesh(cells, L)
    Mten = np.array([[2.0, 0.3], [0.3, 1.0]]) * 1e-3 if dim == 2 else 1e-3
    Mass, K = fem.assemble_mass(mesh), fem.assemble_stiffness(mesh, Mten)
    C_m, theta, dt = 0.01, 0.5, 0.05
    A = (C_m * Mass + theta * dt * K).tocsr()
    B = (C_m * Mass - (1 - theta) * dt * K).tocsr()
    n = mesh.num_nodes
    nn = tuple(c + 1 for c in cells) + (1,) * (3 - dim)
    rng = np.random.default_rng(sum(cells) + dim)
    ops = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_tables(dim, (0.1,) * dim, Mten))
    ops.set_timestep(C_m, theta, dt)
    x = rng.standard_normal(n)
    fx, fy = ops.new_field(), ops.new_field()
    fx.set(x)
    fx.ghost_lo.fill_(float("nan"))
    fx.ghost_hi.fill_(float("nan"))
    ops.apply(0, fx, fy)
    scale = (abs(A) @ np.ones(n)).max() * np.abs(x).max()
    assert np.abs(fy.numpy() - A @ x).max() <= 1e-13 * scale
    v_prev = -85.0 + 30.0 * rng.random(n)
    fv, fs = ops.new_field(), ops.new_field()
    fv.set(v_prev)
    res = ops.solve_single(fv, [], [], fs, 1e-12, 1e-50, 500)
    assert res.converged_reason > 0
    exact = spla.spsolve(A.tocsc(), B @ v_prev)
    np.testing.assert_allclose(fs.numpy(), exact, rtol=0, atol=1e-9 * np.abs(exact).max())


def test_tp06_step_on_edge_case_states(hip_ctx):
    """60 000 states drawn from edge values -- potentials on both sides of every branch and singular point of the
    specification (-40 mV, 15 mV, 0), gates at exactly 0 and 1 and at 1e-300, concentrations over five decades -- and
    three step sizes: the kernel's result is finite everywhere (the literal oracle is not: ~2 % of these columns hit its
    0/0 at 15 mV) and agrees with the oracle to 1e-10 wherever the oracle is finite and away from 15 mV."""
    from beat import _hip
    from oracle import ionic

    rng = np.random.default_rng(99)
    n = 60000
    S = _random_tp06_states(n, 5)
    idx = ionic.tp06_state_index
    S[idx("V")] = rng.choice([-120.0, -100.0, -86.2, -40.0, -40.0 + 1e-12, -39.999999, 0.0, 15.0, 15.0 + 1e-13, 14.99999,
                              35.0, 60.0, 80.0], n) + rng.choice([0.0, 1e-9, -1e-9, 0.3], n)
    for gate in ["Xr1", "Xr2", "Xs", "m", "h", "j", "d", "f", "f2", "fCass", "s", "r", "R_prime"]:
        S[idx(gate)] = rng.choice([0.0, 1.0, 1e-300, 1e-12, 0.5, 1 - 1e-16], n)
    S[idx("Ca_i")] = rng.choice([1e-7, 1e-5, 1e-4, 1e-3, 1e-2], n)
    S[idx("Ca_ss")] = rng.choice([1e-7, 1e-4, 1e-3, 1e-1, 1.0], n)
    S[idx("Ca_SR")] = rng.choice([0.01, 1.0, 4.0, 10.0], n)
    S[idx("Na_i")] = rng.choice([2.0, 8.6, 20.0, 50.0], n)
    S[idx("K_i")] = rng.choice([50.0, 136.9, 160.0], n)
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    for dt in (0.05, 0.01, 0.5):
        out = _ode_step(hip_ctx, _hip.MODEL_TP06_GRL1, S, P, 0.0, dt)
        assert np.isfinite(out).all()
        with np.errstate(all="ignore"):
            ref = ionic.tp06_generalized_rush_larsen(S, 0.0, dt, P)
        ok = np.isfinite(ref).all(axis=0) & (np.abs(S[idx("V")] - 15.0) > 0.2)
        assert ok.mean() > 0.7 and not np.isfinite(ref).all()
        err = np.abs(out[:, ok] - ref[:, ok]) / np.maximum(np.abs(ref[:, ok]), 1e-3)
        assert err.max() < 1e-10, err.max()


@pytest.mark.parametrize("per_node", [False, True])
def test_pcg_degenerate_right_hand_sides(hip_ctx, per_node):
    """Fields for which the initial residual vanishes (constant: K v = 0; zero; 1e-300) return at once with the input
    unchanged, with and without the deferred last update; a field of size 1e150 converges without overflow."""
    from beat import _stencil
    from beat._engine import HipOps

    nn = (33, 17, 9)
    M = np.diag([1e-3, 5e-4, 2e-4])
    rng = np.random.default_rng(0)
    if per_node:
        cells = tuple(n - 1 for n in nn)
        active = rng.random(int(np.prod(cells))) < 0.7
        ops = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_fields(3, cells, (0.1,) * 3, M, active), per_node=True)
    else:
        ops = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_tables(3, (0.1,) * 3, M))
    ops.set_timestep(0.01, 0.5, 0.05)
    n = int(np.prod(nn))
    fv, fx = ops.new_field(), ops.new_field()
    for v in (np.full(n, -85.0), np.zeros(n), np.full(n, 1e-300)):
        fv.set(v)
        for defer in (False, True):
            fx.set(np.full(n, 7.0))
            res = ops.solve_single(fv, [], [], fx, 1e-8, 1e-50, 200, defer_flush=defer)
            ops.flush_pending()
            assert res.iterations == 0 and res.converged_reason > 0
            np.testing.assert_array_equal(fx.numpy(), v)
    fv.set(1e150 * rng.standard_normal(n))
    res = ops.solve_single(fv, [], [], fx, 1e-8, 1e-50, 200)
    assert res.converged_reason > 0 and 0 < res.iterations < 40 and np.isfinite(fx.numpy()).all()


@pytest.mark.parametrize("nn", [(41, 15, 7), (32, 16, 16), (100, 1, 1), (64, 32, 1), (2, 2, 2)])
def test_one_launch_solve_equals_the_multi_launch_solve(hip_ctx, nn):
    """csrc/beat_pde_small.hip (whole solve of a small grid in one workgroup) against the multi-launch kernels on the
    same operator: a sequence of solves with a stimulus and the extrapolated guess -- same iteration counts, solutions
    equal to rounding (the dot products are summed in another order), same recorded history; a solve cut short by
    max_it reports -3 with the same iterate; an atol-dominated stopping test reports reason 3; 8192 nodes is the
    largest grid taken (16 per thread), one more node goes to the multi-launch path."""
    import ctypes as C

    from beat import _hip, _stencil
    from beat._engine import HipOps

    dim = 3 - sum(1 for v in nn[1:] if v == 1) if nn != (2, 2, 2) else 3
    n = int(np.prod(nn))
    M = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.1], [0.0, 0.1, 0.5]])[:dim, :dim] * 1e-3
    rng = np.random.default_rng(n)
    w = rng.random(n) * 1e-3
    noise = 0.01 * rng.random(n)
    xs = np.arange(n) % nn[0]
    out = {}
    for small in (True, False):
        ops = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_tables(dim, (0.1,) * dim, M))
        ops.set_small(small)
        ops.set_guess_order(3)
        ops.set_timestep(0.01, 0.5, 0.05)
        fv, fw, fx = ops.new_field(), ops.new_field(), ops.new_field()
        fw.set(w)
        rec = []
        for step in range(5):
            fv.set(-85.0 + 60.0 * np.exp(-((xs - 3.0 - 0.4 * step) ** 2) / 8.0) + noise * (step == 0))
            res = ops.solve_single(fv, [fw], [0.7 if step < 3 else 0.0], fx, 1e-11, 1e-50, 500, defer_flush=bool(step % 2))
            ops.flush_pending()
            rec.append((res.iterations, res.converged_reason, fx.numpy().copy(), res.residual_norm, res.rhs_norm))
        h0, cnt = C.c_void_p(), C.c_int()
        _hip.check(ops.lib.beat_pde_guess_history(ops.handle, C.byref(h0), None, C.byref(cnt)))
        d = hip_ctx.torch.empty(n, dtype=hip_ctx.torch.float64, device=hip_ctx.device)
        _hip.check(ops.lib.beat_copy(hip_ctx.handle, C.c_void_p(d.data_ptr()), h0, n))
        cut = ops.solve_single(fv, [fw], [0.3], fx, 1e-14, 1e-50, 2)
        x_cut = fx.numpy().copy()
        ops.guess_reset()
        loose = ops.solve_single(fv, [fw], [0.3], fx, 1e-30, 1e-6, 500)
        out[small] = (rec, d.cpu().numpy(), cnt.value, cut, x_cut, loose)
    (ra, da, ca, cuta, xa, la), (rb, db, cb, cutb, xb, lb) = out[True], out[False]
    for (ia, qa, va, rna, bna), (ib, qb, vb, rnb, bnb) in zip(ra, rb):
        assert qa > 0 and qb > 0 and abs(ia - ib) <= 1
        np.testing.assert_allclose(va, vb, rtol=0, atol=1e-9 * np.abs(vb).max())
        assert np.isclose(bna, bnb, rtol=1e-12)
    assert ca == cb == 4
    np.testing.assert_allclose(da, db, rtol=0, atol=1e-9 * 85.0)
    assert cuta.converged_reason == cutb.converged_reason == -3 and cuta.iterations == cutb.iterations == 2
    np.testing.assert_allclose(xa, xb, rtol=0, atol=1e-9 * np.abs(xb).max())
    assert la.converged_reason == lb.converged_reason == 3


def test_one_launch_solve_size_limit(hip_ctx):
    """8192 nodes are solved in one launch, 8193 are not (observable: a deferring solve leaves its update pending only
    on the multi-launch path).  The row of 8193 nodes is turned away by its LDS request (a 1-D grid needs about 5 n doubles:
    8192 x 1 x 1 would be, too); 2 x 2 x 2048 and 2 x 2 x 2049, whose LDS request is small, meet the node count itself."""
    from beat import _stencil
    from beat._engine import HipOps

    for nn, one_launch in (((32, 16, 16), True), ((8193, 1, 1), False), ((2, 2, 2048), True), ((2, 2, 2049), False)):
        dim = 3 if nn[1] > 1 else 1
        ops = HipOps(hip_ctx, nn, True, True, *_stencil.stencil_tables(dim, (0.1,) * dim, 1e-3))
        ops.set_small(True)
        assert ops.small_active() == one_launch, nn
        ops.set_timestep(0.01, 0.5, 0.05)
        fv, fx = ops.new_field(), ops.new_field()
        fv.set(-85.0 + 50.0 * np.exp(-((np.arange(int(np.prod(nn))) % nn[0] - 5.0) ** 2) / 9.0))
        res = ops.solve_single(fv, [], [], fx, 1e-8, 1e-50, 500, defer_flush=True)
        assert res.converged_reason > 0 and res.iterations % 6 != 0, res
        assert (ops.pending is None) == one_launch
        ops.flush_pending()
