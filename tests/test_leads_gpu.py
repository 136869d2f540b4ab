"""ECG lead traces on the device (csrc/beat_leads.hip: beat_field_leads; beat.ecg.LeadRecorder): the kernel against math.fsum
with the worst-case bound of any summation order, its two bitwise properties and its refusals; the recorder against the oracle's
sparse LU, against ``ECGRecovery.solve`` + ``assemble_scalar`` (what the reference does per sample, src/beat/ecg.py:282-298) on
the meshes of test_api_gpu.test_ecg_recovery, and over a time loop of a TP06 slab."""
import ctypes as C
import functools
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -53
MAX_LEADS = 16
SENTINEL = -7.25e11
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 600_001)
NLEADS = (1, 2, 3, 8, 9, 16)
OFFSETS = (0, 1, 7)
RTOL = 1e-7  # test_ecg_recovery's figure for a recovery at ksp_rtol 1e-12


def _gamma(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def _case(n):
    """Random v in [-90, 40], 16 random rows with both signs, and per row the fsum of the products and gamma_n sum |q_i v_i|.
    Made once per size; nothing changes it afterwards."""
    rng = np.random.default_rng(1000 + n)
    v = rng.uniform(-90.0, 40.0, n)
    Q = rng.uniform(-1.0, 1.0, (MAX_LEADS, n)) * np.exp(rng.uniform(-3.0, 3.0, (MAX_LEADS, n)))
    assert n < 63 or ((Q > 0).any(axis=1).all() and (Q < 0).any(axis=1).all())
    prod = Q * v
    ref = np.array([math.fsum(row) for row in prod])
    bound = _gamma(n) * np.array([math.fsum(row) for row in np.abs(prod)])
    for a in (v, Q, ref, bound):
        a.setflags(write=False)
    return v, Q, ref, bound


def _leads(ctx, v_ptr, n, q_ptr, ldq, nleads, out_ptr):
    return ctx.lib.beat_field_leads(ctx.handle, C.c_void_p(v_ptr), n, C.c_void_p(q_ptr), ldq, nleads, C.c_void_p(out_ptr))


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_fsum(hip_ctx, n):
    """beat_field_leads on n nodes for nleads in {1, 2, 3, 8, 9, 16}, v at 0, 1 and 7 doubles past a 512-byte boundary of a larger
    allocation that holds NaN everywhere else, rows ldq = n rounded up to 64 and ldq = n + 5 apart (these rows start 3 doubles into
    their allocation) with NaN in every padding entry: |out - fsum| <= gamma_n sum |q_i v_i|, gamma_n = n u / (1 - n u), u = 2^-53
    -- the bound of recursive summation in ANY order (Higham, Accuracy and Stability, 4.2) with n roundings; the kernel makes one
    rounding per fma and fewer than n additions on any path to a result, the reference one rounding per product.  Entries of out
    past nleads keep their sentinel; a second call gives the same bits; out[l] is the same for every nleads > l; and each row of
    the nleads = 9 call equals the call with that row alone."""
    import torch

    from beat import _hip

    ctx = hip_ctx
    v, Q, ref, bound = _case(n)
    vbuf = torch.full((64 + n + 64 + 8,), float("nan"), dtype=torch.float64, device=ctx.device)
    out = torch.empty(MAX_LEADS + 2, dtype=torch.float64, device=ctx.device)
    worst = 0.0
    for ldq, lead in (((n + 63) // 64 * 64, 0), (n + 5, 3)):
        qhost = np.full(lead + MAX_LEADS * ldq, np.nan)
        qhost[lead:].reshape(MAX_LEADS, ldq)[:, :n] = Q
        qdev = ctx.from_numpy(qhost)
        q_ptr = qdev.data_ptr() + 8 * lead
        for off in OFFSETS:
            vbuf.fill_(float("nan"))
            vbuf[64 + off : 64 + off + n].copy_(torch.from_numpy(np.array(v)))
            v_ptr = vbuf.data_ptr() + 8 * (64 + off)
            assert v_ptr % 512 == 8 * off
            first = {}
            for nleads in NLEADS:
                out.fill_(SENTINEL)
                _hip.check(_leads(ctx, v_ptr, n, q_ptr, ldq, nleads, out.data_ptr() + 8))
                got = out.cpu().numpy()
                assert (got[[0, -1]] == SENTINEL).all() and (got[1 + nleads : -1] == SENTINEL).all(), (n, ldq, off, nleads)
                got = got[1 : 1 + nleads].copy()
                assert not np.isnan(got).any(), (n, ldq, off, nleads, got)
                err = np.abs(got - ref[:nleads])
                worst = max(worst, float((err / bound[:nleads]).max()))
                assert (err <= bound[:nleads]).all(), (n, ldq, off, nleads, err, bound[:nleads])
                out.fill_(SENTINEL)
                _hip.check(_leads(ctx, v_ptr, n, q_ptr, ldq, nleads, out.data_ptr() + 8))
                np.testing.assert_array_equal(out.cpu().numpy()[1 : 1 + nleads], got, err_msg="two calls, same input")
                for l in range(nleads):  # the row's bits do not depend on the company it is in
                    assert first.setdefault(l, got[l]) == got[l], (n, ldq, off, nleads, l)
            for l in range(9):
                out.fill_(SENTINEL)
                _hip.check(_leads(ctx, v_ptr, n, q_ptr + 8 * l * ldq, ldq, 1, out.data_ptr() + 8))
                alone = out.cpu().numpy()
                assert alone[1] == first[l] and (alone[2:] == SENTINEL).all(), (n, ldq, off, l)
    print(f"n = {n}: largest |out - fsum| / bound = {worst:.3e}")


def test_refused_arguments(hip_ctx):
    """Every EINVAL case returns -1 and leaves dev_out alone: null pointers, n <= 0, nleads outside 1..16, ldq < n, pointers that
    are not 8-byte aligned."""
    import torch

    ctx = hip_ctx
    n, ldq = 300, 320
    v = torch.ones(n + 8, dtype=torch.float64, device=ctx.device)
    q = torch.ones(17 * ldq + 8, dtype=torch.float64, device=ctx.device)
    out = torch.full((MAX_LEADS + 2,), SENTINEL, dtype=torch.float64, device=ctx.device)
    vp, qp, op = v.data_ptr(), q.data_ptr(), out.data_ptr()
    lib, h = ctx.lib, ctx.handle
    bad = [
        (None, vp, n, qp, ldq, 2, op), (h, None, n, qp, ldq, 2, op), (h, vp, n, None, ldq, 2, op), (h, vp, n, qp, ldq, 2, None),
        (h, vp, 0, qp, ldq, 2, op), (h, vp, -5, qp, ldq, 2, op), (h, vp, n, qp, ldq, 0, op), (h, vp, n, qp, ldq, -1, op),
        (h, vp, n, qp, ldq, MAX_LEADS + 1, op), (h, vp, n, qp, n - 1, 2, op), (h, vp + 4, n, qp, ldq, 2, op),
        (h, vp, n, qp + 4, ldq, 2, op), (h, vp, n, qp, ldq, 2, op + 4),
    ]
    for args in bad:
        assert lib.beat_field_leads(*args) == -1, args
        assert lib.beat_last_error()
    ctx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert lib.beat_field_leads(h, vp, n, qp, ldq, MAX_LEADS, op) == 0  # (the accepted call next to them)
    np.testing.assert_array_equal(out.cpu().numpy()[:MAX_LEADS], float(n))


# ---- the recorder -------------------------------------------------------------------------------------------------------------
BOX_CELLS, BOX_L = (8, 6, 5), (2.0, 1.5, 1.0)
BOX_M = np.array([[2.0e-3, 3.0e-4, 0.0], [3.0e-4, 1.0e-3, 0.0], [0.0, 0.0, 5.0e-4]])
# nine electrodes around the 2 x 1.5 x 1 box, none on a plane through its centre (1, 0.75, 0.5) or through the bump of v
BOX_ELECTRODES = {"RA": (-0.7, 1.9, 1.3), "LA": (2.8, 2.1, 1.2), "LL": (2.4, -0.9, -0.6), "V1": (0.3, -0.5, 1.6), "V2": (0.7, -0.6, 1.7),
                  "V3": (1.2, -0.7, 1.5), "V4": (1.6, -0.6, 1.4), "V5": (2.5, -0.4, 0.9), "V6": (2.9, 0.2, 0.7)}


def _box_potential(x):
    return -80.0 + 100.0 * np.exp(-((x[0] - 0.6) ** 2 + (x[1] - 0.5) ** 2 + (x[2] - 0.4) ** 2) / 0.2)


def _solve_and_assemble(ecg, forms):
    import beat

    ecg.solve()
    return np.array([beat.ecg.assemble_scalar(f) for f in forms])


def _assert_rows_close(got, want, what):
    rel = np.abs(got - want) / np.abs(want)
    print(f"{what}: largest relative difference {float(rel.max()):.3e}; smallest |lead| {float(np.abs(want).min()):.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.0, err_msg=what)


def test_recorder_against_the_oracle_and_the_recovery():
    """The 8 x 6 x 5 box of test_ecg_recovery (anisotropic tensor, C_m = 0.01, sigma_b = 2), nine electrodes: every recorded lead
    equals w . spsolve(-C_m Mass, K v) of the oracle (fem.assemble_mass / assemble_stiffness / load_vector) and ecg.solve() +
    assemble_scalar on the same state to 1e-7 relative, for two states; leads12() is Leads12 of the columns; lead_field(name) dotted
    with v on the host is the recorded value within the kernel's bound gamma_n sum |q_i v_i|; 17 electrodes are refused."""
    import scipy.sparse.linalg as spla

    import beat
    from beat import grid as g
    from oracle import fem

    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(BOX_L)], list(BOX_CELLS))
    v = g.Function(g.functionspace(mesh, ("P", 1)))
    v.interpolate(_box_potential)
    ecg = beat.ECGRecovery(v=v, M=BOX_M, C_m=0.01, sigma_b=2.0, petsc_options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    rec = beat.LeadRecorder(ecg, BOX_ELECTRODES)
    assert rec.names == tuple(BOX_ELECTRODES) and len(rec) == 0 and rec.values().shape == (0, 9)
    forms = [ecg.eval(p) for p in BOX_ELECTRODES.values()]
    omesh = fem.BoxMesh(BOX_CELLS, BOX_L)
    lu = spla.splu((-0.01 * fem.assemble_mass(omesh)).tocsc())
    K = fem.assemble_stiffness(omesh, BOX_M)
    W = np.array([fem.load_vector(omesh, lambda x, p=p: 1.0 / (4 * np.pi * 2.0) / np.sqrt(sum((x[a] - p[a]) ** 2 for a in range(3))))
                  for p in BOX_ELECTRODES.values()])
    states = []
    for k in range(2):
        if k == 1:
            v.interpolate(lambda x: 20.0 - 95.0 / (1.0 + np.exp(-(1.5 * x[0] + 0.8 * x[1] - 0.6 * x[2] - 1.7) / 0.15)))
        states.append(np.asarray(v.x.array).copy())
        rec.record()
        got = rec.values()[k]
        assert len(rec) == k + 1
        _assert_rows_close(got, W @ lu.solve(K @ states[k]), f"state {k}, oracle")
        _assert_rows_close(got, _solve_and_assemble(ecg, forms), f"state {k}, ecg.solve + assemble_scalar")
    vals = rec.values()
    np.testing.assert_array_equal(rec.signal("V3"), vals[:, 5])
    l12 = rec.leads12()
    by_hand = beat.ecg.Leads12(RA=vals[:, 0], LA=vals[:, 1], LL=vals[:, 2], V1=vals[:, 3], V2=vals[:, 4], V3=vals[:, 5], V4=vals[:, 6],
                               V5=vals[:, 7], V6=vals[:, 8])
    assert l12.RL is None
    for name in ("RA", "LA", "LL", "V1", "V6", "I", "II", "III", "aVR", "aVL", "aVF", "V1_", "V4_"):
        np.testing.assert_array_equal(getattr(l12, name), getattr(by_hand, name), err_msg=name)
    n = mesh.num_nodes
    for col, name in enumerate(BOX_ELECTRODES):
        q = np.asarray(rec.lead_field(name).x.array)
        assert q.shape == (n,)
        prod = q * states[1]
        err, bound = abs(math.fsum(prod) - vals[1, col]), _gamma(n) * math.fsum(np.abs(prod))
        assert err <= bound, (name, err, bound)
    with pytest.raises(ValueError):
        beat.LeadRecorder(ecg, [(3.0 + 0.1 * k, 0.5, 0.5) for k in range(MAX_LEADS + 1)])
    seq = beat.LeadRecorder(ecg, [BOX_ELECTRODES["RA"], BOX_ELECTRODES["V1"]])
    assert seq.names == ("0", "1")
    seq.record()
    np.testing.assert_array_equal(seq.values()[0], vals[1, [0, 3]])  # a row does not depend on the other rows of its recorder


def test_recorder_on_the_unit_square():
    """The 2-D mesh of test_ecg_recovery (5 x 5 unit square, v = (x - 0.5)^2, M = C_m = sigma_b = 1) with electrodes off its
    symmetry line: the recorded leads equal ecg.solve() + assemble_scalar to 1e-7."""
    import beat
    from beat import grid as g

    mesh = g.create_unit_square(g.COMM_WORLD, 5, 5, g.CellType.triangle)
    V = g.functionspace(mesh, ("P", 1))
    v = g.Function(V)
    X = g.SpatialCoordinate(mesh)
    v.interpolate(g.Expression((X[0] - 0.5) ** 2, beat.utils.interpolation_points(V)))
    ecg = beat.ECGRecovery(v=v, M=1.0, C_m=1.0, sigma_b=1.0, petsc_options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    points = [(1.5, 0.3), (-0.4, 0.8), (0.2, 1.6)]
    rec = beat.LeadRecorder(ecg, points)
    rec.record()
    _assert_rows_close(rec.values()[0], _solve_and_assemble(ecg, [ecg.eval(p) for p in points]), "unit square")


def test_recorder_with_a_fibre_field_per_cell():
    """A box whose conductivity comes from a fibre direction per cell: the operator is per-node rows (beat_pde_create_var), the route
    of voxel geometries.  Recorded leads against ecg.solve() + assemble_scalar, 1e-7."""
    import beat
    from beat import grid as g

    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(BOX_L)], list(BOX_CELLS))
    c = g.cell_centers(mesh)
    ang = 0.9 * c[:, 0] + 0.5 * c[:, 2]
    f0 = np.stack([np.cos(ang), np.sin(ang), 0.2 * np.ones(len(c))], axis=1)
    f0 /= np.linalg.norm(f0, axis=1, keepdims=True)
    M = beat.conductivities.define_conductivity_tensor(f0=g.CellField(mesh, f0), **beat.conductivities.default_conductivities("Bishop"))
    v = g.Function(g.functionspace(mesh, ("P", 1)))
    v.interpolate(_box_potential)
    ecg = beat.ECGRecovery(v=v, M=M, C_m=0.01, sigma_b=2.0, petsc_options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    assert ecg._ops.per_node
    rec = beat.LeadRecorder(ecg, BOX_ELECTRODES)
    rec.record()
    _assert_rows_close(rec.values()[0], _solve_and_assemble(ecg, [ecg.eval(p) for p in BOX_ELECTRODES.values()]), "per-cell fibres")


def test_recorder_on_a_voxel_mask():
    """An ellipsoid voxelised on a 10 x 8 x 6 box (per-node rows assembled on the device from the mask).  ECGRecovery takes such a
    mesh as it takes any other (nodes outside the tissue carry identity rows and keep a zero current: the case "accepts" of the two
    the recorder could meet), so the recorder does too: its leads equal ecg.solve() + assemble_scalar to 1e-7, and the lead fields are
    zero outside the tissue."""
    import beat
    from beat import grid as g

    n, h = (10, 8, 6), 0.25
    ax = [(np.arange(c) + 0.5) * h for c in n]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    mask = ((X - 1.2) ** 2 / 1.3 ** 2 + (Y - 1.0) ** 2 / 0.9 ** 2 + (Z - 0.7) ** 2 / 0.7 ** 2) < 1.0
    assert 0.2 < mask.mean() < 0.7
    mesh = g.create_voxel_mesh(g.COMM_WORLD, mask, h)
    active = mesh.node_active()
    xyz = mesh.node_coordinates(pad3=True)
    v = g.Function(g.functionspace(mesh, ("P", 1)))
    v.x.array[:] = np.where(active, _box_potential((xyz[:, 0] * 0.8, xyz[:, 1] * 0.75, xyz[:, 2] * 0.7)), 0.0)
    ecg = beat.ECGRecovery(v=v, M=BOX_M, C_m=0.01, sigma_b=2.0, petsc_options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    assert ecg._ops.per_node
    points = {"a": (3.4, 0.4, 1.9), "b": (-0.9, 2.6, 1.7), "c": (1.9, -1.1, -0.8)}
    rec = beat.LeadRecorder(ecg, points)
    rec.record()
    _assert_rows_close(rec.values()[0], _solve_and_assemble(ecg, [ecg.eval(p) for p in points.values()]), "voxel mask")
    q = np.asarray(rec.lead_field("b").x.array)
    assert np.all(q[~active] == 0.0) and np.abs(q[active]).max() > 0.0


# ---- a time loop --------------------------------------------------------------------------------------------------------------
SLAB_ELECTRODES = {"RA": (-4.0, 7.5, 4.0), "LA": (14.5, 8.0, 3.5), "LL": (13.0, -3.5, -2.5), "V1": (2.2, -2.0, 5.0)}


def _tp06_slab():
    """The slab of demos/slab_ecg.py at dx = 0.5: 21 x 11 x 5 nodes, a corner stimulus from t = 0."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=10.0, Ly=5.0, Lz=2.0, dx=0.5)
    mesh = geo.mesh
    cond = beat.conductivities.default_conductivities("Niederer")
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
    time = g.Constant(mesh, 0.0)
    cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 1.5 + 1e-10) & (x[1] <= 1.5 + 1e-10))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1, mesh_unit="mm",
                                           amplitude=50_000.0, duration=2.0)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ)
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinODESolver(
        v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen, init_states=ic,
        parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(ic), v_index=tp06.state_index("V"))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    assert pde.state.x.array.size == 21 * 11 * 5
    ecg = beat.ECGRecovery(v=pde.state, sigma_b=1.0, C_m=C_m, M=M, petsc_options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    return solver, ecg


def test_time_loop_equals_the_recovery_after_every_step():
    """TP06 on 21 x 11 x 5 nodes, 20 steps of 0.05 ms: solve(..., recorder=[events, leads]) against a step() loop that calls
    ecg.solve() and assemble_scalar per electrode after every step, row by row to 1e-7; the same run with capacity = 8 (two
    read-backs in mid-run) gives the same array bit for bit.  (21 x 11 x 5 nodes are solved in one launch: nothing is pending on the
    operator when the recorder reads the potential.)"""
    import beat

    dt, nsteps = 0.05, 20
    a, ecg_a = _tp06_slab()
    rec = beat.LeadRecorder(ecg_a, SLAB_ELECTRODES)
    events = beat.EventRecorder(a.pde.state, -40.0)
    assert not a._can_batch(rec)
    a.solve((0.0, nsteps * dt), dt, recorder=[events, rec])
    assert len(rec) == nsteps
    got = rec.values()
    assert got.shape == (nsteps, len(SLAB_ELECTRODES)) and np.isfinite(got).all()

    b, ecg_b = _tp06_slab()
    forms = [ecg_b.eval(p) for p in SLAB_ELECTRODES.values()]
    want = np.zeros_like(got)
    for k in range(nsteps):
        b.step((k * dt, (k + 1) * dt))
        want[k] = _solve_and_assemble(ecg_b, forms)
    print("largest difference of the final potentials:", float(np.abs(np.asarray(a.pde.state.x.array) - np.asarray(b.pde.state.x.array)).max()))
    for k in range(nsteps):
        print(f"step {k + 1}: leads {want[k]}, relative difference {np.abs(got[k] - want[k]) / np.abs(want[k])}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.0)

    c, ecg_c = _tp06_slab()
    small = beat.LeadRecorder(ecg_c, SLAB_ELECTRODES, capacity=8)
    c.solve((0.0, nsteps * dt), dt, recorder=[beat.EventRecorder(c.pde.state, -40.0), small])
    assert len(small) == nsteps and len(small._done) == 2
    np.testing.assert_array_equal(small.values(), got)


def test_demo_runs_at_a_reduced_size(capsys):
    """demos/ecg_leads.py --dx 0.5 --T 6: finite traces of every step, a lead that is not zero."""
    demos = ROOT / "demos"
    sys.path.insert(0, str(demos))
    try:
        spec = importlib.util.spec_from_file_location("demo_ecg_leads", demos / "ecg_leads.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(str(demos))
    leads, values = mod.main(["--dx", "0.5", "--T", "6"])
    assert values.shape == (120, 9) and np.isfinite(values).all()
    for name in ("I", "II", "V1_"):
        trace = getattr(leads, name)
        assert trace.shape == (120,) and np.isfinite(trace).all() and np.abs(trace).max() > 1e-4, name
    assert "lead I" in capsys.readouterr().out
