"""GPU: rule-based fibres.  The kernel through the C ABI against tests/_fibres_ref.py on the inputs the CPU test holds the header to; the
public API on a slab against its closed form; the operators built from device-resident tensors against those built from their host
copy, bit for bit; one split step on a small shell with generated fibres."""
import ctypes as C
import math

import numpy as np
import pytest

import _fibres_ref as ref

pytestmark = pytest.mark.gpu


def _call(ctx, c, want_frame, want_tensor):
    """beat_fibres_rule on the case ``c``; outputs that are not wanted are passed as NULL.  Every output starts as NaN."""
    from beat import _hip

    torch = ctx.torch
    nvox = int(np.prod(c.cells))
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device)  # noqa: E731
    f, s, n = (new(nvox, 3) if want_frame else None for _ in range(3))
    M = new(nvox, 9) if want_tensor else None
    count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    phi = ctx.from_numpy(c.phi.copy())  # (the shared inputs are read-only: torch wants a writable buffer)
    psi = None if c.psi is None else ctx.from_numpy(c.psi.copy())
    active = None if c.active is None else ctx.from_numpy(c.active.astype(np.uint8))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rad = [math.radians(a) for a in ref.ANGLES]
    _hip.check(ctx.lib.beat_fibres_rule(ctx.handle, (C.c_int64 * 3)(*c.cells), (C.c_double * 3)(*c.h), ptr(phi), ptr(psi),
                                        None if c.axis is None else (C.c_double * 3)(*c.axis), ptr(active), *rad, ref.S_L, ref.S_T,
                                        ptr(f), ptr(s), ptr(n), ptr(M), ptr(count)))
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return host(f), host(s), host(n), None if M is None else host(M).reshape(nvox, 3, 3), int(count.item())


@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_kernel_against_reference(hip_ctx, case):
    """All outputs at once, then only dev_M with the others NULL: f, s, n within 1e-12 per component, the tensor within
    1e-12 max(|s_l|, |s_t|), the same degenerate count, zeros on the inactive voxels."""
    c = ref.case(*case)
    ref.assert_well_conditioned(c.ref)
    f, s, n, M, count = _call(hip_ctx, c, True, True)
    worst = max(np.abs(got - getattr(c.ref, k)).max() for k, got in (("f", f), ("s", s), ("n", n)))
    tensor = np.abs(M - c.ref.M).max() / max(abs(ref.S_L), abs(ref.S_T))
    print(f"kernel vs reference on {case}: max |f, s, n difference| = {worst:.3e}, tensor {tensor:.3e} (relative to max(s_l, s_t))")
    assert count == c.ref.count
    assert worst <= ref.TOL
    assert tensor <= ref.TOL
    if c.active is not None:
        assert not f[~c.active].any() and not s[~c.active].any() and not n[~c.active].any() and not M[~c.active].any()
    _, _, _, M_only, count_only = _call(hip_ctx, c, False, True)
    assert count_only == count and np.array_equal(M_only, M)


def test_kernel_counts_degenerate_voxels(hip_ctx):
    """phi constant over every voxel, with a mask: zeros, the isotropic tensor, and only the active voxels counted."""
    base = ref.case((130, 3, 3), False, True)
    phi = np.full_like(base.phi, 0.5)
    c = type(base)(**{**vars(base), "phi": phi})
    f, s, n, M, count = _call(hip_ctx, c, True, True)
    assert count == int(base.active.sum())
    assert not f.any() and not s.any() and not n.any()
    assert np.array_equal(M[base.active], np.broadcast_to(ref.S_T * np.eye(3), (count, 3, 3))) and not M[~base.active].any()


def test_entry_point_refuses(hip_ctx):
    """BEAT_EINVAL before anything is enqueued."""
    ctx = hip_ctx
    torch = ctx.torch
    buf = torch.zeros(64, dtype=torch.float64, device=ctx.device)
    count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    p, q = C.c_void_p(buf.data_ptr()), C.c_void_p(count.data_ptr())
    cells, h, axis = (C.c_int64 * 3)(1, 1, 1), (C.c_double * 3)(1.0, 1.0, 1.0), (C.c_double * 3)(0.0, 0.0, 1.0)
    angles = (1.0, -1.0, 0.0, 0.0, 1.0, 1.0)
    call = ctx.lib.beat_fibres_rule
    assert call(ctx.handle, cells, h, p, None, axis, None, *angles, p, None, None, None, q) == 0  # (the accepted call next to them)
    assert call(ctx.handle, cells, h, None, None, axis, None, *angles, p, None, None, None, q) == -1
    assert call(ctx.handle, cells, h, p, None, None, None, *angles, p, None, None, None, q) == -1
    assert call(ctx.handle, cells, h, p, None, axis, None, *angles, None, None, None, None, q) == -1
    assert call(ctx.handle, cells, h, p, None, axis, None, *angles, p, None, None, None, None) == -1
    assert call(ctx.handle, (C.c_int64 * 3)(1, 0, 1), h, p, None, axis, None, *angles, p, None, None, None, q) == -1
    assert call(ctx.handle, cells, (C.c_double * 3)(1.0, 0.0, 1.0), p, None, axis, None, *angles, p, None, None, None, q) == -1
    assert call(ctx.handle, cells, h, C.c_void_p(buf.data_ptr() + 4), None, axis, None, *angles, p, None, None, None, q) == -1
    ctx.synchronize()
    assert int(count.item()) == 1  # the accepted call's one voxel (phi = 0 at its corners: degenerate); the refused ones counted nothing


# ---- the public API ---------------------------------------------------------------------------------------------------------------

def _slab():
    from beat import grid as g

    cells, L = (8, 4, 4), (2.0, 1.0, 1.0)
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(L)], list(cells))
    faces = {1: lambda x: np.isclose(x[0], 0.0), 2: lambda x: np.isclose(x[0], L[0]),
             3: lambda x: np.isclose(x[2], L[2]), 4: lambda x: np.isclose(x[2], 0.0)}
    ids = {k: g.locate_entities_boundary(mesh, 2, fn) for k, fn in faces.items()}
    ft = g.meshtags(mesh, 2, np.concatenate(list(ids.values())), np.concatenate([np.full(len(v), k) for k, v in ids.items()]))
    return mesh, g.functionspace(mesh, ("P", 1)), ft, ids[4]


@pytest.mark.parametrize("longitudinal", ["axis", "base and apex facets"])
def test_slab_through_the_public_api(hip_ctx, longitudinal):
    """lv_rule_based on the (8, 4, 4) box, endocardium x = 0, epicardium x = Lx: every f0 within 1e-5 of (0, cos alpha, sin alpha),
    alpha linear in the voxel's x.  (The Laplace PCG stops at rtol 1e-10 on a grid of condition < 100: phi is good to ~1e-8, the
    direction to ~1e-7.)  Seen on an MI355X, worst of f0, s0, n0: 2.7e-10 with the axis, 4.1e-10 with psi from the base / apex facets."""
    import beat
    from beat import grid as g

    mesh, V, ft, apex = _slab()
    kw = {"long_axis": (0.0, 0.0, 1.0)} if longitudinal == "axis" else {"base_marker": 3, "apex_facets": apex}
    ms = beat.fibres.lv_rule_based(V, ft, 1, 2, alpha_endo=60.0, alpha_epi=-60.0, **kw)
    assert isinstance(ms.f0, g.DeviceCellField) and ms.f0.device_values.is_cuda and ms.degenerate == 0
    phic = np.tile((np.arange(8) + 0.5) / 8, 16)
    alpha = np.deg2rad(60.0 * (1.0 - phic) - 60.0 * phic)
    zero = np.zeros_like(alpha)
    want = {"f0": np.stack([zero, np.cos(alpha), np.sin(alpha)], axis=1), "s0": np.stack([zero + 1.0, zero, zero], axis=1),
            "n0": np.stack([zero, -np.sin(alpha), np.cos(alpha)], axis=1)}
    for name, w in want.items():
        err = np.abs(getattr(ms, name).values - w).max()
        print(f"slab, longitudinal = {longitudinal}: max |{name} - closed form| = {err:.3e}")
        assert err <= 1e-5, name


def _shell_mesh(n=16, h=0.25):
    """A truncated spherical shell as a voxel mask, its inner (10) and outer (20) staircase surface tagged by the facet centre."""
    from beat import grid as g

    ax = (np.arange(n) + 0.5) * h - n * h / 2.0
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    r = np.sqrt(X**2 + Y**2 + Z**2)
    ro, ri = 0.48 * n * h, 0.30 * n * h
    mesh = g.create_voxel_mesh(g.COMM_WORLD, (r < ro) & (r > ri) & (Z < 0.3 * n * h), h)
    facets = mesh.exterior_facets()
    xyz = g._node_xyz(mesh, mesh.facet_vertices(facets).ravel()).reshape(len(facets), 4, 3)
    ctr = xyz.mean(axis=1) - n * h / 2.0
    rc = np.linalg.norm(ctr, axis=1)
    top = (np.ptp(xyz[:, :, 2], axis=1) < 1e-12) & (ctr[:, 2] > ctr[:, 2].max() - 1e-9)
    keep = ~top
    ft = g.meshtags(mesh, 2, facets[keep], np.where(rc[keep] < 0.5 * (ro + ri), 10, 20).astype(np.int32))
    return mesh, g.functionspace(mesh, ("P", 1)), ft


@pytest.mark.parametrize("masked", [True, False], ids=["shell", "full box"])
def test_device_path_equals_host_path(hip_ctx, masked):
    """The (15, n) mass and stiffness rows of the operators built from the device-resident tensors are bit for bit those built from
    ``M.values``, the host copy of the same numbers; and the device route fetched no host copy on its way."""
    import torch

    from beat import conductivities, fibres
    from beat import grid as g
    from beat._engine import build_ops, conductivity_array

    if masked:
        mesh, V, _ = _shell_mesh()
    else:
        mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([1.1, 0.9, 0.7])], [11, 9, 7])
        V = g.functionspace(mesh, ("P", 1))
    x = mesh.node_coordinates(pad3=True)
    centre = 0.5 * (np.array(mesh.lower) + np.array(mesh.upper))
    phi = g.Function(V)
    phi.x.array[:] = np.linalg.norm(x - centre, axis=1) / np.linalg.norm(np.array(mesh.upper) - centre)
    ms = fibres.rule_based(mesh, phi, (0.1, -0.2, 1.0))
    M = conductivities.conductivity_tensor(ref.S_L, ref.S_T, ms.f0)
    assert isinstance(M, g.DeviceCellField) and tuple(M.device_values.shape) == (mesh.num_box_cells, 3, 3)
    ops_dev = build_ops(hip_ctx, mesh, conductivity_array(M, mesh))
    assert ms.f0._host_values is None and M._host_values is None  # nothing crossed to the host
    host = g.CellField(mesh, M.values.copy())  # (the fetched copy is read-only; the upload wants a writable buffer)
    assert type(host) is g.CellField and isinstance(conductivity_array(host, mesh), np.ndarray)
    ops_host = build_ops(hip_ctx, mesh, conductivity_array(host, mesh))
    assert ops_dev.per_node and ops_host.per_node
    assert torch.equal(ops_dev._mass_dev, ops_host._mass_dev) and torch.equal(ops_dev._stiff_dev, ops_host._stiff_dev)
    # the tensors themselves: those NumPy forms from the host copy of the fibres, to rounding
    f = ms.f0.values
    want = ref.S_T * np.eye(3)[None] + (ref.S_L - ref.S_T) * np.einsum("ci,cj->cij", f, f)
    assert np.abs(M.values - want).max() <= 4e-16 * ref.S_L
    assert float(ops_dev._stiff_dev.abs().max()) > 0.0


def test_one_split_step_on_a_shell_with_generated_fibres(hip_ctx):
    """A 16^3 box: Laplace solve, fibres, tensors and operators on the device, then one split step; the potential stays finite."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    mesh, V, ft = _shell_mesh()
    ms = beat.fibres.lv_rule_based(V, ft, 10, 20, long_axis=(0.0, 0.0, 1.0))
    active = mesh.active_box
    f0 = ms.f0.values
    assert int((active & ~f0.any(axis=1)).sum()) == ms.degenerate and not f0[~active].any()
    norm = np.linalg.norm(f0[active & f0.any(axis=1)], axis=1)
    assert np.abs(norm - 1.0).max() <= 1e-14
    cond = beat.conductivities.default_conductivities("Bishop")
    M = beat.conductivities.define_conductivity_tensor(f0=ms.f0, **cond)
    time = g.Constant(mesh, 0.0)
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=ft, marker=10, mesh_unit="mm",
                                           amplitude=2000.0, start=0.0, duration=1.0)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01)
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=pde.state, fun=tp06.generalized_rush_larsen, init_states=ic,
                                         parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(ic),
                                         v_index=tp06.state_index("V"))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    solver.step((0.0, 0.05))
    v = np.asarray(pde.state.x.array)
    assert np.isfinite(v).all()
    tissue = v[mesh.node_active()]
    print(f"one split step: v in [{tissue.min():.3f}, {tissue.max():.3f}] mV on {tissue.size} tissue nodes, {ms.degenerate} degenerate voxels")
