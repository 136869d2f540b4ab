"""GPU: bi-ventricular rule-based fibres.  The kernel through the C ABI against tests/_fibres_biv_ref.py on the inputs the CPU test
holds the header to; the public API with exactly linear fields against the closed forms; the synthetic geometry of
demos/biv_fibres.py at 24^3 through biv_rule_based, down to the operator rows; one split step on it."""
import ctypes as C
import importlib.util
import logging
import math
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import _fibres_biv_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _call(ctx, c, want_frame, want_tensor):
    """beat_fibres_biv_rule on the case ``c``; outputs that are not wanted are passed as NULL.  Every output starts as NaN."""
    from beat import _hip

    torch = ctx.torch
    nvox = int(np.prod(c.cells))
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device)  # noqa: E731
    f, s, n = (new(nvox, 3) if want_frame else None for _ in range(3))
    M = new(nvox, 9) if want_tensor else None
    count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    fields = [ctx.from_numpy(np.array(a)) for a in (c.phi_lv, c.phi_rv, c.phi_epi)]  # (copies: the shared inputs are read-only)
    psi = None if c.psi is None else ctx.from_numpy(np.array(c.psi))
    active = None if c.active is None else ctx.from_numpy(c.active.astype(np.uint8))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rad = [math.radians(a) for a in ref.ANGLES]
    _hip.check(ctx.lib.beat_fibres_biv_rule(ctx.handle, (C.c_int64 * 3)(*c.cells), (C.c_double * 3)(*c.h), *(ptr(t) for t in fields),
                                            ptr(psi), None if c.axis is None else (C.c_double * 3)(*c.axis), ptr(active), *rad,
                                            ref.S_L, ref.S_T, ptr(f), ptr(s), ptr(n), ptr(M), ptr(count)))
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return host(f), host(s), host(n), None if M is None else host(M).reshape(nvox, 3, 3), int(count.item())


@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_kernel_against_reference(hip_ctx, case):
    """(1) all outputs at once, then only dev_M with the others NULL: f, s, n within TOL per component, the tensor within
    TOL max(|s_l|, |s_t|), the same degenerate count, zeros on the inactive voxels; the two runs' tensors bit-equal."""
    c = ref.case(*case)
    ref.assert_conditions(c.ref)
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
    """(2) all three fields constant over every voxel, with a mask: zeros, the isotropic tensor, and only the active voxels counted."""
    base = ref.case((130, 3, 3), False, True, "septum")
    flat = np.full_like(base.phi_lv, 0.5)
    c = type(base)(**{**vars(base), "phi_lv": flat, "phi_rv": flat, "phi_epi": flat})
    f, s, n, M, count = _call(hip_ctx, c, True, True)
    assert count == int(base.active.sum())
    assert not f.any() and not s.any() and not n.any()
    assert np.array_equal(M[base.active], np.broadcast_to(ref.S_T * np.eye(3), (count, 3, 3))) and not M[~base.active].any()


def test_entry_point_refuses(hip_ctx):
    """(3) BEAT_EINVAL before anything is enqueued."""
    ctx = hip_ctx
    torch = ctx.torch
    buf = torch.zeros(64, dtype=torch.float64, device=ctx.device)
    out = torch.full((3,), 7.0, dtype=torch.float64, device=ctx.device)
    count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    p, o, q = C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(count.data_ptr())
    odd = C.c_void_p(buf.data_ptr() + 4)
    cells, h, axis = (C.c_int64 * 3)(1, 1, 1), (C.c_double * 3)(1.0, 1.0, 1.0), (C.c_double * 3)(0.0, 0.0, 1.0)
    angles = (1.0, -1.0, 0.0, 0.0, 1.0, 1.0)
    call = ctx.lib.beat_fibres_biv_rule
    for lv, rv, epi in ((None, p, p), (p, None, p), (p, p, None), (odd, p, p), (p, odd, p), (p, p, odd)):  # every field is required
        assert call(ctx.handle, cells, h, lv, rv, epi, None, axis, None, *angles, o, None, None, None, q) == -1
    assert call(ctx.handle, cells, h, p, p, p, None, None, None, *angles, o, None, None, None, q) == -1  # neither psi nor axis
    assert call(ctx.handle, cells, h, p, p, p, odd, None, None, *angles, o, None, None, None, q) == -1
    assert call(ctx.handle, cells, h, p, p, p, None, axis, None, *angles, None, None, None, None, q) == -1  # no output
    assert call(ctx.handle, cells, h, p, p, p, None, axis, None, *angles, o, None, None, None, None) == -1  # no counter
    assert call(ctx.handle, (C.c_int64 * 3)(1, 0, 1), h, p, p, p, None, axis, None, *angles, o, None, None, None, q) == -1
    assert call(ctx.handle, (C.c_int64 * 3)(1 << 20, 1, 1), h, p, p, p, None, axis, None, *angles, o, None, None, None, q) == -1
    assert call(ctx.handle, cells, (C.c_double * 3)(1.0, 0.0, 1.0), p, p, p, None, axis, None, *angles, o, None, None, None, q) == -1
    ctx.synchronize()
    assert int(count.item()) == 0 and (out == 7.0).all()  # the refused calls counted and wrote nothing
    assert call(ctx.handle, cells, h, p, p, p, None, axis, None, *angles, o, None, None, None, q) == 0  # the accepted call next to them
    ctx.synchronize()
    assert int(count.item()) == 1 and not out.any()  # its one voxel (all fields 0 at its corners) is degenerate


# ---- the public API ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("region", ref.REGIONS)
def test_closed_forms_through_the_public_api(hip_ctx, region):
    """(4) biv_rule with exactly linear P1 functions on the (8, 4, 4) box reproduces the closed forms of the CPU test to 1e-12, up to
    sign; no Laplace solve is involved."""
    from beat import fibres
    from beat import grid as g

    cells, _, L, x, _ = ref.slab()
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(L)], list(cells))
    V = g.functionspace(mesh, ("P", 1))
    angles = (40.0, -50.0, 0.0, 0.0)
    forms, angle = ref.closed_form(region, angles)
    fields = []
    for fn in forms:
        fields.append(g.Function(V))
        fields[-1].x.array[:] = fn(x / L[0])
    ms = fibres.biv_rule(mesh, *fields, (0.0, 0.0, 1.0), *angles)
    assert isinstance(ms.f0, g.DeviceCellField) and ms.f0.device_values.is_cuda and ms.degenerate == 0
    want = np.stack([np.zeros_like(angle), np.cos(angle), np.sin(angle)], axis=1)
    f0, s0, n0 = ms.f0.values, ms.s0.values, ms.n0.values
    sign = np.where((f0 * want).sum(axis=1) < 0.0, -1.0, 1.0)[:, None]
    err = np.abs(f0 - sign * want).max()
    print(f"{region}: max |f0 -+ closed form| = {err:.3e}")
    assert err <= 1e-12
    assert np.abs(np.abs(s0[:, 0]) - 1.0).max() <= 1e-12 and np.abs(np.cross(f0, n0) - s0).max() <= 1e-12


@lru_cache(maxsize=None)
def _demo():
    sys.path.insert(0, str(ROOT / "demos"))
    try:
        spec = importlib.util.spec_from_file_location("demo_biv_fibres", ROOT / "demos" / "biv_fibres.py")
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        sys.path.remove(str(ROOT / "demos"))
    return module


@lru_cache(maxsize=None)
def _heart():
    """The 24^3 instance of the demo's geometry and its fibres, made once: (demo module, mesh, V, ft, apex, Microstructure, the log)."""
    import beat

    demo = _demo()
    mesh, V, ft, apex = demo.geometry(24, 0.5)
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    log = logging.getLogger("beat.fibres")
    log.addHandler(handler)
    try:
        ms = beat.fibres.biv_rule_based(V, ft, demo.ENDO_LV, demo.ENDO_RV, demo.EPI, base_marker=demo.BASE, apex_facets=apex)
    finally:
        log.removeHandler(handler)
    return demo, mesh, V, ft, apex, ms, [r.getMessage() for r in records if r.levelno >= logging.WARNING]


def test_synthetic_heart_frames(hip_ctx):
    """(5) f0 is a DeviceCellField on the device; the frames are orthonormal to 1e-14 on the non-degenerate tissue voxels and exactly
    zero on the inactive and the degenerate ones; the logged count matches; fewer than 1 % of the tissue voxels are degenerate."""
    from beat import grid as g

    _, mesh, _, _, _, ms, warnings = _heart()
    assert isinstance(ms.f0, g.DeviceCellField) and ms.f0.device_values.is_cuda
    active = mesh.active_box
    f0, s0, n0 = ms.f0.values, ms.s0.values, ms.n0.values
    dead = active & ~f0.any(axis=1)
    live = active & ~dead
    print(f"24^3 heart: {int(active.sum())} tissue voxels, {ms.degenerate} degenerate = {100.0 * ms.degenerate / active.sum():.2f} %")
    assert int(dead.sum()) == ms.degenerate
    if ms.degenerate:
        assert len(warnings) == 1 and f"{ms.degenerate} degenerate voxel(s)" in warnings[0], warnings
    else:
        assert not warnings, warnings
    assert ms.degenerate < 0.01 * active.sum()
    for v in (f0, s0, n0):
        assert not v[~live].any()
        assert np.abs(np.linalg.norm(v[live], axis=1) - 1.0).max() <= 1e-14
    for a, b in ((f0, s0), (f0, n0), (s0, n0)):
        assert np.abs((a[live] * b[live]).sum(axis=1)).max() <= 1e-14
    assert np.abs(np.cross(f0[live], n0[live]) - s0[live]).max() <= 1e-14


def test_synthetic_heart_equals_biv_rule_on_the_same_solutions(hip_ctx):
    """(5) biv_rule_based is biv_rule fed the four Laplace solutions it describes, bit for bit."""
    from beat import fibres
    from beat.utils import laplace_dirichlet

    demo, mesh, V, ft, apex, ms, _ = _heart()
    lv, rv, epi = (ft.find(m) for m in (demo.ENDO_LV, demo.ENDO_RV, demo.EPI))
    phi_lv = laplace_dirichlet(V, [(rv, 0.0), (epi, 0.0), (lv, 1.0)])
    phi_rv = laplace_dirichlet(V, [(lv, 0.0), (epi, 0.0), (rv, 1.0)])
    phi_epi = laplace_dirichlet(V, [(lv, 0.0), (rv, 0.0), (epi, 1.0)])
    psi = laplace_dirichlet(V, [(apex, 0.0), (ft.find(demo.BASE), 1.0)])
    for u in (phi_lv, phi_rv, phi_epi, psi):
        a = np.asarray(u.x.array)[mesh.node_active()]
        assert a.min() >= -1e-8 and a.max() <= 1.0 + 1e-8 and np.ptp(a) > 0.99
    again = fibres.biv_rule(mesh, phi_lv, phi_rv, phi_epi, psi)
    assert again.degenerate == ms.degenerate
    for name in ("f0", "s0", "n0"):
        assert np.array_equal(getattr(again, name).values, getattr(ms, name).values), name


def test_synthetic_heart_device_path_equals_host_path(hip_ctx):
    """(5) the (15, n) mass and stiffness rows of the operators built from the device-resident tensors are bit for bit those built
    from their host copy, and the device route fetched no host copy on its way."""
    import torch

    from beat import conductivities, fibres
    from beat import grid as g
    from beat._engine import build_ops, conductivity_array

    demo, mesh, V, ft, apex, _, _ = _heart()
    ms = fibres.biv_rule_based(V, ft, demo.ENDO_LV, demo.ENDO_RV, demo.EPI, long_axis=(0.0, 0.0, 1.0))  # (a frame nobody has fetched)
    M = conductivities.conductivity_tensor(ref.S_L, ref.S_T, ms.f0)
    assert isinstance(M, g.DeviceCellField) and tuple(M.device_values.shape) == (mesh.num_box_cells, 3, 3)
    ops_dev = build_ops(hip_ctx, mesh, conductivity_array(M, mesh))
    assert ms.f0._host_values is None and M._host_values is None  # nothing crossed to the host
    host = g.CellField(mesh, M.values.copy())  # (the fetched copy is read-only; the upload wants a writable buffer)
    assert type(host) is g.CellField and isinstance(conductivity_array(host, mesh), np.ndarray)
    ops_host = build_ops(hip_ctx, mesh, conductivity_array(host, mesh))
    assert ops_dev.per_node and ops_host.per_node
    assert torch.equal(ops_dev._mass_dev, ops_host._mass_dev) and torch.equal(ops_dev._stiff_dev, ops_host._stiff_dev)
    assert float(ops_dev._stiff_dev.abs().max()) > 0.0


def test_one_split_step_on_the_synthetic_heart(hip_ctx):
    """(6) fibres, tensors and operators made on the device, then one split step with TP06; the potential stays finite."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    demo, mesh, V, ft, _, ms, _ = _heart()
    cond = beat.conductivities.default_conductivities("Bishop")
    M = beat.conductivities.define_conductivity_tensor(f0=ms.f0, **cond)
    time = g.Constant(mesh, 0.0)
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=ft, marker=demo.ENDO_LV, mesh_unit="mm",
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
    assert tissue.max() > tissue.min()
