"""Rule-based fibre, sheet and sheet-normal fields of a voxel geometry, made ON THE DEVICE.

The reference's ventricular demos (demos/lv_endocardial.py, demos/biv_endocardial.py, demos/ukb_atlas.py) take their fibres from
``cardiac_geometries(create_fibers=True, fiber_angle_endo=60, fiber_angle_epi=-60)``, a Laplace-Dirichlet rule-based generator over
FEniCSx.  Here the two harmonic fields come from ``beat.utils.laplace_dirichlet``, one kernel (beat_fibres_rule, include/beat_hip.h
has the rule) turns them into an orthonormal frame per voxel, and the frame stays on the device: ``grid.DeviceCellField`` goes
through ``conductivities.define_conductivity_tensor`` into the operator assembly without a host copy.

Conventions.  ``transmural`` is 0 on the endocardium and 1 on the epicardium, ``longitudinal`` increases from apex to base (or is a
constant vector pointing that way).  With e_l the unit longitudinal direction, e_t the unit transmural direction made orthogonal to
it and e_c = e_l x e_t the circumferential one, the fibre is e_c turned by alpha towards e_l and the sheet e_t turned by beta about
the fibre; both angles are linear in the transmural field (in degrees here, Bayer et al. 2012's ``orient``).  (f0, n0, s0) is
right-handed.  A voxel where one of the gradients vanishes or the two are parallel is *degenerate*: its three vectors are 0, which
makes its conductivity the isotropic s_t I.

One ventricle, one rank, per-voxel output: bi-ventricular rules with a septum (they need Bayer's ``bislerp``), decomposed meshes and
per-simplex fields are not implemented."""

from __future__ import annotations

import ctypes as C
import logging
import math
from typing import NamedTuple

import numpy as np

from . import _hip, grid

logger = logging.getLogger(__name__)


class Microstructure(NamedTuple):
    """Per-voxel fibre, sheet and sheet-normal fields (``grid.DeviceCellField``, (num_box_cells, 3)) and the number of degenerate voxels."""

    f0: grid.DeviceCellField
    s0: grid.DeviceCellField
    n0: grid.DeviceCellField
    degenerate: int


def _check_mesh(mesh) -> None:
    if mesh.dim != 3:
        raise ValueError(f"rule-based fibres need a 3-D voxel mesh, got a {mesh.dim}-D one")
    if mesh.comm.size > 1:
        raise NotImplementedError("rule_based on a decomposed mesh: the kernel would need the harmonic fields' upper ghost plane "
                                  "and each rank its own slab of voxels, and nothing exchanges or tests them yet")
    if mesh.active is not None and mesh.active_box is None:
        raise ValueError("rule-based fibres are per voxel: the mesh's mask was given per simplex")


def _axis(longitudinal) -> np.ndarray:
    try:
        a = np.asarray(longitudinal.value if isinstance(longitudinal, grid.Constant) else longitudinal, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("longitudinal must be a P1 function or a 3-vector") from None
    if a.shape != (3,):
        raise ValueError(f"the longitudinal axis must have 3 components, got shape {a.shape}")
    if not np.isfinite(a).all() or not np.any(a != 0.0):
        raise ValueError(f"the longitudinal axis must be finite and non-zero, got {a}")
    return a


def _nodal(f, mesh, what):
    if not isinstance(f, grid.Function) or not f.function_space.is_p1:
        raise TypeError(f"{what} must be a P1 function (beat.utils.laplace_dirichlet returns one)")
    if f.num_values != mesh.num_nodes:
        raise ValueError(f"{what} has {f.num_values} values on a mesh of {mesh.num_nodes} nodes")
    return f.field


def rule_based(mesh, transmural, longitudinal, alpha_endo=60.0, alpha_epi=-60.0, beta_endo=0.0, beta_epi=0.0) -> Microstructure:
    """Fibres, sheets and sheet normals of the (active) voxels of ``mesh`` from the P1 function ``transmural`` (0 endo, 1 epi) and
    ``longitudinal``: a P1 function increasing from apex to base, or a constant 3-vector.  Angles in degrees.  Logs a warning when
    there are degenerate voxels and returns their number."""
    _check_mesh(mesh)
    if longitudinal is None:
        raise ValueError("no longitudinal input: give a P1 function that increases from apex to base, or a 3-vector")
    axis = None if isinstance(longitudinal, grid.Function) else _axis(longitudinal)
    angles = [float(v) for v in (alpha_endo, alpha_epi, beta_endo, beta_epi)]
    if not all(math.isfinite(v) for v in angles):
        raise ValueError(f"angles must be finite, got {angles}")
    phi = _nodal(transmural, mesh, "transmural")
    psi = None if axis is not None else _nodal(longitudinal, mesh, "longitudinal")
    ctx = transmural._ctx
    torch = ctx.torch
    nvox = mesh.num_box_cells
    out = [torch.empty((nvox, 3), dtype=torch.float64, device=ctx.device) for _ in range(3)]
    count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    active = None if mesh.active_box is None else ctx.from_numpy(mesh.active_box.astype(np.uint8))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    _hip.check(ctx.lib.beat_fibres_rule(
        ctx.handle, (C.c_int64 * 3)(*mesh.n), (C.c_double * 3)(*mesh.h), phi.ptr, None if psi is None else psi.ptr,
        None if axis is None else (C.c_double * 3)(*axis), ptr(active), *(math.radians(v) for v in angles), 1.0, 1.0,
        ptr(out[0]), ptr(out[1]), ptr(out[2]), None, ptr(count)))
    degenerate = int(count.item())  # (waits for the kernel; `active` and the inputs are alive until here)
    if degenerate:
        logger.warning("rule_based: %d degenerate voxel(s) (a vanishing gradient, or the transmural and the longitudinal direction "
                       "parallel) got f0 = s0 = n0 = 0: their conductivity is isotropic", degenerate)
    f0, s0, n0 = (grid.DeviceCellField(mesh, t) for t in out)
    return Microstructure(f0, s0, n0, degenerate)


def lv_rule_based(V, ft, endo_marker, epi_marker, base_marker=None, apex_facets=None, long_axis=None, **angles) -> Microstructure:
    """``rule_based`` for one ventricle whose surfaces are tagged in ``ft``: the transmural field is harmonic with 0 on the facets
    tagged ``endo_marker`` and 1 on those tagged ``epi_marker``; the longitudinal one harmonic with 0 on ``apex_facets`` (facet ids)
    and 1 on the facets tagged ``base_marker`` when both are given, the constant ``long_axis`` otherwise.  Both solves run on the
    device (``utils.laplace_dirichlet``).  ``angles``: alpha_endo, alpha_epi, beta_endo, beta_epi in degrees."""
    from .utils import laplace_dirichlet

    mesh = V.mesh
    _check_mesh(mesh)
    if np.ndim(endo_marker) != 0 or np.ndim(epi_marker) != 0:
        raise NotImplementedError("one endocardial and one epicardial marker: a bi-ventricular rule (two endocardia, a septum) needs "
                                  "Bayer's bislerp between the two ventricles' frames, which is not implemented")
    unknown = set(angles) - {"alpha_endo", "alpha_epi", "beta_endo", "beta_epi"}
    if unknown:
        raise TypeError(f"unknown arguments {sorted(unknown)}")
    solve_psi = base_marker is not None and apex_facets is not None
    if not solve_psi:
        if long_axis is None:
            raise ValueError("no longitudinal input: give base_marker and apex_facets (a harmonic apex-to-base field is solved "
                             "for), or long_axis")
        long_axis = _axis(long_axis)
    phi = laplace_dirichlet(V, [(ft.find(endo_marker), 0.0), (ft.find(epi_marker), 1.0)])
    if solve_psi:
        psi = laplace_dirichlet(V, [(np.asarray(apex_facets, dtype=np.int64), 0.0), (ft.find(base_marker), 1.0)])
        return rule_based(mesh, phi, psi, **angles)
    return rule_based(mesh, phi, long_axis, **angles)
