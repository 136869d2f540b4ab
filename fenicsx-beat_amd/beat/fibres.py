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

Two ventricles (``biv_rule``, ``biv_rule_based``; beat_fibres_biv_rule) follow Algorithm 1 of Bayer, Blake, Plank and Trayanova
(2012).  Three transmural fields, each 1 on its own surface and 0 on the other two -- LV endocardium, RV endocardium, epicardium --
give one frame each by the rule above: the two endocardial ones with the angles alpha_endo (1 - 2 d), beta_endo (1 - 2 d), where
d = phi_rv / (phi_lv + phi_rv) runs from 0 at the LV to 1 at the RV endocardium, the epicardial one with the angles linear in
phi_epi.  ``bislerp`` -- the spherical interpolation of two frames as quaternions, after the first has been replaced by whichever
of (f, n, s), (f, -n, -s), (-f, n, -s), (-f, -n, s) is nearest to the second -- blends the endocardial two by d and the result with
the epicardial one by phi_epi.  A frame whose gradients vanish or are parallel is left out of its blend; a voxel is degenerate
where all three are.  A fibre is a line: the result may have two of its vectors negated relative to an input frame.
The rule's own limit: when the endocardial and the epicardial frame are more than 90 degrees apart, ``bislerp`` turns towards the
flipped candidate and the fibre angle jumps across the wall; for beta = 0 that is phi_epi |alpha_epi - alpha_endo| > 90 degrees.
The defaults there are the paper's, alpha_endo = 40 and alpha_epi = -50, which stay inside it; ``biv_rule`` logs a warning otherwise.

One rank, per-voxel output, one set of angles for both ventricles and the septum: decomposed meshes, per-simplex fields and
separate LV / RV / septal angles are not implemented."""

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


def _checked_inputs(mesh, longitudinal, angles):
    """What both rules check before they look at a transmural field: (the axis or None, the four angles as floats)."""
    _check_mesh(mesh)
    if longitudinal is None:
        raise ValueError("no longitudinal input: give a P1 function that increases from apex to base, or a 3-vector")
    axis = None if isinstance(longitudinal, grid.Function) else _axis(longitudinal)
    angles = [float(v) for v in angles]
    if not all(math.isfinite(v) for v in angles):
        raise ValueError(f"angles must be finite, got {angles}")
    return axis, angles


def _frames(mesh, entry, transmural, psi, axis, angles, who, why) -> Microstructure:
    """One launch of ``entry`` (beat_fibres_rule or beat_fibres_biv_rule: they differ in the number of transmural fields) for the three
    vectors of every voxel; the degenerate voxels are logged as ``who``'s, degenerate because of ``why``."""
    ctx = transmural[0].ctx
    torch = ctx.torch
    nvox = mesh.num_box_cells
    out = [torch.empty((nvox, 3), dtype=torch.float64, device=ctx.device) for _ in range(3)]
    count = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    active = None if mesh.active_box is None else ctx.from_numpy(mesh.active_box.astype(np.uint8))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    _hip.check(getattr(ctx.lib, entry)(
        ctx.handle, (C.c_int64 * 3)(*mesh.n), (C.c_double * 3)(*mesh.h), *(phi.ptr for phi in transmural),
        None if psi is None else psi.ptr, None if axis is None else (C.c_double * 3)(*axis), ptr(active),
        *(math.radians(v) for v in angles), 1.0, 1.0, ptr(out[0]), ptr(out[1]), ptr(out[2]), None, ptr(count)))
    degenerate = int(count.item())  # (waits for the kernel; `active` and the inputs are alive until here)
    if degenerate:
        logger.warning("%s: %d degenerate voxel(s) (%s) got f0 = s0 = n0 = 0: their conductivity is isotropic", who, degenerate, why)
    f0, s0, n0 = (grid.DeviceCellField(mesh, t) for t in out)
    return Microstructure(f0, s0, n0, degenerate)


def rule_based(mesh, transmural, longitudinal, alpha_endo=60.0, alpha_epi=-60.0, beta_endo=0.0, beta_epi=0.0) -> Microstructure:
    """Fibres, sheets and sheet normals of the (active) voxels of ``mesh`` from the P1 function ``transmural`` (0 endo, 1 epi) and
    ``longitudinal``: a P1 function increasing from apex to base, or a constant 3-vector.  Angles in degrees.  Logs a warning when
    there are degenerate voxels and returns their number."""
    axis, angles = _checked_inputs(mesh, longitudinal, (alpha_endo, alpha_epi, beta_endo, beta_epi))
    phi = _nodal(transmural, mesh, "transmural")
    psi = None if axis is not None else _nodal(longitudinal, mesh, "longitudinal")
    return _frames(mesh, "beat_fibres_rule", [phi], psi, axis, angles, "rule_based",
                   "a vanishing gradient, or the transmural and the longitudinal direction parallel")


def biv_rule(mesh, phi_lv, phi_rv, phi_epi, longitudinal, alpha_endo=40.0, alpha_epi=-50.0, beta_endo=0.0, beta_epi=0.0) -> Microstructure:
    """Fibres, sheets and sheet normals of the (active) voxels of a bi-ventricular ``mesh`` by Bayer's rule (the module's docstring):
    ``phi_lv``, ``phi_rv`` and ``phi_epi`` are P1 functions, each 1 on its own surface (LV endocardium, RV endocardium, epicardium) and
    0 on the other two; ``longitudinal`` is a P1 function increasing from apex to base, or a constant 3-vector.  Angles in degrees,
    one set for both ventricles; the defaults are the paper's.  More than 90 degrees between alpha_endo and alpha_epi is past the
    rule's limit -- the fibre angle jumps inside the wall -- and is logged as a warning, not refused.  Logs a warning when there are
    degenerate voxels and returns their number."""
    axis, angles = _checked_inputs(mesh, longitudinal, (alpha_endo, alpha_epi, beta_endo, beta_epi))
    if abs(angles[1] - angles[0]) > 90.0:
        logger.warning("biv_rule: alpha_endo = %g and alpha_epi = %g are more than 90 degrees apart: where phi_epi |alpha_epi - "
                       "alpha_endo| passes 90 degrees bislerp turns towards the flipped frame and the fibre angle jumps", *angles[:2])
    transmural = [_nodal(f, mesh, name) for f, name in ((phi_lv, "phi_lv"), (phi_rv, "phi_rv"), (phi_epi, "phi_epi"))]
    psi = None if axis is not None else _nodal(longitudinal, mesh, "longitudinal")
    return _frames(mesh, "beat_fibres_biv_rule", transmural, psi, axis, angles, "biv_rule",
                   "none of the three frames is defined: every transmural gradient vanishes or is parallel to the longitudinal direction")


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
                                  "Bayer's bislerp between the two ventricles' frames, which is biv_rule_based, not this function")
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


def biv_rule_based(V, ft, endo_lv_marker, endo_rv_marker, epi_marker, base_marker=None, apex_facets=None, long_axis=None,
                   **angles) -> Microstructure:
    """``biv_rule`` for two ventricles whose surfaces are tagged in ``ft``: three harmonic fields, each 1 on the facets of one of
    ``endo_lv_marker``, ``endo_rv_marker``, ``epi_marker`` and 0 on those of the other two; the longitudinal input as for
    ``lv_rule_based``.  All solves run on the device (``utils.laplace_dirichlet``).  ``angles``: alpha_endo, alpha_epi, beta_endo,
    beta_epi in degrees."""
    from .utils import laplace_dirichlet

    mesh = V.mesh
    _check_mesh(mesh)
    unknown = set(angles) - {"alpha_endo", "alpha_epi", "beta_endo", "beta_epi"}
    if unknown:
        raise TypeError(f"unknown arguments {sorted(unknown)}")
    solve_psi = base_marker is not None and apex_facets is not None
    if not solve_psi:
        if long_axis is None:
            raise ValueError("no longitudinal input: give base_marker and apex_facets (a harmonic apex-to-base field is solved "
                             "for), or long_axis")
        long_axis = _axis(long_axis)
    surfaces = {"endo_lv_marker": endo_lv_marker, "endo_rv_marker": endo_rv_marker, "epi_marker": epi_marker}
    facets = {}
    for name, marker in surfaces.items():
        facets[name] = ft.find(marker)
        if len(facets[name]) == 0:
            raise ValueError(f"{name} = {marker} tags no facet: biv_rule_based needs both endocardia and the epicardium (one "
                             f"ventricle: lv_rule_based)")
    # (each field's own surface comes last: where two surfaces share a vertex, laplace_dirichlet lets the later entry win)
    phi = [laplace_dirichlet(V, [(f, 0.0) for name, f in facets.items() if name != one] + [(facets[one], 1.0)]) for one in surfaces]
    if solve_psi:
        psi = laplace_dirichlet(V, [(np.asarray(apex_facets, dtype=np.int64), 0.0), (ft.find(base_marker), 1.0)])
        return biv_rule(mesh, *phi, psi, **angles)
    return biv_rule(mesh, *phi, long_axis, **angles)
