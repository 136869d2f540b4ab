#!/usr/bin/env python3
"""Rule-based fibres on a voxelised pair of ventricles: two truncated ellipsoidal cavities in one truncated ellipsoidal body as a
voxel mask, LV / RV endocardium, epicardium, base and apex tagged on the staircase surface, and from there everything on the device
-- four Laplace solves and Bayer's rule with bislerp for the fibre / sheet / normal frame of every voxel
(``beat.fibres.biv_rule_based``), endo / mid / epi layers (``utils.expand_layer_biv``), the conductivity tensors
(``define_conductivity_tensor``), the operators -- then a few split steps of ToR-ORd with one parameter set per layer and a stimulus
on the LV endocardium.

The reference's bi-ventricular demos get this input from ``cardiac_geometries(create_fibers=True, ...)`` (demos/biv_endocardial.py,
demos/ukb_atlas.py).

    python demos/biv_fibres.py [--size 24] [--h 0.5] [--steps 3] [--dt 0.05]

Prints the facet counts, the number of degenerate voxels (none of the three frames defined: all of a voxel's corners but one carry
Dirichlet values, which happens in the apex cap), the layer sizes and the potential's range."""
import argparse

import _path  # noqa: F401
import numpy as np

import beat
from beat import grid as g
from beat.models import torord

MIN_SIZE = 24  # below this the thinnest wall is thinner than two voxels
ENDO_LV, ENDO_RV, EPI, BASE = 10, 11, 20, 30
CAP_LAYERS = 1  # voxel layers at the apex whose epicardial facets carry the longitudinal field's 0
BASE_PLANE = 0.8  # the truncation plane, as a share of the box's height
# centres and semi-axes as shares of the box's edge: the body, and the two cavities that the plane cuts open.  Walls and septum are
# 0.09 to 0.15 of the edge thick.
BODY = ((0.50, 0.50, 0.50), (0.48, 0.44, 0.48))
LV_CAVITY = ((0.35, 0.50, 0.50), (0.19, 0.30, 0.36))
RV_CAVITY = ((0.755, 0.50, 0.55), (0.10, 0.26, 0.30))


def _level(points, ellipsoid, edge, grow=0.0):
    """< 1 inside the ellipsoid, whose semi-axes are made ``grow`` longer."""
    centre, semi = (np.asarray(v) * edge for v in ellipsoid)
    return np.sqrt((((points - centre) / (semi + grow)) ** 2).sum(axis=-1))


def biv_mask(n, h):
    """(n, n, n) bool: the voxels whose centre lies in the body, in neither cavity and below the base plane."""
    ax = (np.arange(n) + 0.5) * h
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    P = np.stack([X, Y, Z], axis=-1)
    edge = n * h
    return ((_level(P, BODY, edge) < 1.0) & (_level(P, LV_CAVITY, edge) > 1.0) & (_level(P, RV_CAVITY, edge) > 1.0)
            & (Z < BASE_PLANE * edge))


def tag_biv(mesh, n, h):
    """Facet tags of the staircase surface by where the facet centre lies -- BASE on the top plane, ENDO_LV inside the LV cavity's
    ellipsoid, ENDO_RV inside the RV one, EPI elsewhere -- and the ids of the apex facets (epicardial facets of the lowest CAP_LAYERS
    voxel layers).  A cavity facet's centre is half a voxel from a voxel centre inside the cavity, so the ellipsoids are taken half
    a voxel larger here."""
    edge = n * h
    facets = mesh.exterior_facets()
    xyz = g._node_xyz(mesh, mesh.facet_vertices(facets).ravel()).reshape(len(facets), 4, 3)
    ctr = xyz.mean(axis=1)
    base = (np.ptp(xyz[:, :, 2], axis=1) < 1e-12) & (ctr[:, 2] > ctr[:, 2].max() - 1e-9)
    lv = ~base & (_level(ctr, LV_CAVITY, edge, grow=0.5 * h) < 1.0)
    rv = ~base & ~lv & (_level(ctr, RV_CAVITY, edge, grow=0.5 * h) < 1.0)
    values = np.where(base, BASE, np.where(lv, ENDO_LV, np.where(rv, ENDO_RV, EPI))).astype(np.int32)
    apex = facets[(values == EPI) & (ctr[:, 2] < ctr[:, 2].min() + (CAP_LAYERS - 0.25) * h)]
    return g.meshtags(mesh, 2, facets, values), apex


def geometry(n, h):
    """The mesh, its P1 space, the facet tags and the apex facets of the n^3 box."""
    mesh = g.create_voxel_mesh(g.COMM_WORLD, biv_mask(n, h), h)
    ft, apex = tag_biv(mesh, n, h)
    return mesh, g.functionspace(mesh, ("P", 1)), ft, apex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=MIN_SIZE, help=f"voxels per axis (at least {MIN_SIZE})")
    ap.add_argument("--h", type=float, default=0.5, help="voxel edge in mm")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--dt", type=float, default=0.05)
    args = ap.parse_args()
    if args.size < MIN_SIZE:
        ap.error(f"--size must be at least {MIN_SIZE}")
    n, h = args.size, args.h

    mesh, V, ft, apex = geometry(n, h)
    tissue = mesh.node_active()
    print(f"box {n}^3, {int(mesh.active_box.sum())} tissue voxels, facets LV endo / RV endo / epi / base / apex = "
          f"{[int((ft.values == k).sum()) for k in (ENDO_LV, ENDO_RV, EPI, BASE)] + [len(apex)]}", flush=True)

    ms = beat.fibres.biv_rule_based(V, ft, ENDO_LV, ENDO_RV, EPI, base_marker=BASE, apex_facets=apex)
    print(f"degenerate voxels: {ms.degenerate} of {int(mesh.active_box.sum())}", flush=True)
    layers = beat.utils.expand_layer_biv(V, ft, ENDO_LV, ENDO_RV, EPI, endo_size=0.3, epi_size=0.3)
    marker_arr = np.where(tissue, np.asarray(layers.x.array), -1.0)
    markers = g.Function(V)
    markers.x.array[:] = marker_arr
    print(f"endo / mid / epi nodes = {[int((marker_arr == k).sum()) for k in (1, 0, 2)]}", flush=True)
    cond = beat.conductivities.default_conductivities("Bishop")
    M = beat.conductivities.define_conductivity_tensor(f0=ms.f0, **cond)  # stays on the device

    time = g.Constant(mesh, 0.0)
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=ft, marker=ENDO_LV, mesh_unit="mm",
                                           amplitude=2000.0, start=0.0, duration=1.0)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01)
    keys = (0, 1, 2)  # layer markers: 1 endo, 0 mid, 2 epi; the model's celltype: 0 endo, 1 epi, 2 mid
    celltype = {1: 0, 2: 1, 0: 2}
    ic = torord.init_state_values()
    ode = beat.odesolver.DolfinMultiODESolver(
        v_ode=g.Function(V), v_pde=pde.state, markers=markers, num_states={k: len(ic) for k in keys},
        fun={k: torord.generalized_rush_larsen for k in keys}, init_states={k: ic for k in keys},
        parameters={k: torord.init_parameter_values(i_Stim_Amplitude=0.0, celltype=celltype[k]) for k in keys},
        v_index={k: torord.state_index("v") for k in keys})
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    t = 0.0
    for _ in range(args.steps):
        solver.step((t, t + args.dt))
        t += args.dt
    v = np.asarray(pde.state.x.array)[tissue]
    if not np.isfinite(v).all():
        raise SystemExit("the potential is not finite")
    print(f"{args.steps} split steps of {args.dt} ms: v in [{v.min():.2f}, {v.max():.2f}] mV on the tissue nodes")

    # the report: the host copy of the fibres is fetched here, for the first time
    f0 = ms.f0.values
    active = mesh.active_box
    dead = active & ~f0.any(axis=1)
    assert int(dead.sum()) == ms.degenerate, (int(dead.sum()), ms.degenerate)
    norm = np.linalg.norm(f0[active & ~dead], axis=1)
    print(f"|f0| - 1 on the other {int((active & ~dead).sum())} tissue voxels: at most {np.abs(norm - 1.0).max():.1e}")


if __name__ == "__main__":
    main()
