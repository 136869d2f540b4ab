#!/usr/bin/env python3
"""Rule-based fibres on a voxelised left ventricle: a truncated ellipsoidal shell as a voxel mask, its endo- / epicardium, base and
apex tagged on the staircase surface, and from there everything on the device -- two Laplace solves, the fibre / sheet / normal
frame of every voxel (``beat.fibres.lv_rule_based``), the conductivity tensors (``define_conductivity_tensor``), the operators --
then a few split steps with an endocardial stimulus.

The reference's ventricular demos get this input from ``cardiac_geometries(create_fibers=True, fiber_angle_endo=60,
fiber_angle_epi=-60)`` (demos/lv_endocardial.py, demos/biv_endocardial.py, demos/ukb_atlas.py).

    python demos/lv_fibres.py [--size 48] [--h 0.25] [--steps 5] [--dt 0.05]

Prints the number of degenerate voxels (and how many of them lie outside the apex cap, where the longitudinal field is pinned), and
the mean and the largest angle between the generated fibres and the closed form of the ellipsoid (``tools/bench_biv.py::shell``).  That
angle is the effect of the staircase boundary on the harmonic fields; it is reported, nothing is expected of it.  Inside the cap the
epicardial facets carry the Dirichlet values of both fields, so a voxel with a single free corner there has parallel gradients and
is degenerate (isotropic conductivity).  Seen at --size 16: 16 degenerate voxels, none outside the cap; angle mean 14.3, max 89.2
degrees."""
import argparse
import sys

import _path
import numpy as np

sys.path.insert(0, str(_path.ROOT / "tools"))

import beat  # noqa: E402
from beat import grid as g  # noqa: E402
from beat.models import tp06  # noqa: E402
from bench_biv import shell  # noqa: E402

MIN_SIZE = 16  # below this the wall is thinner than two voxels
ENDO, EPI, BASE = 10, 20, 30
CAP_LAYERS = 2  # voxel layers at the apex whose epicardial facets carry the longitudinal field's 0


def tag_shell(mesh, semi_axes, h):
    """Facet tags (ENDO / EPI / BASE) of the shell's staircase surface, classified by the facet centre as tools/bench_biv.py::build
    does, the ids of the apex facets (epicardial facets of the lowest CAP_LAYERS voxel layers) and the height below which a voxel
    belongs to that cap."""
    so, si, c = semi_axes
    facets = mesh.exterior_facets()
    xyz = g._node_xyz(mesh, mesh.facet_vertices(facets).ravel()).reshape(len(facets), 4, 3)
    ctr = xyz.mean(axis=1)
    ro = np.sqrt((((ctr - c) / so) ** 2).sum(axis=1))
    ri = np.sqrt((((ctr - c) / si) ** 2).sum(axis=1))
    base = (np.ptp(xyz[:, :, 2], axis=1) < 1e-12) & (ctr[:, 2] > ctr[:, 2].max() - 1e-9)  # the truncation plane
    endo = ~base & (np.abs(ri - 1.0) < np.abs(ro - 1.0) * (1.0 / 0.66))
    values = np.where(base, BASE, np.where(endo, ENDO, EPI)).astype(np.int32)
    z_cap = ctr[:, 2].min() + CAP_LAYERS * h
    apex = facets[(values == EPI) & (ctr[:, 2] < z_cap - 1e-9)]
    return g.meshtags(mesh, 2, facets, values), apex, z_cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=48, help=f"voxels per axis (at least {MIN_SIZE})")
    ap.add_argument("--h", type=float, default=0.25, help="voxel edge in mm")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dt", type=float, default=0.05)
    args = ap.parse_args()
    if args.size < MIN_SIZE:
        ap.error(f"--size must be at least {MIN_SIZE}")
    n, h = args.size, args.h

    mask, f_closed, semi_axes = shell(n, h)
    mesh = g.create_voxel_mesh(g.COMM_WORLD, mask, h)
    ft, apex, z_cap = tag_shell(mesh, semi_axes, h)
    V = g.functionspace(mesh, ("P", 1))
    print(f"box {n}^3, {int(mask.sum())} tissue voxels, facets endo / epi / base / apex = "
          f"{[int((ft.values == k).sum()) for k in (ENDO, EPI, BASE)] + [len(apex)]}", flush=True)

    ms = beat.fibres.lv_rule_based(V, ft, ENDO, EPI, base_marker=BASE, apex_facets=apex)
    cond = beat.conductivities.default_conductivities("Bishop")
    M = beat.conductivities.define_conductivity_tensor(f0=ms.f0, **cond)  # stays on the device

    time = g.Constant(mesh, 0.0)
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=ft, marker=ENDO, mesh_unit="mm",
                                           amplitude=2000.0, start=0.0, duration=1.0)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01)
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=pde.state, fun=tp06.generalized_rush_larsen, init_states=ic,
                                         parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(ic),
                                         v_index=tp06.state_index("V"))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    t = 0.0
    for _ in range(args.steps):
        solver.step((t, t + args.dt))
        t += args.dt
    v = np.asarray(pde.state.x.array)[mesh.node_active()]
    if not np.isfinite(v).all():
        raise SystemExit("the potential is not finite")
    print(f"{args.steps} split steps of {args.dt} ms: v in [{v.min():.2f}, {v.max():.2f}] mV on the tissue nodes")

    # the report: the host copy of the fibres is fetched here, for the first time
    f0 = ms.f0.values
    active = mask.ravel()
    dead = active & ~f0.any(axis=1)
    z_centre = g.cell_centers(mesh)[:, 2]
    outside_cap = int((dead & (z_centre > z_cap)).sum())
    assert int(dead.sum()) == ms.degenerate, (int(dead.sum()), ms.degenerate)
    print(f"degenerate voxels: {ms.degenerate} ({outside_cap} outside the apex cap)")
    ok = active & ~dead
    cosine = np.abs((f0[ok] * f_closed[ok]).sum(axis=1)) / np.maximum(np.linalg.norm(f_closed[ok], axis=1), 1e-300)
    angle = np.degrees(np.arccos(np.clip(cosine, 0.0, 1.0)))
    print(f"angle between the generated fibres and the ellipsoid's closed form: mean {angle.mean():.2f} deg, max {angle.max():.2f} deg "
          f"({int(ok.sum())} voxels)")


if __name__ == "__main__":
    main()
