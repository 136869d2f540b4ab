#!/usr/bin/env python3
"""Activation, repolarisation and APD maps of a paced slab (TP06, S1 stimulus in a 1.5 mm corner cube), recorded on the device.

The reference's tissue demos build their activation map on the host, from the whole potential after every step
(demos/irksome_model_gotranx.py:251-254); here ``beat.EventRecorder`` keeps the maps in device memory and nothing but the
solve's record crosses to the host -- the pass that updates them is the one that completes the potential after the diffusion
solve (for which the loop waits once per step).

    python demos/activation_map.py [--lx 20 --ly 7 --lz 3] [--dx 0.25] [--dt 0.05] [--T 40] [--host-loop]

Prints a few percentiles of every map over the nodes that have one.  ``--host-loop`` computes the activation map the reference's
way as well and compares."""
import argparse
import time as wallclock

import _path  # noqa: F401
import numpy as np

import beat
from beat import grid as g
from beat.models import tp06


def build(args):
    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=args.lx, Ly=args.ly, Lz=args.lz, dx=args.dx)
    mesh = geo.mesh
    cond = beat.conductivities.default_conductivities("Niederer")
    C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
    time = g.Constant(mesh, 0.0)
    L, tol = 1.5, 1e-10
    cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= L + tol) & (x[1] <= L + tol) & (x[2] <= L + tol))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                           mesh_unit="mm", amplitude=50_000.0)
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ)
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinODESolver(
        v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
        init_states=ic, parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(ic),
        v_index=tp06.state_index("V"))
    return beat.MonodomainSplittingSolver(pde=pde, ode=ode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=float, default=20.0)
    ap.add_argument("--ly", type=float, default=7.0)
    ap.add_argument("--lz", type=float, default=3.0)
    ap.add_argument("--dx", type=float, default=0.25)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--T", type=float, default=40.0)
    ap.add_argument("--host-loop", action="store_true", help="also build the activation map as the reference does (read the "
                    "potential after every step) and compare")
    args = ap.parse_args()
    solver = build(args)
    # activation: first time v > 0 mV (the Niederer benchmark's rule); repolarisation: back below -70 mV
    rec = beat.EventRecorder(solver.pde.state, 0.0, repolarisation_threshold=-70.0,
                             maps=("activation", "repolarisation", "apd", "dvdt_max", "v_max"), compare=">")
    tic = wallclock.perf_counter()
    solver.solve((0.0, args.T), args.dt, recorder=rec)
    maps = {name: np.asarray(getattr(rec, name).x.array) for name in rec.maps}  # (the first read waits for the device)
    wall = wallclock.perf_counter() - tic
    n = maps["activation"].size
    nsteps = int(round(args.T / args.dt))
    print(f"{n} nodes, {nsteps} steps of {args.dt} ms in {wall:.2f} s ({wall / max(nsteps, 1) * 1e3:.2f} ms/step), "
          f"{rec.fused_passes} observations fused with the potential's update")
    units = {"activation": "ms", "repolarisation": "ms", "apd": "ms", "dvdt_max": "mV/ms", "v_max": "mV"}
    for name, a in maps.items():
        ok = np.isfinite(a)
        line = f"  {name:15s} {ok.sum():8d} nodes"
        if ok.any():
            p = np.percentile(a[ok], [0, 25, 50, 75, 100])
            line += "   min / 25 % / median / 75 % / max: " + " / ".join(f"{v:.2f}" for v in p) + f" {units[name]}"
        print(line)
    if args.host_loop:
        ref = build(args)
        tact = np.full(n, np.nan)
        t = 0.0
        tic = wallclock.perf_counter()
        while t + args.dt < args.T + 1e-12:
            ref.step((t, t + args.dt))
            t = t + args.dt
            v = np.asarray(ref.pde.state.x.array)
            crossed = (v > 0.0) & np.isnan(tact)
            tact[crossed] = t
        wall_host = wallclock.perf_counter() - tic
        same = np.array_equal(tact, maps["activation"], equal_nan=True)
        print(f"host loop: {wall_host:.2f} s ({wall_host / max(nsteps, 1) * 1e3:.2f} ms/step), activation map "
              f"{'identical' if same else 'DIFFERENT'}")
        if not same:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
