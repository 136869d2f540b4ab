#!/usr/bin/env python3
"""Currents across a wave front, straight off the device: a gotranx-generated module has ``monitor_values(t, states, parameters)``
for the named intermediates of its ``.ode`` file -- the ionic currents, the fluxes, the ``d<state>_dt`` -- and users plot I_Na or
I_CaL from it.  Here the model is a device kernel (``beat.models.from_ode``) and its states never leave the GPU, so the values are
evaluated there: ``DolfinODESolver.monitor(names, t)`` runs one read-only kernel over the resident state array and returns one
function per name.  The small excitable-cell model of the test suite on a slab with a stimulated corner; after a few steps the
fast inward current ``i_in`` and the pump flux ``j_pump`` are printed as min / max over the nodes.

    python demos/monitor_currents.py [--ode my_model.ode] [--names i_in,j_pump] [--dx 0.25] [--steps 60] [--dt 0.05]"""
import argparse
from pathlib import Path

import _path  # noqa: F401
import numpy as np

import beat
from beat import grid as g
from beat.models import from_ode


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ode", default=str(_path.ROOT / "tests" / "data" / "small_cell.ode"))
    ap.add_argument("--names", default="i_in,j_pump")
    ap.add_argument("--dx", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.05)
    args = ap.parse_args(argv)

    model = from_ode(args.ode)
    names = args.names.split(",")
    v_name = model.v_name or model.state_names[0]
    print(f"{Path(args.ode).name}: {len(model.monitor_names)} values can be monitored: {', '.join(model.monitor_names)}")
    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=6.0, Ly=3.0, Lz=1.5, dx=args.dx)
    mesh = geo.mesh
    time = g.Constant(mesh, 0.0)
    cond = beat.conductivities.default_conductivities("Niederer")
    cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 1.5 + 1e-10) & (x[1] <= 1.5 + 1e-10) & (x[2] <= 1.5 + 1e-10))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1, mesh_unit="mm",
                                           amplitude=50_000.0, duration=2.0)
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01, dx=I_s.dZ)
    no_stim = {k: 0.0 for k in model.parameter_names if k in ("stim_amplitude", "i_Stim_Amplitude")}
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state, fun=model,
                                         init_states=model.init_state_values(), parameters=model.init_parameter_values(**no_stim),
                                         num_states=model.num_states, v_index=model.state_index(v_name))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    t = 0.0
    for _ in range(args.steps):
        solver.step((t, t + args.dt))
        t += args.dt
    fields = ode.monitor(names, t)  # on the device; the functions are read below
    v = np.asarray(pde.state.x.array)
    print(f"{mesh.num_nodes} nodes after {args.steps} steps (t = {t:.2f} ms): {v_name} in [{v.min():.2f}, {v.max():.2f}]")
    out = {}
    for name, f in zip(names, fields):
        a = np.asarray(f.x.array)
        out[name] = a
        print(f"  {name:>10s} in [{a.min():.6g}, {a.max():.6g}]  (node of the minimum: {int(a.argmin())}, of the maximum: {int(a.argmax())})")
    return out, v, solver


if __name__ == "__main__":
    main()
