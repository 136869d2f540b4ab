#!/usr/bin/env python3
"""Three cell layers on a small slab -- endo-, mid- and epicardial TP06 parameter sets behind three markers, one
``DolfinMultiODESolver`` -- that saves frames of the potential AND of a cell state, and restarts from the last frame.

The reference keeps the states of ``DolfinMultiODESolver`` per marker and shows them through ``assign_all_states`` /
``states_to_dolfin`` (src/beat/odesolver.py:312-339): every marker's whole array through the host, once per state.  Here
``beat.FieldWriter`` takes ``(ode, "V")`` and ``(ode, "Ca_i")`` -- the row of whatever model a node runs -- expanded on the device
in one launch per frame; ``ode.function_to_state(key, function)`` is the way back.

    python demos/multi_state_output.py [--lx 6 --ly 3 --lz 1.5] [--dx 0.25] [--dt 0.05] [--T 4] [--out results_multi_state]

The directory ``<out>`` then holds ``V_<k>.npy``, ``Ca_i_<k>.npy`` and ``index.json``."""
import argparse

import _path  # noqa: F401
import numpy as np

import beat
from beat import grid as g
from beat.models import tp06

STATES = ("V", "Ca_i")


def build(args):
    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=args.lx, Ly=args.ly, Lz=args.lz, dx=args.dx)
    mesh = geo.mesh
    cond = beat.conductivities.default_conductivities("Niederer")
    C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
    time = g.Constant(mesh, 0.0)
    L, tol = 1.5, 1e-10
    corner = g.locate_entities(mesh, 3, lambda x: (x[0] <= L + tol) & (x[1] <= L + tol) & (x[2] <= L + tol))
    tags = g.meshtags(mesh, 3, corner, np.full(len(corner), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1, mesh_unit="mm",
                                           amplitude=50_000.0)
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ)
    V = g.functionspace(mesh, ("P", 1))
    z = mesh.node_coordinates(pad3=True)[:, 2]
    markers = g.Function(V)
    markers.x.array[:] = np.minimum(np.floor(3.0 * z / args.lz), 2.0)  # three layers across the wall
    keys = (0, 1, 2)
    params = {0: tp06.init_parameter_values(stim_amplitude=0.0, g_Ks=0.392), 1: tp06.init_parameter_values(stim_amplitude=0.0, g_Ks=0.098),
              2: tp06.init_parameter_values(stim_amplitude=0.0, g_Ks=0.392, g_to=0.294)}
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinMultiODESolver(
        v_ode=g.Function(V), v_pde=pde.state, markers=markers, num_states={k: len(ic) for k in keys},
        fun={k: tp06.generalized_rush_larsen for k in keys}, init_states={k: ic for k in keys}, parameters=params,
        v_index={k: tp06.state_index("V") for k in keys})
    return beat.MonodomainSplittingSolver(pde=pde, ode=ode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=float, default=6.0)
    ap.add_argument("--ly", type=float, default=3.0)
    ap.add_argument("--lz", type=float, default=1.5)
    ap.add_argument("--dx", type=float, default=0.25)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--T", type=float, default=4.0)
    ap.add_argument("--every-ms", type=float, default=1.0)
    ap.add_argument("--out", default="results_multi_state")
    args = ap.parse_args()
    solver = build(args)
    ode = solver.ode
    every, nsteps = max(1, int(round(args.every_ms / args.dt))), int(round(args.T / args.dt))
    with beat.FieldWriter(args.out, {name: (ode, name) for name in STATES}, stride=1, dtype="float64", format="npy") as w:
        for first in range(0, nsteps, every):
            last = min(first + every, nsteps)
            solver.solve((first * args.dt, last * args.dt), args.dt)
            w.write(last * args.dt)  # one expand launch and one pack launch; returns without waiting
    for t, stats in w.frames:
        print(f"t = {t:5.2f} ms   V in [{stats['V'][0]:8.3f}, {stats['V'][1]:8.3f}] mV   Ca_i in [{stats['Ca_i'][0]:.3e}, {stats['Ca_i'][1]:.3e}] mM")

    # a restart from the last frame: a fresh solver gets the other states as a checkpoint of the arrays would give them (the two
    # saved rows left at their initial values), then the two saved states from the frames through function_to_state
    k = len(w.frames) - 1
    fresh = build(args)
    V = fresh.ode.v_ode.function_space
    ic = tp06.init_state_values()
    for m in (0, 1, 2):
        stale = ode.values(m).copy()
        for name in STATES:
            stale[tp06.state_index(name)] = ic[tp06.state_index(name)]
        fresh.ode.set_values(m, stale)
    for name in STATES:
        f = g.Function(V, name=name)
        f.x.array[:] = np.load(f"{args.out}/{name}_{k}.npy").reshape(-1)
        fresh.ode.function_to_state(name, f)
    for m in (0, 1, 2):
        assert np.array_equal(fresh.ode.values(m), ode.values(m)), m
    print(f"restarted {V.mesh.num_nodes} nodes from frame {k} (t = {w.frames[k][0]:.2f} ms): the states of the fresh solver equal the first run's")


if __name__ == "__main__":
    main()
