#!/usr/bin/env python3
"""The slab of slab_ecg.py with nine electrodes around it and the ECG recorded at EVERY step, on the device
(``beat.ecg.LeadRecorder``): each electrode's lead field q = -(1/C_m) K Mass^-1 w is made once, a sample of all nine leads is
then one pass over the potential (lead = q . v) -- no mass solve per sample and no host round trip per electrode, which is why
slab_ecg.py samples once per millisecond.  Prints the limb leads I and II and the precordial lead V1 (against Wilson's central
terminal), one value per millisecond out of the recorded 1 / dt.

    python demos/ecg_leads.py [--dx 0.5] [--T 40] [--dt 0.05]"""
import argparse

import _path  # noqa: F401
import numpy as np

import beat
from beat import grid as g
from beat.models import tp06


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dx", type=float, default=0.5)
    ap.add_argument("--T", type=float, default=40.0)
    ap.add_argument("--dt", type=float, default=0.05)
    args = ap.parse_args(argv)
    Lx, Ly, Lz = 10.0, 5.0, 2.0
    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=Lx, Ly=Ly, Lz=Lz, dx=args.dx)
    mesh = geo.mesh
    cond = beat.conductivities.default_conductivities("Niederer")
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
    time = g.Constant(mesh, 0.0)
    cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 1.5 + 1e-10) & (x[1] <= 1.5 + 1e-10))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                           mesh_unit="mm", amplitude=50_000.0, duration=2.0)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ)
    y0 = tp06.init_state_values()
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state,
                                         fun=tp06.generalized_rush_larsen, init_states=y0,
                                         parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(y0),
                                         v_index=tp06.state_index("V"))
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    ecg = beat.ecg.ECGRecovery(v=pde.state, sigma_b=1.0, C_m=C_m, M=M)
    # a torso in miniature: the limb electrodes far from the slab, the precordial ones in an arc 3 mm above it
    electrodes = {"RA": (-8.0, Ly + 8.0, Lz + 6.0), "LA": (Lx + 8.0, Ly + 8.0, Lz + 6.0), "LL": (Lx + 6.0, -10.0, Lz - 6.0)}
    for k in range(6):
        a = np.pi * (k + 0.5) / 6.0
        electrodes[f"V{k + 1}"] = (Lx / 2 - (Lx / 2 + 2.0) * np.cos(a), Ly / 2 - 1.0 + 0.4 * k, Lz + 3.0 * np.sin(a) + 1.0)
    rec = beat.ecg.LeadRecorder(ecg, electrodes)
    solver.solve((0.0, args.T), args.dt, recorder=rec)
    values = rec.values()
    leads = rec.leads12()
    every = max(1, int(round(1.0 / args.dt)))
    v = np.asarray(pde.state.x.array)
    print(f"{mesh.num_nodes} nodes, {len(rec)} steps of {args.dt} ms, {len(electrodes)} electrodes sampled at every step "
          f"({8 * len(electrodes) * mesh.num_nodes / 1e6:.2f} MB of lead fields); v in [{v.min():.2f}, {v.max():.2f}] mV")
    for name, trace in (("I", leads.I), ("II", leads.II), ("V1", leads.V1_)):
        print(f"lead {name}, one value per ms:")
        print("  " + " ".join(f"{x:8.4f}" for x in trace[every - 1 :: every]))
    return leads, values


if __name__ == "__main__":
    main()
