#!/usr/bin/env python3
"""A cell model cut in two, both halves on the device: gotran models are routinely split -- an electrophysiology half and a
mechanics half -- and each half then MISSES a few variables the other one owns.  ``beat.models.from_ode(path, missing=...)`` makes
a device kernel of such a half: the missing variables are input rows behind its states, read per node and never advanced.  Here
the small excitable-cell model of the test suite is run three ways on the nodes of a small slab (cells only, no diffusion):

  whole     tests/data/small_cell.ode, one ``DolfinODESolver``;
  split     tests/data/split_membrane.ode (misses ``ca``) and tests/data/split_calcium.ode (misses ``V, m, h``) as two solvers that
            hand each other their step-start rows ON THE DEVICE before every step: ``state_to_function`` copies a state row into
            the other solver's ``missing_function`` -- the function whose field IS the kernel's input row.  No field visits the host.

Both halves miss only STATES of the other, so a GRL1 (or forward-Euler) step of the two is mathematically one step of the whole
model, and the two runs differ by rounding alone.  That would NOT hold if a half missed an INTERMEDIATE that depends on one of
its own states (say the membrane half took ``i_out`` from elsewhere): the self-derivative J_kk treats a missing variable as a
constant, so such a split drops a term of J_kk and is another scheme.  Under GRL2 a missing variable is held at its step-start
value through both stages: the step is first order in it.

    python demos/split_cell.py [--dx 0.5] [--steps 40] [--dt 0.05] [--scheme generalized_rush_larsen]"""
import argparse

import _path  # noqa: F401
import numpy as np

import beat
from beat import grid as g
from beat.models import from_ode

DATA = _path.ROOT / "tests" / "data"


def build(V, scheme, v0):
    """(whole, membrane, calcium) solvers on the space ``V``, the potential starting at ``v0`` per node."""
    def solver(model, init, v_index, **kw):
        return beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=model, init_states=init,
                                              parameters=model.init_parameter_values(), num_states=model.num_states, v_index=v_index, **kw)

    n = len(v0)
    whole = from_ode(DATA / "small_cell.ode", scheme=scheme)
    mem = from_ode(DATA / "split_membrane.ode", scheme=scheme, missing=["ca"])
    cal = from_ode(DATA / "split_calcium.ode", scheme=scheme, missing=["V", "m", "h"], missing_ranges={"V": (-100.0, 60.0)})
    y = np.repeat(whole.init_state_values()[:, None], n, axis=1)
    y[whole.state_index("V")] = v0
    rows = [whole.state_index(s) for s in mem.state_names]
    ca = whole.state_index("ca")
    return (solver(whole, y.copy(), whole.state_index("V")),
            solver(mem, y[rows].copy(), mem.state_index("V"), missing_variables=y[[ca]].copy(), num_missing_variables=1),
            solver(cal, y[[ca]].copy(), 0, missing_variables=y[[whole.state_index(s) for s in cal.missing_names]].copy(),
                   num_missing_variables=3))


def exchange(mem, cal) -> None:
    """Each half's step-start rows into the other's input rows: device copies."""
    for name in cal.fun.missing_names:
        mem.state_to_function(name, cal.missing_function(name))
    cal.state_to_function("ca", mem.missing_function("ca"))


def run(whole, mem, cal, steps, dt) -> None:
    t = 0.0
    for _ in range(steps):
        whole.step(t, dt)
        exchange(mem, cal)
        mem.step(t, dt)
        cal.step(t, dt)
        t += dt


def difference(whole, mem, cal):
    """(largest |split - whole| relative to each state's range over the nodes, the whole model's (5, N) states)."""
    w = np.asarray(whole.values)
    names = whole.fun.state_names
    s = np.empty_like(w)
    s[[names.index(nm) for nm in mem.fun.state_names]] = np.asarray(mem.values)
    s[names.index("ca")] = np.asarray(cal.values)[0]
    span = np.maximum(w.max(axis=1) - w.min(axis=1), 1e-300)
    return float((np.abs(s - w).max(axis=1) / span).max()), w


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dx", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--scheme", default="generalized_rush_larsen")
    args = ap.parse_args(argv)

    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=6.0, Ly=3.0, Lz=1.5, dx=args.dx)
    V = g.functionspace(geo.mesh, ("P", 1))
    x = np.asarray(V.tabulate_dof_coordinates())[:, 0]
    whole, mem, cal = build(V, args.scheme, -84.0 + 30.0 * x / x.max())  # (rest at one end, 30 mV above it at the other)
    run(whole, mem, cal, args.steps, args.dt)
    diff, w = difference(whole, mem, cal)
    v = w[whole.fun.state_index("V")]
    print(f"{len(x)} cells, {args.steps} steps of {args.dt} ms ({args.scheme}): V in [{v.min():.2f}, {v.max():.2f}]")
    print(f"split against whole: largest difference {diff:.3e} of a state's range")
    print("status OK" if np.isfinite(w).all() and np.isfinite(diff) else "status FAILED")
    return diff, w, (whole, mem, cal)


if __name__ == "__main__":
    main()
