#!/usr/bin/env python3
"""What a state row of DolfinMultiODESolver costs as a field of the grid: three TP06 markers on a dense n^3-node box, by thirds along x
(grid-spanning layout, BEAT_MULTI_COMPACT=0, and compact, =1) and as a checkerboard (every wave meets all three classes: the worst
case of the kernel's class loop), each in a solver of its own, one after the other in one process.

Per case: the expand launch (beat_rows_to_fields through the solver's plan) for 1, 4 and 8 rows, with plain and with non-temporal
loads, timed by events around ``--launches`` launches, the median of ``--reps`` such timings; beside it, timed the same way in the
same run, beat_copy of as many doubles as the launch moves.  Bytes of the expand: 1 per node for the class, 4 for the position
where there is one, 16 per field and marked node; of the copy 16 per double.  Then, for ONE state, the route without the kernel:
``values(marker)[k]`` for every marker, assembled on the host and assigned to a function (wall clock, the device idle before and
after), against ``states_to_functions([k])`` timed the same way.

    python tools/bench_rows.py [--n 257] [--reps 9] [--launches 10] [--md out.md]"""
import argparse
import ctypes as C
import os
import sys
import time as wallclock
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "fenicsx-beat_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

CASES = (("thirds, grid-spanning", "thirds", "0"), ("thirds, compact", "thirds", "1"), ("checkerboard, grid-spanning", "checker", "0"),
         ("checkerboard, compact", "checker", "1"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def build(n, pattern, compact):
    import beat
    from beat import grid as g
    from beat.models import tp06

    os.environ["BEAT_MULTI_COMPACT"] = compact
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.full(3, 1.0)], [n - 1] * 3)
    V = g.functionspace(mesh, ("P", 1))
    iz, iy, ix = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    marker_arr = (np.minimum(ix * 3 // n, 2) if pattern == "thirds" else (ix + iy + iz) % 3).ravel().astype(np.float64)
    markers = g.Function(V)
    markers.x.array[:] = marker_arr
    keys = (0, 1, 2)
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinMultiODESolver(
        v_ode=g.Function(V), v_pde=g.Function(V), markers=markers, num_states={k: len(ic) for k in keys},
        fun={k: tp06.generalized_rush_larsen for k in keys}, init_states={k: ic * (1.0 + 0.001 * k) for k in keys},
        parameters={k: tp06.init_parameter_values(stim_amplitude=0.0) for k in keys}, v_index={k: tp06.state_index("V") for k in keys})
    assert ode._marked and (ode._node_idx is not None) == (compact == "1")
    return ode, V


def timed(ctx, fn, reps, launches):
    """ms per launch: median, min, max over ``reps`` timings of ``launches`` launches each (after a warm-up of as many)."""
    import torch

    for _ in range(launches):
        fn()
    ctx.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ctx.stream)
        for _ in range(launches):
            fn()
        b.record(ctx.stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) / launches)
    return median(ts), min(ts), max(ts)


def case(label, pattern, compact, args, out, say):
    import torch

    from beat import _hip, grid as g

    say(f"{label}: building")
    ode, V = build(args.n, pattern, compact)
    ctx = ode._ctx
    n = ode.markers.x.array.size
    plan = ode._rows_plan()
    has_pos = plan._pos is not None
    fields = [g.Function(V) for _ in range(8)]
    # the values are right before they are timed
    got = ode.states_to_functions([13], [fields[0]])[0]
    want = np.zeros(n)
    for m in (0, 1, 2):
        want[ode._inds[m]] = ode.values(m)[13]
    assert np.array_equal(np.asarray(got.x.array), want)
    out.append(f"### {label}: {n:,} nodes, all marked, {'an int32 position per node' if has_pos else 'no positions'}\n")
    out.append("| rows | loads | expand ms: median (min .. max) | bytes | GB/s | beat_copy of as many doubles, ms | copy GB/s | expand / copy rate |")
    out.append("|---:|---|---:|---:|---:|---:|---:|---:|")
    src, dst = ctx.zeros(8 * n), ctx.zeros(8 * n)
    for nf in (1, 4, 8):
        rows = [[r] * 3 for r in range(nf)]
        flds = [f.writable_field() for f in fields[:nf]]
        cp = timed(ctx, lambda: _hip.check(ctx.lib.beat_copy(ctx.handle, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nf * n)),
                   args.reps, args.launches)
        copy_rate = 16 * nf * n / cp[0] / 1e6
        for nt in (False, True):
            ex = timed(ctx, lambda: plan.expand(rows, flds, None, nt), args.reps, args.launches)
            nbytes = n * (1 + (4 if has_pos else 0)) + 16 * nf * n
            rate = nbytes / ex[0] / 1e6
            out.append(f"| {nf} | {'non-temporal' if nt else 'plain'} | {ex[0]:.4f} ({ex[1]:.4f} .. {ex[2]:.4f}) | {nbytes / 1e6:.0f} MB | {rate:.0f} | "
                       f"{cp[0]:.4f} | {copy_rate:.0f} | {rate / copy_rate:.2f} |")
    del src, dst
    out.append("")
    # one state: through the host, as the solver did it without the kernel, against the device route -- wall clock, device idle around
    def host_route():
        arr = np.asarray(fields[0].x.array).copy()
        for m in (0, 1, 2):
            arr[ode._inds[m]] = ode.values(m)[13, :]
        fields[0].x.array[:] = arr

    def device_route():
        ode.states_to_functions([13], [fields[0]])

    walls = {}
    for name, fn, reps in (("host", host_route, 2), ("device", device_route, 20)):
        fn()
        ctx.synchronize()
        ts = []
        for _ in range(reps):
            tic = wallclock.perf_counter()
            fn()
            ctx.synchronize()
            ts.append(1e3 * (wallclock.perf_counter() - tic))
        walls[name] = median(ts)
    out.append(f"One state into a function: through the host (values(marker)[k] per marker, assembled, assigned) {walls['host']:.1f} ms; "
               f"states_to_functions {walls['device']:.3f} ms with the host's share and the wait: {walls['host'] / walls['device']:.0f} x.\n")
    del ode, fields, plan
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=257, help="nodes per axis")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    out = []

    def say(msg):
        print(msg, file=sys.stderr, flush=True)

    for label, pattern, compact in CASES:
        case(label, pattern, compact, args, out, say)
        if args.md:  # (what is measured so far is kept)
            Path(args.md).write_text("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
