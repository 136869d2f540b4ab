#!/usr/bin/env python3
"""What saving a field costs the time loop: the benchmark's workload (bench.py: TP06 on an n^3 box, dt = 0.01 ms, public API), saved
at the reference demos' cadence -- once per millisecond of simulated time, every 100th step -- in four variants that alternate in
one process on one build:

  (a) no output
  (b) beat.io.write_function(dir, pde.state, time=t, name="v") as it stands: flush, synchronous fp64 copy, np.save on the loop's thread
  (c) beat.FieldWriter at stride 2 / fp32 (.vti)
  (d) beat.FieldWriter at stride 1 / fp64 (.vti)

ms/step = wall time of the loop (its last step complete on the device) over its steps; what ``close()`` then still waits for is
given beside it.  Then the pack kernel alone (events around beat_snap_enqueue's launch, the copy runs on another stream) beside
one read of a field of that size by the library's streaming probe (beat_stream_probe mode 1, as tools/stream_probe.py times it).

    python tools/bench_output.py [--sizes 256 512] [--reps 3] [--frames 2] [--every 100] [--md out.md]"""
import argparse
import ctypes as C
import shutil
import sys
import tempfile
import time as wallclock
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "fenicsx-beat_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def build(n, rtol):
    """bench.py's public-API solver on an n^3 box, with its initial state."""
    import bench
    import beat
    from beat import grid as g
    from beat.models import tp06

    ic, params, v_index = bench.tp06_defaults()
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.full(3, (n - 1) * bench.H)], [n - 1] * 3)
    pde = beat.MonodomainModel(time=g.Constant(mesh, 0.0), mesh=mesh, M=bench.conductivity(), C_m=bench.C_M,
                               params={"theta": bench.THETA, "petsc_options": {"ksp_rtol": rtol, "ksp_atol": 1e-50, "ksp_max_it": 500,
                                                                               "ksp_guess_order": -1}})
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state,
                                         fun=tp06.generalized_rush_larsen, init_states=ic, parameters=params, num_states=len(ic),
                                         v_index=v_index)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    bench.init_states(pde._ctx, ode._dev.states, ic, v_index, n, mesh.slab, 1234, n)
    return solver, bench.DT


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def loop_variants(solver, dt, args, out, say):
    import beat

    ctx = solver.pde._ctx
    t = [0.0]

    def run(variant, nsteps):
        """(ms per step of the loop, seconds close() still took, bytes on disk)"""
        work = Path(tempfile.mkdtemp(prefix=f"beat_out_{variant}_", dir=args.tmp))
        writer = None
        if variant == "c":
            writer = beat.FieldWriter(work / "run", {"v": solver.pde.state}, stride=2, dtype="float32", every=args.every, time=lambda: t[0])
        elif variant == "d":
            writer = beat.FieldWriter(work / "run", {"v": solver.pde.state}, stride=1, dtype="float64", every=args.every, time=lambda: t[0])
        ctx.synchronize()
        tic = wallclock.perf_counter()
        for k in range(nsteps):
            solver.step((t[0], t[0] + dt))
            t[0] += dt
            if writer is not None:
                writer.record()
            elif variant == "b" and (k + 1) % args.every == 0:
                beat.io.write_function(work / "chk", solver.pde.state, time=t[0], name="v")
        ctx.synchronize()
        loop = wallclock.perf_counter() - tic
        tic = wallclock.perf_counter()
        if writer is not None:
            writer.close()
        drain = wallclock.perf_counter() - tic
        size = sum(f.stat().st_size for f in work.rglob("*") if f.is_file())
        shutil.rmtree(work, ignore_errors=True)
        return 1e3 * loop / nsteps, drain, size

    run("a", 10)  # warm-up: kernels loaded, the guess's history filled
    nsteps = args.frames * args.every
    rows = {v: [] for v in "abcd"}
    for rep in range(args.reps):
        for variant in ("abcd" if rep % 2 == 0 else "dcba"):
            rows[variant].append(run(variant, nsteps))
            say(f"  rep {rep} ({variant}): {rows[variant][-1][0]:.3f} ms/step, close {rows[variant][-1][1]:.2f} s")
    names = {"a": "(a) no output", "b": "(b) beat.io.write_function", "c": "(c) FieldWriter stride 2 / fp32",
             "d": "(d) FieldWriter stride 1 / fp64"}
    out.append(f"| variant | ms/step: median (min .. max) of {args.reps} | per frame over (a), ms | close() after the loop, s | bytes per frame |")
    out.append("|---|---:|---:|---:|---:|")
    base = median([r[0] for r in rows["a"]])
    for v in "abcd":
        ms = [r[0] for r in rows[v]]
        per_frame = (median(ms) - base) * args.every
        out.append(f"| {names[v]} | {median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f}) | {per_frame:.1f} | "
                   f"{median([r[1] for r in rows[v]]):.2f} | {rows[v][0][2] // max(1, args.frames):,} |")


def kernel_times(solver, args, out):
    """The pack launch alone, by events on the compute stream, beside one read of the field by the streaming probe."""
    import torch

    from beat import _hip

    ctx = solver.pde._ctx
    lib = ctx.lib
    mesh = solver.pde.state.function_space.mesh
    field = solver.pde.state.field  # (complete: what was pending is applied)
    n = field.n

    def timed(fn):
        fn()
        ctx.synchronize()
        ts = []
        for _ in range(args.kernel_reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ctx.stream)
            fn()
            b.record(ctx.stream)
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return median(ts), min(ts), max(ts)

    reads = {}
    for policy, pname in ((0, "plain"), (1, "nt loads")):
        for unroll in (1, 4):
            for blocks in (2048, 8192):
                reads[(pname, unroll, blocks)] = timed(lambda: _hip.check(lib.beat_stream_probe(
                    ctx.handle, field.ptr, n & ~1, 1, policy, unroll, blocks, 0, 0)))
    best = min(reads, key=lambda k: reads[k][0])
    read_ms = reads[best][0]
    one = reads[("plain", 1, 2048)][0]
    out.append(f"One read of the field ({n * 8 / 1e9:.3f} GB) by beat_stream_probe mode 1: best {read_ms:.3f} ms = "
               f"{n * 8 / read_ms / 1e6:.0f} GB/s ({best[0]}, {best[1]} x 16 B in flight per lane, {best[2]} workgroups); "
               f"plain, one access in flight, 2048 workgroups: {one:.3f} ms = {n * 8 / one / 1e6:.0f} GB/s.")
    out.append("")
    out.append("| pack launch | loads | ms: median (min .. max) | field bytes read / time, GB/s | over the best one-read time |")
    out.append("|---|---|---:|---:|---:|")
    i64 = lambda v: (C.c_int64 * 3)(*v)  # noqa: E731
    shape = list(mesh.shape_global)
    for label, stride, dtype, stats in (("stride 2 / fp32, statistics", 2, 1, 1), ("stride 2 / fp32, no statistics", 2, 1, 0),
                                        ("stride 1 / fp64, statistics", 1, 0, 1), ("stride 1 / fp64, no statistics", 1, 0, 0)):
        for nt in (0, 1):
            snap = C.c_void_p()
            _hip.check(lib.beat_snap_create(ctx.handle, i64(shape), i64([0, 0, 0]), i64(shape), i64([stride] * 3), dtype, 1, 1, None,
                                            float("nan"), stats | (2 * nt), C.byref(snap)))
            ptrs = (C.c_void_p * 1)(field.ptr.value)
            slot = C.c_int()

            def fn():
                _hip.check(lib.beat_snap_enqueue(snap, ptrs, C.byref(slot)))

            fn_ms = []  # (the release waits for the copy: outside the events)
            for _ in range(args.kernel_reps + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.synchronize()
                a.record(ctx.stream)
                fn()
                b.record(ctx.stream)
                b.synchronize()
                _hip.check(lib.beat_snap_release(snap, slot.value))
                fn_ms.append(a.elapsed_time(b))
            fn_ms = fn_ms[1:]  # (the first loads the kernel)
            _hip.check(lib.beat_snap_destroy(snap))
            # bytes of the field the launch reads: all of it with the statistics, the lattice's rows (whole) without
            frac = 1.0 if stats else 1.0 / (stride * stride)
            m = median(fn_ms)
            out.append(f"| {label} | {'non-temporal' if nt else 'plain'} | {m:.3f} ({min(fn_ms):.3f} .. {max(fn_ms):.3f}) | "
                       f"{frac * n * 8 / m / 1e6:.0f} | {m / read_ms:.2f} x |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=2, help="frames per timed loop")
    ap.add_argument("--every", type=int, default=100, help="steps between two frames (dt = 0.01 ms: 100 = once per millisecond)")
    ap.add_argument("--kernel-reps", type=int, default=7)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--tmp", default=None, help="where the frames are written (default: the system's temporary directory)")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    import torch

    out = []

    def say(msg):
        print(msg, file=sys.stderr, flush=True)

    for n in args.sizes:
        free = torch.cuda.mem_get_info()[0]
        need = (19 + 16) * 8 * n**3 + 4 * 8 * n**3  # states, the solve's work fields, the writers' slots
        if free < need:
            out.append(f"## {n}^3: skipped, {free / 1e9:.0f} GB free on the device, about {need / 1e9:.0f} GB needed\n")
            continue
        say(f"{n}^3: building")
        solver, dt = build(n, args.rtol)
        out.append(f"## {n}^3 nodes, dt = {dt} ms, a frame every {args.every} steps, {args.frames} frames per loop\n")
        loop_variants(solver, dt, args, out, say)
        out.append("")
        kernel_times(solver, args, out)
        out.append("")
        del solver
        torch.cuda.empty_cache()
    text = "\n".join(out)
    print(text)
    if args.md:
        Path(args.md).write_text(text + "\n")


if __name__ == "__main__":
    main()
