#!/usr/bin/env python3
"""A paced slab (TP06, S1 stimulus in a 1.5 mm corner cube) that SAVES as the reference's tissue demos do -- the potential and the
activation map once per millisecond of simulated time, and a progress line with the potential's extremes -- without the time loop
waiting for the copy or the disk.

The reference's ``save(t)`` (demos/niederer_benchmark.py:226-277, demos/slab.py:284-299) is ``vtx.write(t)``,
``io4dolfinx.write_function(..., solver.pde.state, time=t, name="v")`` and ``print(v.max(), v.min())`` on the thread that drives the
solver.  ``beat.FieldWriter`` takes the frame in one launch on the device, copies it on a stream of its own and writes it from a
thread of its own; the launch's pass over the field yields the extremes, so the progress line costs no copy.

    python demos/slab_output.py [--lx 20 --ly 7 --lz 3] [--dx 0.25] [--dt 0.05] [--T 20] [--out results_slab_output/slab]
                                [--stride 2] [--dtype float32] [--format vti]

Open ``<out>.pvd`` in ParaView (``--format npy``: the directory ``<out>`` with ``index.json``)."""
import argparse
import time as wallclock

import _path  # noqa: F401
from activation_map import build

import beat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lx", type=float, default=20.0)
    ap.add_argument("--ly", type=float, default=7.0)
    ap.add_argument("--lz", type=float, default=3.0)
    ap.add_argument("--dx", type=float, default=0.25)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--T", type=float, default=20.0)
    ap.add_argument("--out", default="results_slab_output/slab")
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float64"))
    ap.add_argument("--format", default="vti", choices=beat.output.FORMATS)
    ap.add_argument("--every-ms", type=float, default=1.0, help="simulated time between two frames")
    args = ap.parse_args()
    solver = build(args)
    rec = beat.EventRecorder(solver.pde.state, 0.0, compare=">")  # activation: first time v > 0 mV
    every = max(1, int(round(args.every_ms / args.dt)))
    nsteps = int(round(args.T / args.dt))
    tic = wallclock.perf_counter()
    with beat.FieldWriter(args.out, {"v": solver.pde.state, "activation": rec.activation}, stride=args.stride, dtype=args.dtype,
                          format=args.format) as w:
        shown = 0
        for first in range(0, nsteps, every):  # the reference's loop: advance an output interval, save(t)
            last = min(first + every, nsteps)
            solver.solve((first * args.dt, last * args.dt), args.dt, recorder=rec)
            w.write(last * args.dt)  # returns without waiting for the device
            for t, stats in w.frames[shown:]:  # (frames the writer's thread has finished by now; the rest after close)
                print(f"t = {t:7.2f} ms   v in [{stats['v'][0]:8.3f}, {stats['v'][1]:8.3f}] mV   "
                      f"activated by {stats['activation'][1]:6.2f} ms   non-finite: {stats['v'][2]}")
            shown = len(w.frames)
    for t, stats in w.frames[shown:]:
        print(f"t = {t:7.2f} ms   v in [{stats['v'][0]:8.3f}, {stats['v'][1]:8.3f}] mV   "
              f"activated by {stats['activation'][1]:6.2f} ms   non-finite: {stats['v'][2]}")
    wall = wallclock.perf_counter() - tic
    print(f"{solver.pde.state.x.array.size} nodes, {nsteps} steps of {args.dt} ms and {len(w.frames)} frames of shape {w.shape} "
          f"({args.dtype}) in {wall:.2f} s ({wall / max(nsteps, 1) * 1e3:.2f} ms/step)")


if __name__ == "__main__":
    main()
