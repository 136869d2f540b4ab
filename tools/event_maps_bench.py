#!/usr/bin/env python3
"""What the event maps cost per step of bench.py's workload (n^3 TP06, dt 0.01 ms, the PDE's theta 0.5, the same initial bump), and
what they replace.  The splitting's own theta stays at its default 1 (one ionic step, one solve per step): only then is the update
that a recorder takes over the one the next ionic kernel would have applied, and */fused against */2pass the comparison meant.  One process, one state array, the variants one after another on the same memory:

  none        step() and nothing else (the ionic kernel applies the deferred update of the potential)
  act/fused   step() + EventRecorder(maps=("activation",)).observe: the pass is the deferred update as well
  act/2pass   the same with flush_pending() first: beat_pde_x_flush, then beat_field_events
  all/fused   all six maps
  all/2pass
  host loop   the reference demo's way (demos/irksome_model_gotranx.py:251-254): read pde.state.x.array after every step, mask

    python tools/event_maps_bench.py [--n 256] [--steps 40] [--warmup 10] [--host-steps 5]

Prints one line per variant (ms per step: wall time over the block of steps with one synchronisation at its end, median of
--repeats blocks) and one JSON line at the end; the event pass alone is timed with HIP events."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "fenicsx-beat_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-8)
    args = ap.parse_args()
    import torch

    import beat
    import bench
    from beat import grid as g
    from beat.models import tp06

    n = args.n
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.full(3, (n - 1) * bench.H)], [n - 1] * 3)
    time_c = g.Constant(mesh, 0.0)
    pde = beat.MonodomainModel(time=time_c, mesh=mesh, M=bench.conductivity(), C_m=bench.C_M,
                               params={"theta": bench.THETA, "petsc_options": {"ksp_rtol": args.rtol, "ksp_atol": 1e-50, "ksp_max_it": 500}})
    ic, params, v_index = bench.tp06_defaults()
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state,
                                         fun=tp06.generalized_rush_larsen, init_states=ic, parameters=params, num_states=len(ic),
                                         v_index=v_index)
    solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    ctx, ops = pde._ctx, pde._ops
    bench.init_states(ctx, ode._dev.states, ic, v_index, n, mesh.slab, 1234)
    dt = bench.DT
    clock = {"t": 0.0}

    def advance(k, after=None):
        for _ in range(k):
            t0 = clock["t"]
            solver.step((t0, t0 + dt))
            clock["t"] = t0 + dt
            if after is not None:
                after(t0, t0 + dt)

    def measure(after=None, steps=args.steps):
        advance(args.warmup if after is None else 3, after)
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            tic = time.perf_counter()
            advance(steps, after)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - tic) / steps * 1e3)
        return sorted(out)[len(out) // 2]

    all_maps = tuple(beat.events.MAPS)
    # thresholds inside the bump's range, so that events happen during the timed steps
    rec_act = beat.EventRecorder(pde.state, -40.0, compare=">")
    rec_all = beat.EventRecorder(pde.state, -40.0, repolarisation_threshold=-60.0, maps=all_maps, compare=">")

    def two_pass(rec):
        def after(t0, t1):
            ops.flush_pending()
            rec.observe(t0, t1)
        return after

    results = {"n": n, "nodes": n**3, "steps": args.steps, "unit": "ms/step"}
    results["none"] = measure()
    for name, rec in (("act", rec_act), ("all", rec_all)):
        rec.fused_passes = 0
        results[name + "/fused"] = measure(rec.observe)
        results[name + "/fused_share"] = rec.fused_passes / (3 + args.repeats * args.steps)
        results[name + "/2pass"] = measure(two_pass(rec))
    results["none_again"] = measure()

    # the passes alone, by HIP events, on a potential that is complete
    ops.flush_pending()
    torch.cuda.synchronize()

    def pass_ms(fn, reps=20):
        evs = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]

    t = clock["t"]
    results["pass_act_ms"] = pass_ms(lambda: rec_act.observe(t, t + dt))
    results["pass_all_ms"] = pass_ms(lambda: rec_all.observe(t, t + dt))
    # rates over the bytes every node moves whatever happens (maps read on candidate events and stored on events come on top, up to
    # 16 and 56 B/node: profiles/event_maps.md), so lower bounds: v read (+ act_first where the node is above the threshold) ...
    results["pass_act_GBs_min"] = 8.0 * n**3 / results["pass_act_ms"] / 1e6
    # ... and v, v_prev read, v_prev written, dvdt_max and v_max read
    results["pass_all_GBs_min"] = 40.0 * n**3 / results["pass_all_ms"] / 1e6

    # the reference demo's loop
    tact = np.full(n**3, np.nan)

    def host(t0, t1):
        v = np.asarray(pde.state.x.array)
        crossed = (v > -40.0) & np.isnan(tact)
        tact[crossed] = t1

    args.repeats, keep = 1, args.repeats
    results["host_loop"] = measure(host, steps=args.host_steps)
    args.repeats = keep
    got = np.asarray(rec_act.activation.x.array)
    results["activated"] = int(np.isfinite(got).sum())
    for k, v in results.items():
        print(f"  {k:18s} {v:.4f}" if isinstance(v, float) else f"  {k:18s} {v}")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
