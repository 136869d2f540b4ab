#!/usr/bin/env python3
"""The ionic launch of a generated model under GRL1 and under GRL2, side by side: median over event-timed launches after two warm-up
launches (the method of tools/bench_kernels.py), the two schemes alternating so that both see the same clocks.  GRL1's generated
source is what it was before GRL2 existed (tests/test_grl2_cpu.py pins it), so its time is the baseline.

    python tools/bench_grl2.py [file.ode ...] [--n 16777216] [--reps 15] [--json out.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
SCHEMES = ("generalized_rush_larsen", "generalized_rush_larsen_2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ode", nargs="*", default=[str(ROOT / "tests" / "data" / "small_cell.ode")])
    ap.add_argument("--n", type=int, default=256**3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    from beat import telemetry
    from beat._device import Context
    from beat.models import from_ode
    from beat.odesolver import _DeviceODE

    ctx = Context.default()
    results = []
    for path in args.ode:
        odes, first = {}, None
        for scheme in SCHEMES:
            model = from_ode(path, scheme=scheme)
            ode = _DeviceODE(ctx, model, model.num_states, args.n, 0, model.init_parameter_values(), telemetry.NullMonitor())
            ode.set_initial(model.init_state_values())
            if model.v_name:  # the same spread of potentials under both schemes
                row = ode.states.rows[model.state_index(model.v_name)]
                if first is None:
                    first = row + 40.0 * torch.rand(args.n, dtype=torch.float64, device=row.device)
                row.copy_(first)
            odes[scheme] = ode
        first = None
        for ode in odes.values():
            for _ in range(2):
                ode.step(0.0, args.dt)
        torch.cuda.synchronize()
        events = {s: [] for s in SCHEMES}
        for _ in range(args.reps):
            for s in SCHEMES:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                odes[s].step(0.0, args.dt)
                b.record()
                events[s].append((a, b))
        torch.cuda.synchronize()
        ms = {s: sorted(a.elapsed_time(b) for a, b in events[s]) for s in SCHEMES}
        med = {s: ms[s][len(ms[s]) // 2] for s in SCHEMES}
        model = odes[SCHEMES[0]].model
        finite = all(bool(torch.isfinite(o.states.rows).all()) for o in odes.values())
        out = {"file": Path(path).name, "states": model.num_states, "nodes": args.n, "reps": args.reps,
               "grl1_ms": med[SCHEMES[0]], "grl2_ms": med[SCHEMES[1]], "ratio": med[SCHEMES[1]] / med[SCHEMES[0]],
               "grl1_min_ms": ms[SCHEMES[0]][0], "grl2_min_ms": ms[SCHEMES[1]][0],
               "grl1_TBps": 16.0 * model.num_states * args.n / med[SCHEMES[0]] / 1e9, "grl2_TBps": 16.0 * model.num_states * args.n / med[SCHEMES[1]] / 1e9,
               "finite": finite}
        print(json.dumps(out), flush=True)
        results.append(out)
        del odes
    if args.json:
        Path(args.json).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
