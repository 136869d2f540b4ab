#!/usr/bin/env python3
"""One timed process: the per-sample time of ``LeadRecorder.record()`` or of ``ecg.solve()`` + L x ``assemble_scalar``
(profiles/lead_recorder.md).  Prints one JSON line.

    python tools/lead_recorder_bench.py --grid demo|box --L 2|9 --mode record|ecg [--tree DIR] [--cells 256] [--tag NAME]

``--tree``: the checkout whose package is timed (default: this one; a checkout of the parent commit for ``--mode ecg``);
``BEAT_HIP_LIBRARY`` chooses the library (a -DBEAT_LEADS_Q_NT=1 build beside the shipped one).  ``--grid box`` lumps the electrodes'
weights (kernel at the node times the nodal volume) instead of integrating them, to keep the set-up short: neither timed call
depends on their values."""
import argparse, json, sys, time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
ap.add_argument("--grid", default="demo")
ap.add_argument("--L", type=int, default=9)
ap.add_argument("--mode", default="record")
ap.add_argument("--tag", default="")
ap.add_argument("--cells", type=int, default=256)
args = ap.parse_args()
tree = Path(args.tree).resolve()
sys.path[:0] = [str(tree), str(tree / "fenicsx-beat_amd")]
import numpy as np
import beat
from beat import grid as g
import beat.ecg as becg

assert Path(beat.__file__).resolve().is_relative_to(tree), beat.__file__
if args.grid == "demo":
    L3, cells = (10.0, 5.0, 2.0), (20, 10, 4)
else:
    L3, cells = (25.6, 25.6, 25.6), (args.cells,) * 3

    def lumped(mesh, cells_, spatial):  # node value x nodal volume: set-up only, the timed calls do not depend on the values
        x = mesh.node_coordinates(pad3=True).T
        return np.asarray(spatial.evaluate(x), dtype=np.float64) * float(np.prod(mesh.h))

    becg.assemble_weights = lumped
mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array(L3)], list(cells))
V = g.functionspace(mesh, ("P", 1))
v = g.Function(V)
v.interpolate(lambda x: -85.0 + 110.0 / (1.0 + np.exp((x[0] + 0.5 * x[1] + 0.3 * x[2] - 0.6 * L3[0]) / 0.4)))
M = np.diag([1.3e-4, 1.7e-5, 1.7e-5])
ecg = beat.ECGRecovery(v=v, sigma_b=1.0, C_m=0.01, M=M)
pts = [(-8.0, L3[1] + 8, L3[2] + 6), (L3[0] + 8, L3[1] + 8, L3[2] + 6), (L3[0] + 6, -10.0, -4.0)] + \
      [(L3[0] * (k + 0.5) / 6, -1.0 + 0.4 * k, L3[2] + 3.0 + 0.2 * k) for k in range(6)]
pts = pts[: args.L]
ctx = ecg._ctx
t_setup = time.perf_counter()
if args.mode == "record":
    rec = beat.LeadRecorder(ecg, pts, capacity=1 << 16)
    sample = rec.record
else:
    forms = [ecg.eval(p) for p in pts]

    def sample():
        ecg.solve()
        return [becg.assemble_scalar(f) for f in forms]
ctx.synchronize()
t_setup = time.perf_counter() - t_setup
for _ in range(5):
    sample()
ctx.synchronize()
t0 = time.perf_counter(); sample(); ctx.synchronize(); one = time.perf_counter() - t0
reps = int(min(5000, max(20, 0.4 / max(one, 1e-6))))
windows = []
for _ in range(5):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        sample()
    ctx.synchronize()
    windows.append((time.perf_counter() - t0) / reps * 1e6)
windows.sort()
n = mesh.num_nodes
out = {"tag": args.tag, "mode": args.mode, "grid": args.grid, "nodes": n, "L": args.L, "reps": reps, "us_per_sample_median": round(windows[2], 2),
       "us_min": round(windows[0], 2), "us_max": round(windows[-1], 2), "setup_s": round(t_setup, 2)}
if args.mode == "record":
    bytes_ = (args.L + (args.L + 7) // 8) * 8 * n
    out["GBps_algorithmic"] = round(bytes_ / windows[2] / 1e3, 1)
    out["value0"] = float(rec.values()[-1][0])
else:
    out["ksp_its"] = ecg.ksp.iterations
    out["value0"] = float(sample()[0])
print(json.dumps(out))
