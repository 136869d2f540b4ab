#!/usr/bin/env python3
"""One timed process: the monitor kernel of a generated model on a resident state array (profiles/monitor_values.md).  Prints one
JSON line: the time of one launch, the bytes the pass needs -- 8 (states the selection loads + names) per node -- and the rate.

    python tools/monitor_values_bench.py [--ode tests/data/big_cell.ode] [--names I_0,dV_dt,dc_6_dt] [--nodes 4194304] [--per-node]

The states are ``_sample_states`` of 65 536 nodes repeated over the array; the first launches (compile, self-check, code object
load) are outside the five timed windows of about 0.4 s each."""
import argparse, ctypes as C, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
ap = argparse.ArgumentParser()
ap.add_argument("--ode", default=str(ROOT / "tests" / "data" / "big_cell.ode"))
ap.add_argument("--names", default="I_0,dV_dt,dc_6_dt")
ap.add_argument("--nodes", type=int, default=1 << 22)
ap.add_argument("--per-node", action="store_true")
args = ap.parse_args()
sys.path[:0] = [str(ROOT), str(ROOT / "fenicsx-beat_amd")]
import numpy as np
from beat._device import Context, StateArray
from beat.models import from_ode

model = from_ode(args.ode)
names = args.names.split(",")
ctx = Context.default()
n, block = args.nodes, 1 << 16
assert n % block == 0
sa = StateArray(ctx, model.num_states, n)
sa.rows.copy_(ctx.from_numpy(model._sample_states(block)).repeat(1, n // block))
out = StateArray(ctx, len(names), n)
p = model.init_parameter_values()
kw = dict(host_params=p)
if args.per_node:
    rows = ctx.from_numpy(np.repeat(p[:, None], block, axis=1)).repeat(1, n // block).contiguous()
    kw = dict(per_node=(C.c_void_p(rows.data_ptr()), n))


def launch():
    model.monitor_on_device(ctx, names, sa.ptr, n, sa.ld, 0.3, out.ptr, out.ld, **kw)


for _ in range(5):
    launch()
ctx.synchronize()
check = out.rows[:, :block].cpu().numpy()
ref = model.numpy_monitor(model._sample_states(block), 0.3, p, names)
err = float(model.monitor_error(check, ref).max())
t0 = time.perf_counter(); launch(); ctx.synchronize(); one = time.perf_counter() - t0
reps = int(min(5000, max(20, 0.4 / max(one, 1e-6))))
windows = []
for _ in range(5):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        launch()
    ctx.synchronize()
    windows.append((time.perf_counter() - t0) / reps * 1e3)
windows.sort()
(_, source, _), = model.monitor_sources(names)
loads = source.count("io.load(")
param_rows = source.count("= p[") if args.per_node else 0
bytes_ = 8 * (loads + len(names) + param_rows) * n
print(json.dumps({"ode": Path(args.ode).name, "names": names, "nodes": n, "per_node": args.per_node, "states_loaded": loads,
                  "of_states": model.num_states, "param_rows_loaded": param_rows, "reps": reps, "ms_median": round(windows[2], 4),
                  "ms_min": round(windows[0], 4), "ms_max": round(windows[-1], 4), "bytes_per_node": bytes_ // n,
                  "GBps_algorithmic": round(bytes_ / windows[2] / 1e6, 1), "max_error_vs_numpy": err}))
