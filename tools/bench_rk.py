#!/usr/bin/env python3
"""Implicit Runge-Kutta PDE step (beat.IrksomeMonodomainModel) on one GPU, beside the theta-rule model in the same process:
python tools/bench_rk.py [--n 256] [--steps 10]

Prints, as markdown lines and one JSON line at the end:
  - ms per PDE step at n^3 nodes for BackwardEuler(), RadauIIA(2), GaussLegendre(2) and MonodomainModel(theta=0.5)
    (bench.py's conductivity and C_m, dt = 0.01 ms, a Gaussian bump of potential, host-timed with the device synchronised);
  - time per iteration of the complex COCG solve, of its real instantiation and of the theta-rule's Jacobi-PCG
    (a fixed number of iterations: rtol = 0), HIP-event timed.
Profile the complex stencil kernel with rocprofv3 --kernel-trace --stats -- python tools/bench_rk.py --only iters."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default="", help="'steps' or 'iters'")
    args = ap.parse_args()
    import torch

    import beat
    import bench
    from beat import butcher, grid as g

    n, dt, C_m = args.n, 0.01, bench.C_M
    h = 0.1
    L = np.array([(n - 1) * h] * 3)
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), L], [n - 1] * 3)
    M = bench.conductivity()
    bump = lambda p: -85.0 + 100.0 * np.exp(-((p[0] - 0.5 * L[0]) ** 2 + (p[1] - 0.5 * L[1]) ** 2 + (p[2] - 0.5 * L[2]) ** 2) / 4.0)  # noqa: E731
    out = {"n": n, "dt": dt}
    tol = {"petsc_options": {"ksp_rtol": 1e-8}}

    def run(model):
        model.state.interpolate(bump)
        if isinstance(model, beat.MonodomainModel):
            model.assign_previous()
        t0 = 0.0
        model.step((t0, t0 + dt))  # warm-up
        t0 += dt
        its = []
        torch.cuda.synchronize()
        tic = time.perf_counter()
        for _ in range(args.steps):
            if isinstance(model, beat.MonodomainModel):
                model.assign_previous()
            model.step((t0, t0 + dt))
            its.append(model.ksp.iterations)
            t0 += dt
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - tic) / args.steps, float(np.mean(its))

    if args.only in ("", "steps"):
        print(f"| method at {n}^3, dt {dt} ms | ms/step | iterations/step |")
        print("|---|---|---|")
        for name in ("theta=0.5", "BackwardEuler()", "RadauIIA(2)", "GaussLegendre(2)"):
            time_c = g.Constant(mesh, 0.0)
            if name.startswith("theta"):
                model = beat.MonodomainModel(time=time_c, mesh=mesh, M=M, C_m=C_m, params=dict(theta=0.5, **tol))
            else:
                model = beat.IrksomeMonodomainModel(time=time_c, mesh=mesh, M=M, C_m=C_m,
                                                    butcher_tableau=eval(name, vars(butcher)), params=tol)
            ms, it = run(model)
            out[name] = {"ms_per_step": round(ms, 3), "iterations_per_step": it}
            print(f"| {name} | {ms:.3f} | {it:.1f} |", flush=True)
            del model
            torch.cuda.empty_cache()

    if args.only in ("", "iters"):
        model = beat.IrksomeMonodomainModel(time=g.Constant(mesh, 0.0), mesh=mesh, M=M, C_m=C_m,
                                            butcher_tableau=butcher.RadauIIA(2))
        ops = model._ops
        rng = torch.Generator(device="cuda").manual_seed(1)
        br, bi, xr, xi = (ops.field(k) for k in ("b_br", "b_bi", "b_xr", "b_xi"))
        br.data.copy_(torch.randn(ops.n, dtype=torch.float64, device="cuda", generator=rng))
        bi.data.copy_(torch.randn(ops.n, dtype=torch.float64, device="cuda", generator=rng))
        lam = complex(1 / 3, np.sqrt(2) / 6) * dt
        K = args.iters

        def timed(fn):
            fn()  # warm-up
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            res = fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e), res

        ms_c, rc = timed(lambda: ops.solve(C_m, lam, br, bi, xr, xi, 0.0, 0.0, K))
        ms_r, rr = timed(lambda: ops.solve(C_m, lam.real, br, None, xr, None, 0.0, 0.0, K))
        time_c = g.Constant(mesh, 0.0)
        theta = beat.MonodomainModel(time=time_c, mesh=mesh, M=M, C_m=C_m, params=dict(theta=0.5))
        tops = theta._ops
        tops.set_guess_order(0)
        theta._state.interpolate(bump)
        x = theta._ops.new_field()

        def pcg():
            x.copy_from(theta._state.field)
            return tops.solve_single(theta._state.field, [], [], x, 0.0, 0.0, K)

        ms_p, rp = timed(pcg)
        per = {"cocg_complex_ms_per_it": ms_c / rc.iterations, "cocg_real_ms_per_it": ms_r / rr.iterations,
               "theta_pcg_ms_per_it": ms_p / max(1, rp.iterations)}
        per["complex_over_theta_pcg"] = per["cocg_complex_ms_per_it"] / per["theta_pcg_ms_per_it"]
        per["complex_over_real_instantiation"] = per["cocg_complex_ms_per_it"] / per["cocg_real_ms_per_it"]
        N = ops.n
        per["cocg_complex_GBps_at_176B"] = 176.0 * N / (per["cocg_complex_ms_per_it"] * 1e6)
        per["iterations"] = [rc.iterations, rr.iterations, rp.iterations]
        out["per_iteration"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in per.items()}
        print("| solve at %d^3 | ms/iteration |" % n)
        print("|---|---|")
        print(f"| COCG, complex shift | {per['cocg_complex_ms_per_it']:.4f} |")
        print(f"| COCG kernels, real instantiation | {per['cocg_real_ms_per_it']:.4f} |")
        print(f"| theta-rule Jacobi-PCG (beat_pde_solve) | {per['theta_pcg_ms_per_it']:.4f} |")
        print(f"complex / theta-rule PCG: {per['complex_over_theta_pcg']:.2f}x; "
              f"complex at 176 B/node: {per['cocg_complex_GBps_at_176B']:.0f} GB/s", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
