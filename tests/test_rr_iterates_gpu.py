"""The register-row PCG (rr_kernel of csrc/beat_pde_rr.hip: RHS, PDOT, RUPD, UDOT, PRUPD) iterate by iterate against a host PCG.

A PCG corrects itself: a pass whose p.Ap or r.D^-1 r is slightly wrong -- a doubled halo lane, a row dropped when ny % RY != 0, a
chunk seam counted twice -- changes alpha and beta, costs an iteration and still converges to the right x, so comparing converged
solutions cannot see it.  Here every solve is cut at max_it = 1, 2, 3, 7 and its ITERATE is compared with the host's
(tests/_pcg_ref.py, in longdouble) of the same k; uncut solves must stop at the host's iteration, not within one of it.  The
yardstick is the distance between the host's own float64 and longdouble runs of the same case: err <= 16 max(delta_k, 2^-52 max|x|);
no tolerance comes from the device.  An error of one part in 1e9 in a single alpha is some 100 times that bound.

BEAT_RR_RY, BEAT_RR_PD and BEAT_RR_BY_ROWS are read once per process: one child (tests/_rr_iterates_script.py) per setting, one
at a time, which asserts through beat_pde_rr_route that it got the instance it asked for.  A child that dies on a signal, aborts
or runs into its time limit fails its test and every later one without another child being started.

The device is given oracle/fem's per-node-type tables and the host their expansion over the box: the same float64 numbers.  (With
the matrices assembled on the whole mesh as the host's operator, the first run on the MI355X missed the bound by up to 1.5 x on the
long boxes, at every k and converged alike: max|x_dev - x| = 2.8e-14 on 125 x 4 x 2 against a bound of 1.9e-14 - 2.7e-14.  The
assembled entries carry the rounding of each cell's own coordinates, u * x / h, differ from node to node, and move A^-1 b itself by
2.75e-14 there -- computed on the host alone, no kernel involved.  test_pcg_ref_cpu.py holds the two sets of matrices together.)

Measured on an MI355X, per process configuration (730 solves each): the largest err / max(delta_k, 2^-52 max|x|) over all iterates
(the bound is 16), the child's own wall time (interpreter and HIP start-up not counted: about 2 s more), and what beat_pde_rr_route
reported for 130 x 6 x 9 in one chunk (x segments, row blocks, planes per chunk, workgroups):

    BEAT_RR_RY  BEAT_RR_PD  BEAT_RR_BY_ROWS   err / yardstick   seconds   route {ry, pd, mask; nsegx, nrb, zc, blocks}
        2           1           -                 1.99            4.8 (first child)   {2, 1, 0;  3, 3, 9, 3}
        2           2           -                 1.99            2.2     {2, 2, 0;  3, 3, 9, 3}
        2           3           -                 1.99            2.1     {2, 3, 0;  3, 3, 9, 3}
        4           1           -                 2.40            2.1     {4, 1, 0;  3, 2, 9, 2}
        4           2           -                 2.40            2.2     {4, 2, 0;  3, 2, 9, 2}
        4           3           -                 2.40            2.6     {4, 3, 0;  3, 2, 9, 2}
        2           1           31                1.99            2.2     {2, 1, 31; 3, 3, 9, 3}
        4           1           31                2.40            2.2     {4, 1, 31; 3, 2, 9, 3}

The worst cases: 65 x 3 x 5 at the stop of rtol 1e-6 (RY = 2), 64 x 4 x 3 at k = 1 (RY = 4).  Norms: at most 0.46 of their bound's
yardstick (1 x 1 x 7, single-reduction loop, k = 1).  Chunk lengths run: 130 x 6 x 9: 1, 2, 3, 5, 9; 129 x 7 x 6: 1, 2, 3, 6;
63 x 5 x 4: 1, 2, 4; 1 x 1 x 7: 1, 2, 3, 4, 7 -- chunks of one plane stay below the limit on block partials at these sizes, so no
operator declined the register-row loop.  The right-hand side with a guess reported 2 rows per wave in every configuration.

Off theta = 1/2 (ref.OPSET_SHAPES under be and skew, keys shape@set; the children of (RY 2, PD 1) and (RY 4, PD 1) without
BEAT_RR_BY_ROWS): at (C_m, theta, dt) = (0.01, 0.5, 0.05), the operator of every case above, A and B have the same factor of K,
and a theta written for 1 - theta, theta dt for dt or a ||b|| formed with the wrong factor passes all of it.  Loops (a) - (d),
both stops and the guess sequences as above, plus a handle re-timed while its guess history is full (run_retime of the child:
cn, skew, cn): the cuts behind set_timestep equal those of a handle created under the set bit for bit, records included, and
their first iterate is the plain reference's.  Measured on an MI355X, same run, same machine (250 solves more per child; the
child's time without them is the earlier commit's child):

    child          set      solves   worst err / yardstick                     worst norm / yardstick    seconds, of the child's
    RY 2, PD 1     be        128     1.49  (65 x 3 x 5, guess order 1, k = 1)   0.35  (64 x 1 x 1, k = 1)
                   skew      106     2.24  (257 x 5 x 1, k = 1)                 0.22  (65 x 3 x 5, k = 1)
                   re-timed   16     1.58  (skew, k = 1)                        0.22                      0.09 of 5.34 (first child)
    RY 4, PD 1     be        128     1.50  (129 x 7 x 6, guess order 1, k = 1)  0.35  (64 x 1 x 1, k = 1)
                   skew      106     1.63  (257 x 5 x 1, k = 1)                 0.21  (129 x 7 x 6, guess order 3, k = 3)
                   re-timed   16     1.12  (skew, k = 1)                        0.11                      0.09 of 2.72

Under cn both children report what they did before: 1.99 / 2.40 and 0.46.  The tests take 9.2 s and 6.3 s with the host's
references (the first took 5.5 and 6.2 s at the earlier commit in two runs of the same session): the device's share of the new cases is 0.1 s, the
rest their longdouble references.  What it found: nothing -- the library is right off theta = 1/2.

The same cases against builds of the library with one arithmetic slip each (a wrong number only; no address, bound, barrier,
exchange or flag changed), and the modules of the commit before these cases (the four iterate modules, tests/test_gpu_kernels.py,
tests/test_var_gpu.py, tests/test_guess_gpu.py; for slip 1 tests/test_distributed_gpu.py as well) against the same builds:
  1 theta for 1 - theta in h_B of upload_tables (csrc/beat_pde.hip) -- the table of B is read by beat_pde_apply(which = 1), by the
      one-launch kernel and by the register-row right-hand side WITH a guess.  Fail: every one-launch pair of
      tests/test_small_iterates_gpu.py (41 x 15 x 7 at be: iterate 1 off by 2.1, at skew by 3.0) and its re-timed handle; the guess
      sequences of the register-row children (65 x 3 x 5 at be, order 1: iterate 1 off by 3.4, rhs_norm by 55 %) and of loops R and M
      on slabs at skew (4.8, 5.1); 24 + 16 cases of tests/test_gpu_kernels.py.  Pass: the plain solves of the register-row kernels,
      loop T, the per-node rows.  The earlier modules: all pass (76 + 163 + 42 + 22 tests and the four iterate modules);
  2 tdt for omt_dt in the rows of B in var_form_A_kernel (csrc/beat_pde_var.hip) -- read by the right-hand side on 8-row tiles
      of a single slab.  Fail: 63 x 16 x 6 full and cutshell at both sets on the default route and under BEAT_VTL_PDOT=0 (full at be:
      iterate 1 off by 2.3, at skew by 3.9, the stop of rtol 1e-9 one iteration early) and their re-timed handles;
      test_per_node_theta_step_matches_direct_solve at both sets.  Pass: BEAT_VTL=0, 62 x 9 x 5 (the gather kernel forms b), and the
      slabs of tests/test_dist_iterates_gpu.py on F, Q and S (a slab with a live face takes the split right-hand side, which does
      not read those rows).  The earlier modules: the iterate modules pass; test_expand_layer_and_surface_stimulus_on_voxel_shell
      of tests/test_var_gpu.py FAILS (its Laplace solve sets (0, 1, 1): u off by 1.0) -- this slip was caught before, by a
      converged solution at theta = 1;
  3 omt_dt taken as theta dt in beat_rr_launch of csrc/beat_pde_rr.hip, where the kernel without a guess uses it for ||b|| only.
      Every iterate and residual_norm of every cut passes; rhs_norm fails in every plain solve on the register-row kernels (65 x 3 x 5
      at be: 1.97e-4 for 1.47e-4), in loops (a) - (d), R and M, on the multi-launch route of tests/test_small_iterates_gpu.py and
      behind the re-timing; 129 x 7 x 6 and 130 x 6 x 9 at be stop one iteration early (12 for 13 at rtol 1e-6), 64 x 32 x 1 at skew
      one late (9 for 8): nothing else moves, and only off theta = 1/2.  Solves with a guess, loop T and the
      one-launch kernel pass.  The earlier modules: all pass.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _pcg_ref as ref
from _pcg_check import Check as _Check

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SCRIPT = ROOT / "tests" / "_rr_iterates_script.py"
CHILD_TIMEOUT = 60  # seconds; measured on an MI355X: 5.2 s per child, start-up included (8 children and their checks: 41.8 s)
ROUTE_KEYS = ("available", "ry", "pd", "by_rows_mask", "nsegx", "nrb", "zc", "nchunks", "total_blocks", "guess_ry")
# (BEAT_RR_RY, BEAT_RR_PD, BEAT_RR_BY_ROWS): (2, 1) is what every grid below 64 M nodes runs, (4, 1) the 512^3 headline
CONFIGS = [(ry, pd, None) for ry in (2, 4) for pd in (1, 2, 3)] + [(2, 1, 31), (4, 1, 31)]
_fatal: list = []  # why no further child may be started


def run_child(out_path, ry, pd, mask, extra_env=None, timeout=CHILD_TIMEOUT):
    """One child under its time limit; every BEAT_* switch but the three of the configuration removed from its environment."""
    if _fatal:
        pytest.fail(f"no child started: an earlier one {_fatal[0]}")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BEAT_")}
    env.update(BEAT_RR_RY=str(ry), BEAT_RR_PD=str(pd))
    if mask is not None:
        env["BEAT_RR_BY_ROWS"] = str(mask)
    env.update(extra_env or {})
    try:
        run = subprocess.run([sys.executable, str(SCRIPT), str(out_path)], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired as exc:
        _fatal.append(f"ran into its time limit of {timeout} s (RY {ry}, PD {pd}, by-rows {mask})")
        err = exc.stderr.decode(errors="replace") if isinstance(exc.stderr, bytes) else (exc.stderr or "")
        pytest.fail(f"child {_fatal[0]}\n{err[-4000:]}")
    if run.returncode < 0 or run.returncode in (134, 139):
        _fatal.append(f"ended with status {run.returncode} (RY {ry}, PD {pd}, by-rows {mask})")
        pytest.fail(f"child {_fatal[0]}\n{run.stderr[-4000:]}")
    assert run.returncode == 0, run.stderr[-4000:]
    return run.stdout


def check_results(npz_path, ry, pd, mask):
    """Every case of one child's results; returns (failures, figures)."""
    data = dict(np.load(npz_path))
    c = _Check(data)
    routes = {k[: -len("|route")]: dict(zip(ROUTE_KEYS, (int(v) for v in data[k]))) for k in data if k.endswith("|route")}
    for key, route in routes.items():
        c.that((route["available"], route["ry"], route["pd"], route["by_rows_mask"], route["guess_ry"]) == (1, ry, pd, mask or 0, 2), key, f"route {route}")
    for shape in ref.SHAPES:
        sk, nz = ref.shape_key(shape), shape[2]
        r = ref.plain_reference(shape)
        settings = sorted({k.split("/")[1] for k in routes if k.startswith(sk + "/") and k.split("/")[2] in "abcd"})
        if shape in ref.CHUNK_SHAPES:
            zcs = {int(s[3:]) for s in settings}
            declined = data[f"{sk}|declined"]
            c.that(all(routes[f"{sk}/zc={zc}/a"]["zc"] == zc for zc in zcs), sk, "a chunk length other than the one asked for")
            c.that(nz in zcs, sk, f"no run in one chunk: {sorted(zcs)}")
            c.that(1 in zcs or len(declined) > 0, sk, f"chunks of one plane neither run nor declined: {sorted(zcs)}")
            c.that(nz < 3 or bool(zcs & {2, 3}), sk, f"no run with chunks of 2 or 3 planes: {sorted(zcs)}")
            c.that(nz not in (7, 9) or any(zc > 1 and nz % zc for zc in zcs), sk, f"no run with nz % zc != 0: {sorted(zcs)}")
        else:
            c.that(settings == ["default"], sk, f"settings {settings}")
        for setting in settings:
            for loop in "abcd":
                base = f"{sk}/{setting}/{loop}"
                c.that(base in routes, base, "no route report")
                for k in ref.CUTS:
                    c.cut(f"{base}/k={k}", r, k)
                if loop != "b" or shape in ref.CHUNK_SHAPES:
                    for rtol in ref.RTOLS:
                        c.uncut(f"{base}/rtol={rtol:g}", r, rtol)
            tails = [f"k={k}" for k in ref.CUTS]
            for tail in tails + ([f"rtol={rtol:g}" for rtol in ref.RTOLS] if shape in ref.CHUNK_SHAPES else []):
                c.same_bits(f"{sk}/{setting}/a/{tail}", f"{sk}/{setting}/b/{tail}", True)  # the predicted stop feeds no iterate
            for tail in tails + [f"rtol={rtol:g}" for rtol in ref.RTOLS]:
                c.same_bits(f"{sk}/{setting}/a/{tail}", f"{sk}/{setting}/c/{tail}", False)  # the two-part launches: same kernels, same order
        if shape in ref.GUESS_SHAPES:
            p = ref.problem(shape)
            v = ref.field(shape, ref.GUESS_SOLVES + 1)
            bL = ref.rhs_longdouble(p, v)
            for order in ref.GUESS_ORDERS:
                for k in ref.GUESS_CUTS:
                    key = f"{sk}/default/e/order={order}/k={k}"
                    # the device's own earlier, converged solves of the sequence supply the increments; they are not what is compared
                    incs = [data[f"{key}/solve={j}|x"] - ref.field(shape, j) for j in range(ref.GUESS_SOLVES, 0, -1)]
                    c.that(all(c.rec(f"{key}/solve={j}")[1] > 0 for j in range(1, ref.GUESS_SOLVES + 1)), key, "a solve in front of the cut did not converge")
                    x0 = v.astype(np.longdouble) + ref.guess_increment(order, incs)
                    c.cut(key, ref.reference(p, bL, x0, k), k)
    cn_worst, cn_worst_norm = c.worst, c.worst_norm
    off_cn = {}
    c.that(bool(data["opsets"]) == (pd == 1 and mask is None), "opsets", f"the cases off theta = 1/2 {'ran' if data['opsets'] else 'did not run'}")
    if pd == 1 and mask is None and bool(data["opsets"]):
        off_cn = check_opsets(c, data, routes)
        off_cn["seconds"] = float(data["opsets_seconds"])
    c.worst, c.worst_norm = cn_worst, cn_worst_norm
    figures = {"worst err/max(delta_k, floor)": c.worst, "worst norm err/bound*16": c.worst_norm, "child seconds": float(data["seconds"]),
               "off theta = 1/2": off_cn,
               "solves": sum(k.endswith("|x") for k in data), "route 130x6x9 one chunk": routes.get("130x6x9/zc=9/a"),
               "route 3x70x2": routes.get("3x70x2/default/a"),
               "chunk lengths": {ref.shape_key(s): sorted({routes[k]["zc"] for k in routes if k.startswith(ref.shape_key(s) + "/zc=")}) for s in ref.CHUNK_SHAPES}}
    return c.failures, figures


def check_opsets(c, data, routes):
    """The pairs of ref.OPSET_SHAPES (keys shape@set) with the checks of the cn cases, and the re-timed handle; per set (solves, worst
    err / yardstick, worst norm / yardstick)."""
    figures = {}
    for name in ref.NEW_SETS:
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        for shape, sets in ref.OPSET_SHAPES.items():
            if name not in sets:
                continue
            ck = ref.case_key(shape, name)
            r = ref.plain_reference(shape, name)
            for loop in "abcd":
                base = f"{ck}/default/{loop}"
                c.that(base in routes, base, "no route report")
                for k in ref.CUTS:
                    c.cut(f"{base}/k={k}", r, k)
                if loop != "b":
                    for rtol in ref.RTOLS:
                        c.uncut(f"{base}/rtol={rtol:g}", r, rtol)
            for tail in [f"k={k}" for k in ref.CUTS]:
                c.same_bits(f"{ck}/default/a/{tail}", f"{ck}/default/b/{tail}", True)
            for tail in [f"k={k}" for k in ref.CUTS] + [f"rtol={rtol:g}" for rtol in ref.RTOLS]:
                c.same_bits(f"{ck}/default/a/{tail}", f"{ck}/default/c/{tail}", False)
            if shape in ref.OPSET_GUESS_SHAPES:
                p = ref.problem(shape, name)
                v = ref.field(shape, ref.GUESS_SOLVES + 1)
                bL = ref.rhs_longdouble(p, v)
                for order in ref.GUESS_ORDERS:
                    for k in ref.GUESS_CUTS:
                        key = f"{ck}/default/e/order={order}/k={k}"
                        incs = [data[f"{key}/solve={j}|x"] - ref.field(shape, j) for j in range(ref.GUESS_SOLVES, 0, -1)]
                        c.that(all(c.rec(f"{key}/solve={j}")[1] > 0 for j in range(1, ref.GUESS_SOLVES + 1)), key, "a solve in front of the cut did not converge")
                        c.cut(key, ref.reference(p, bL, v.astype(np.longdouble) + ref.guess_increment(order, incs), k), k)
        figures[name] = (sum(k.endswith("|x") and f"@{name}/" in k for k in data), c.worst, c.worst_norm)
    # the re-timed handle: first cut of every stage from x0 = v_ (the history was dropped), the stages equal fresh handles bit for bit
    c.worst, c.worst_norm = (0.0, None), (0.0, None)
    shape = next(iter(ref.OPSET_SHAPES))
    base = f"{ref.shape_key(shape)}/retime"
    for stage, name in enumerate(ref.RETIME):
        c.that(f"{base}/live{stage}" in routes, f"{base}/live{stage}", "no route report")
        c.cut(f"{base}/live{stage}/k={ref.CUTS[0]}", ref.plain_reference(shape, name), ref.CUTS[0])
    c.cut(f"{base}/fresh/k={ref.CUTS[0]}", ref.plain_reference(shape, ref.RETIME[1]), ref.CUTS[0])
    for k in ref.CUTS:
        c.same_bits(f"{base}/fresh/k={k}", f"{base}/live1/k={k}", True)   # re-timed to skew: a handle created under skew
        c.same_bits(f"{base}/live0/k={k}", f"{base}/live2/k={k}", True)   # and back: what the handle gave before
        for stage in (1, 2):
            other = "fresh" if stage == 1 else "live0"
            c.that(data[f"{base}/live{stage}/k={k}|rec"].tobytes() == data[f"{base}/{other}/k={k}|rec"].tobytes(), f"{base}/live{stage}/k={k}",
                   f"record {data[f'{base}/live{stage}/k={k}|rec'].tolist()}, {other} {data[f'{base}/{other}/k={k}|rec'].tolist()}")
        c.that(not np.array_equal(data[f"{base}/live0/k={k}|x"], data[f"{base}/live1/k={k}|x"]), f"{base}/live1/k={k}", "the re-timing changed nothing")
    figures["retime"] = (sum(k.endswith("|x") and "/retime/" in k for k in data), c.worst, c.worst_norm)
    return figures


@pytest.mark.parametrize("ry,pd,mask", CONFIGS, ids=[f"ry{ry}-pd{pd}" + (f"-rows{mask}" if mask else "") for ry, pd, mask in CONFIGS])
def test_rr_iterates_match_host_pcg(tmp_path, ry, pd, mask):
    out = tmp_path / "out.npz"
    print(run_child(out, ry, pd, mask).strip())
    failures, figures = check_results(out, ry, pd, mask)
    print(f"RY {ry} PD {pd} by-rows {mask}: {figures}")
    assert not failures, f"{len(failures)} failures (RY {ry}, PD {pd}, by-rows {mask}), the first:\n" + "\n".join(failures[:40])
