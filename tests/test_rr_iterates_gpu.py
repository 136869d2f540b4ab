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
    figures = {"worst err/max(delta_k, floor)": c.worst, "worst norm err/bound*16": c.worst_norm, "child seconds": float(data["seconds"]),
               "solves": sum(k.endswith("|x") for k in data), "route 130x6x9 one chunk": routes.get("130x6x9/zc=9/a"),
               "route 3x70x2": routes.get("3x70x2/default/a"),
               "chunk lengths": {ref.shape_key(s): sorted({routes[k]["zc"] for k in routes if k.startswith(ref.shape_key(s) + "/zc=")}) for s in ref.CHUNK_SHAPES}}
    return c.failures, figures


@pytest.mark.parametrize("ry,pd,mask", CONFIGS, ids=[f"ry{ry}-pd{pd}" + (f"-rows{mask}" if mask else "") for ry, pd, mask in CONFIGS])
def test_rr_iterates_match_host_pcg(tmp_path, ry, pd, mask):
    out = tmp_path / "out.npz"
    print(run_child(out, ry, pd, mask).strip())
    failures, figures = check_results(out, ry, pd, mask)
    print(f"RY {ry} PD {pd} by-rows {mask}: {figures}")
    assert not failures, f"{len(failures)} failures (RY {ry}, PD {pd}, by-rows {mask}), the first:\n" + "\n".join(failures[:40])
