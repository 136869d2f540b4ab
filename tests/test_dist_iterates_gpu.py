"""The slab-decomposed diffusion solve (beat_pde_solve_dist, csrc/beat_dist.hip: the split right-hand sides and the four loops of
beat_dist_enqueue_iterations) on 2 to 8 ranks with LIVE ghost planes, iterate by iterate against the host PCG.

tests/test_rr_iterates_gpu.py, tests/test_small_iterates_gpu.py and tests/test_var_iterates_gpu.py say why converged solutions cannot
be compared: a PCG corrects itself.  All three stop where a slab gets a neighbour, and tests/test_distributed_gpu.py, which does run
slabs with neighbours, compares converged solutions near -85 to 1e-9 and iteration counts "within one".  Here the ranks are threads
over the callback transport (tests/_thread_world.py; its all-reduce adds in rank order, the same bits on every rank), every thread
world in a child process (tests/_dist_iterates_script.py) under its own time limit, and the ASSEMBLED iterate of every solve cut at
max_it = 1, 2, 3, 7 is held to the references of tests/_pcg_ref.py and tests/_var_ref.py with the checks of tests/_pcg_check.py:
err <= 16 max(delta_k, 2^-52 max|x|), delta_k the distance between the host's own float64 and longdouble runs; uncut solves stop at
the host's iteration.  No reference and no tolerance is new; tests/test_dist_cases_cpu.py shows on the host that summing the dot
products slab by slab stays far inside that bound (at most 2.2 of the 16).

children   rr2 (BEAT_RR_RY=2, BEAT_RR_PD=1): constant coefficients, loops R (register-row, two reductions), M (single reduction,
           ops.set_single_reduction) and T (BEAT_RR=0: halo_start(p), beat_pde_spmv_dot_part 0 / 1, cg_update_r, cg_next_oop);
           rr4 (BEAT_RR_RY=4): R and M on the shapes with ny >= 4; varF, varQ, varS: per-node rows, one route each (a child of its
           own keeps each below 10 s) -- F (default: the fused beat_vtl_pdot_part where ALL ranks can run it), Q
           (BEAT_VTL_PDOT=0: beat_pde_spmv_dot_part on the tiles), S (BEAT_VTL=0: the segment lists).
cases      DIST_CASES of the two reference modules; every rank of a per-node case gets its columns of the rows the host expands.
routes     asserted BEFORE any value, against expected_const / expected_var below, which are the rules of the source written out:
           beat_rr_available (no BEAT_RR=0, constant coefficients), beat_vtl_setup and vtl_sizes_declined (a slab of ONE plane, or an
           axis of one node, has no tiles), beat_vtl_available (a slab without a tissue node has no tile list), beat_pde_create_var (a
           slab with a live face keeps a ring of 6: beat_pde_tile_route is 1 or 0), beat_vtl_pdot_dist_available (tiles of 8 rows:
           ny >= 16) and the agreement over the ranks in beat_dist_solve_begin (fused on all ranks or on none).
           So the fused pass cannot run in a world with a one-plane slab: route F then checks the loop it falls to (the classic one,
           on the segment lists of the ranks without tiles), and the expectation says so; every loop and route is run on a middle slab
           and on a one-plane slab, and the fused pass itself on middle slabs of 2, 5 and 7 planes.
per solve  Check.cut / Check.uncut on the assembled x and rank 0's record; every rank's record equal to rank 0's bit for bit; the
           cuts at 3 and 7 again with defer_flush and flush_pending: the same bits; per-node rows: every node off the tissue holds
           exactly its v (1000 + node index), v unchanged on every rank; guess sequences (four converged solves of a moving field,
           then a cut, orders 1 and 3) on DIST_GUESS_CASES, the reference from the host's own extrapolation of the device's increments.
ghost p    R, M and F never exchange the search direction: part 1 of their passes forms it on the ghost planes from the exchanged
           r, the direction kept there and (F) the neighbours' centre coefficients.  Behind the cuts at 2 and 7 every rank's ring
           field of the last direction is read with its ghost planes and each live ghost plane compared with the neighbour's owned
           boundary plane: see check_ghost_planes for what is asserted and why.

What it found, on an MI355X: nothing.  Every case passed on every loop and route as the kernels were, the ghost planes of the
directions bit for bit, one-plane slabs, slabs without a tissue node and seven one-node slabs included.

Measured on an MI355X (the bound on err / max(delta_k, 2^-52 max|x|) is 16; the norms' ratio is to the yardstick of their bound),
per child its own wall time (interpreter and HIP start-up not counted: about 2 s more) and per loop the worst over its cases:

    child  seconds  solves   loop   worst err / yardstick                              worst norm / yardstick
    rr2      6.1      512     R     2.16  (65 x 3 x 5 / 3, guess of order 3, k = 3)    0.37  (65 x 3 x 5 / 3, guess of order 1, k = 1)
                              M     1.99  (65 x 3 x 5 / 2, the stop of rtol 1e-6)      0.36  (2 x 2 x 2 / 2, k = 2)
                              T     2.40  (64 x 4 x 3 / 2, k = 1)                      0.30  (2 x 2 x 2 / 2, k = 2)
    rr4      3.5      216     R, M  2.40  (64 x 4 x 3 / 2, k = 1)                      0.29  (63 x 5 x 4 / 4, k = 1)
    varF     6.7      248     F     3.00  (6 x 4 x 71 layers / 8, k = 1)               0.30  (125 x 18 x 20 cutshell / 3, guess of order 3, k = 1)
    varQ     5.8      208     Q     3.00  (6 x 4 x 71 layers / 8, k = 1)               0.27  (2 x 2 x 2 full / 2, the stop of rtol 1e-9)
    varS     6.4      248     S     3.00  (6 x 4 x 71 layers / 8, k = 1)               0.27  (2 x 2 x 2 full / 2, the stop of rtol 1e-9)

The module: 37.7 s, its tests 7.6, 4.3, 9.1, 6.9 and 7.6 s with the host's checks.  Nothing was trimmed: 125 x 18 x 20 on 4 ranks and
130 x 6 x 9 on 4 ranks run.  One child for all three per-node routes took 11.7 s (14.5 s with its checks): a child per route keeps every
test below 10 s, at the price of building the twelve cases' rows three times (some 3 s of each child's time; its 26 thread worlds
take about 0.12 s each).

The same module against builds with one deliberate arithmetic slip each (wrong numbers; no address, bound, barrier, exchange or
flag changed), and, once per build, the thread tests of tests/test_distributed_gpu.py (-k in_threads: 36 tests):
  1 the first owned plane of a slab with a live lower neighbour counted twice in the partial of p.Ap (rr_kernel, MODE RR_PDOT) -- all
      18 cases of rr2 and all 11 of rr4 fail on loop R from iterate 1 on (64 x 4 x 3 / 2: off by 0.76); M (RR_UDOT), T and the
      per-node children pass.  The thread tests: 18 of 36 fail, the iteration counts off by 10 to 188 -- an error of this size is no
      self-correcting one;
  2 beta dropped where MODE 3 of vtl_spmv_kernel forms p on the upper ghost plane -- the 12 worlds in which a row couples across an
      upper face and the fused pass runs (125 x 18 x 20 full, cutshell, specks / 2, 3, 4; 63 x 16 x 6 full / 2, 3, specks / 3) fail on
      route F from iterate 2 on (125 x 18 x 20 full / 2: 2.7e-4 at k = 2, 1.9e-2 at k = 3) and in the ghost-plane comparison; the
      layers masks and 63 x 16 x 6 specks / 2, where no tissue meets across a face, Q, S and the constant-coefficient children
      pass.  The thread tests: 5 of 36 fail (per-node rows, library loop), x off by 0.39;
  3 the ghost plane of e taken as zero in the right-hand side with a guess (rr_kernel, MODE RR_RHS) -- the guess sequences fail, on R
      and M, from iterate 1 of the cut behind the sequence (65 x 3 x 5 / 3, order 1: off by 0.96); everything without a guess
      passes.  The thread tests: 6 of 36 fail (the split steps with a guess, iteration counts off by up to 187);
  4 slip 1 on ONE lane of one row per wave (lane 5, the first row) instead of the whole plane -- every case at least 6 nodes wide fails
      on loop R from iterate 1 on (64 x 4 x 3 / 2: off by 5.1e-3 at k = 1, 2.4e-5 at k = 7), 2 x 2 x 2, 3 x 70 x 2 and 1 x 1 x 7, which
      have no such node, pass.  The thread tests: test_slabs_in_threads_match_single_slab_solve (16) and
      test_single_reduction_iteration_on_slabs_in_threads (8) PASS -- same converged x, iteration counts within one; 5 of the 12
      split-step cases fail, by 8e-8 to 3e-6 against their 1e-9 after 25 steps;
  5 slip 2 on ONE lane (lane 7) of the upper ghost plane -- the same 12 worlds fail on route F from iterate 2 on (125 x 18 x 20 full
      / 2: 8.3e-7 at k = 2, 6.5e-3 at k = 3).  The thread tests: 5 of 36 fail (x off by 0.11): a direction that differs between the
      two ranks that hold it breaks the recurrence for good.
So slips 1 to 3 are too coarse to pass the thread tests either; what those let through is an error of the size of slip 4 in a
dot product, which costs an iteration at most and leaves the converged x alone.

Off theta = 1/2 (ref.DIST_OPSET_CASES on loops R, M, T in child rr2, vr.DIST_OPSET_CASES on F, Q, S, the guess sequences of
DIST_OPSET_GUESS at skew, keys case@set; tests/test_rr_iterates_gpu.py says why, and holds the record of the builds with a deliberate
slip), and handles re-timed on every rank while their guess history is full (retime_solves of the child: cn, skew, cn; loop R, and
each per-node route -- on F beat_pde_set_timestep invalidates the neighbours' centre coefficients, which the next solve exchanges
again).  The 45 000-node guess case of vr.DIST_GUESS_CASES is not run off cn: a few thousand nodes tell the factors apart.
Measured on an MI355X, same run (the child's time without the new cases is the earlier commit's child):

    child   solves more   seconds, of the child's   worst err / yardstick: be, skew, re-timed             worst norm / yardstick
    rr2        192          1.78 of 7.55            R 1.28, 1.71, 1.58;  M 1.28, 1.58;  T 1.15, 1.57         0.21, 0.18, 0.16
    varF        52          0.64 of 7.12            0.95, 1.77, 1.79                                        0.08, 0.14, 0.14
    varQ        32          0.45 of 5.93            0.95, 1.77, 1.79                                        0.08, 0.14, 0.14
    varS        52          0.52 of 6.77            0.95, 1.77, 1.79                                        0.08, 0.14, 0.14

rr4 is unchanged (3.4 s).  Under cn every loop reports what it did before.  The module: 40.4 s (36.6 s for the earlier commit's, same
session).  What it found: nothing.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _pcg_ref as ref
import _var_ref as vr
from _pcg_check import Check

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SCRIPT = ROOT / "tests" / "_dist_iterates_script.py"
CHILDREN = {"rr2": {"BEAT_RR_RY": "2", "BEAT_RR_PD": "1"}, "rr4": {"BEAT_RR_RY": "4", "BEAT_RR_PD": "1"}, "varF": {}, "varQ": {}, "varS": {}}
CHILD_TIMEOUT = {"rr2": 90, "rr4": 60, "varF": 90, "varQ": 80, "varS": 90}  # seconds: about ten times the measured wall time, start-up included
CONST_LOOPS = {"rr2": ("R", "M", "T"), "rr4": ("R", "M")}
VAR_ROUTES = ("F", "Q", "S")
DEFER_CUTS, GHOST_CUTS = (3, 7), (2, 7)
ROUTE_KEYS = ("available", "ry", "pd", "by_rows_mask", "nsegx", "nrb", "zc", "nchunks", "total_blocks", "guess_ry")
_fatal: list = []  # why no further child may be started


def run_child(out_path, child):
    """One child under its time limit; every BEAT_* switch but those of the child removed from its environment."""
    if _fatal:
        pytest.fail(f"no child started: an earlier one {_fatal[0]}")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BEAT_")}
    env.update(CHILDREN[child])
    timeout = CHILD_TIMEOUT[child]
    try:
        run = subprocess.run([sys.executable, str(SCRIPT), str(out_path), child], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired as exc:
        _fatal.append(f"ran into its time limit of {timeout} s ({child})")
        err = exc.stderr.decode(errors="replace") if isinstance(exc.stderr, bytes) else (exc.stderr or "")
        pytest.fail(f"child {_fatal[0]}\n{err[-4000:]}")
    if run.returncode < 0 or run.returncode in (3, 134, 139):  # (3: a rank did not come back, the child gave up on it)
        _fatal.append(f"ended with status {run.returncode} ({child})")
        pytest.fail(f"child {_fatal[0]}\n{run.stderr[-4000:]}")
    assert run.returncode == 0, run.stderr[-4000:]
    return run.stdout


def const_cases(child):
    return [(s, w) for s, worlds in ref.DIST_CASES.items() for w in worlds if child == "rr2" or s[1] >= ref.DIST_RY4_MIN_NY]


def var_cases():
    return [(c, w) for c, worlds in vr.DIST_CASES for w in worlds]


def expected_const(loop, ry):
    """What beat_pde_rr_route reports on every rank (available, ry, pd, by_rows_mask, guess_ry) and whether the communicator counts
    the solve as a single-reduction one: beat_rr_available declines under BEAT_RR=0 and nowhere else at these sizes (a few blocks
    against BEAT_MAX_PARTIALS), whatever the slab's planes; `merged` of beat_dist_solve_begin needs it."""
    return (0 if loop == "T" else 1, ry, 1, 0, 2), loop == "M"


def expected_var(cs, world, route):
    """Per rank (beat_pde_tile_route, beat_pde_fused_dist_pass)."""
    nx, ny, nz = cs.shape
    plane = nx * ny
    z = np.concatenate([[0], np.cumsum(ref.slab_counts(nz, world))])
    tiles = [int(route != "S" and min(nx, ny, z[r + 1] - z[r]) >= 2 and bool(cs.tissue[z[r] * plane : z[r + 1] * plane].any())) for r in range(world)]
    fused = int(route == "F" and ny >= 16 and all(tiles))
    return [(t, fused) for t in tiles]


def test_every_loop_meets_a_middle_slab_and_a_one_plane_slab():
    """From the tables and the expectations alone (no device): each of R, M, T, F, Q, S is run in a world with a middle slab (both
    ghost planes live) and in one with a one-plane slab -- F, whose fused pass no world with a one-plane slab can agree on, as the
    loop it falls to there, and fused on middle slabs."""
    one = lambda nz, w: 1 in ref.slab_counts(nz, w)  # noqa: E731
    for child, loops in CONST_LOOPS.items():
        cases = const_cases(child)
        assert any(w >= 3 for _, w in cases) and any(one(s[2], w) for s, w in cases), child
        assert any(w >= 3 and ref.slab_counts(s[2], w)[1] == 1 for s, w in cases), child  # a one-plane MIDDLE slab
        assert any(w >= 3 and ref.slab_counts(s[2], w)[1] > 1 for s, w in cases), child
    cases = var_cases()
    assert any(w >= 3 for _, w in cases) and any(one(c[0][2], w) for c, w in cases)  # (every case runs every route)
    fused = [(c, w) for c, w in cases if expected_var(vr.case(c), w, "F")[0][1]]
    assert {ref.slab_counts(c[0][2], w)[1] for c, w in fused if w >= 3} == {2, 5, 7}
    assert not any(one(c[0][2], w) for c, w in fused)
    assert {c[0] for c, _ in fused} == {(125, 18, 20), (63, 16, 6)} and (((63, 16, 6), "layers"), 6) not in fused
    # a world in which no rank has tiles (one-plane slabs), one in which all have tiles of four rows
    assert [t for t, _ in expected_var(vr.case(((63, 16, 6), "layers")), 6, "F")] == [0] * 6
    assert [t for t, _ in expected_var(vr.case(((62, 9, 5), "full")), 2, "F")] == [1, 1]
    assert all(cw in const_cases("rr2") for cw in ref.DIST_GUESS_CASES) and any(cw in const_cases("rr4") for cw in ref.DIST_GUESS_CASES)
    assert all(expected_var(vr.case(c), w, "F")[0][1] for c, w in vr.DIST_GUESS_CASES)


def same_records(c, data, key):
    recs = data[f"{key}|recs"]
    c.that(all(recs[r].tobytes() == recs[0].tobytes() for r in range(len(recs))), key, f"the ranks' records differ: {recs.tolist()}")


def ulps(a, b):
    """max |a - b| in units of the last place of the largest value of b."""
    scale = np.abs(b).max(initial=0.0)
    return 0.0 if np.array_equal(a, b) else float(np.abs(a - b).max() / np.spacing(scale if scale > 0 else 1.0))


def check_ghost_planes(c, data, base, shape, world, coupled=None):
    """The ghost planes each rank keeps of the last direction against the neighbour's owned boundary plane, behind the cuts at 2 and 7.

    Both sides evaluate p = D^-1 r + beta p_old on the same bits: r on the ghost plane is the neighbour's r (exchanged), beta is
    all-reduced, and p_old on the ghost plane was formed the same way one iteration earlier (first iteration: p = D^-1 r).  The
    register-row kernels (rr_kernel of csrc/beat_pde_rr.hip) take D^-1 from the same per-node-type table with the ghost plane's z
    type (beat_pde_set_ghost_types) and form the direction for a ghost plane with the code that forms it for an owned one;
    vtl_spmv_kernel's MODE 3 takes D^-1 of a ghost node as the reciprocal of the exchanged centre coefficient, the expression
    var_form_A_kernel stores in v_dinv.  So bit equality is asserted: on every node of the plane with constant coefficients; with
    per-node rows on the nodes of the ghost plane that a row of this slab couples to (`coupled`: per direction, the tissue nodes with
    a coefficient that is not zero towards the slab's boundary plane, from the rows the device was given) -- the tile pass forms the
    direction where its product reads it and nowhere else, so a ghost node no row reads holds whatever the ring field held (seen on
    63 x 16 x 6 layers on 2 ranks: rank 0's planes 0 - 2 end in a plane without tissue, and its ghost plane 3 is never written).
    Where p is exchanged (T, Q, S and F without the fused pass) the ghost plane is a copy, and equal a fortiori.  Returns the
    number of nodes compared."""
    nx, ny, nz = shape
    plane = nx * ny
    counts = ref.slab_counts(nz, world)
    z = np.concatenate([[0], np.cumsum(counts)])
    compared = 0
    for k in GHOST_CUTS:
        if f"{base}/k={k}|p0" not in data:
            continue
        p = [data[f"{base}/k={k}|p{r}"] for r in range(world)]
        c.that(all(len(p[r]) == (counts[r] + 2) * plane for r in range(world)), base, "a direction of the wrong length")
        for r in range(world - 1):
            sel = slice(None) if coupled is None else coupled[-1][z[r + 1] * plane : (z[r + 1] + 1) * plane]
            compared += plane if coupled is None else int(sel.sum())
            up_ghost, up_owned = p[r][(counts[r] + 1) * plane :][sel], p[r + 1][plane : 2 * plane][sel]
            c.that(np.array_equal(up_ghost, up_owned), f"{base}/k={k}", f"upper ghost plane of rank {r} differs from rank {r + 1}'s first plane in "
                   f"{int((up_ghost != up_owned).sum())} of {up_owned.size} nodes, by {ulps(up_ghost, up_owned):.1f} ulp")
            sel = slice(None) if coupled is None else coupled[+1][(z[r + 1] - 1) * plane : z[r + 1] * plane]
            compared += plane if coupled is None else int(sel.sum())
            lo_ghost, lo_owned = p[r + 1][:plane][sel], p[r][counts[r] * plane : (counts[r] + 1) * plane][sel]
            c.that(np.array_equal(lo_ghost, lo_owned), f"{base}/k={k}", f"lower ghost plane of rank {r + 1} differs from rank {r}'s last plane in "
                   f"{int((lo_ghost != lo_owned).sum())} of {lo_owned.size} nodes, by {ulps(lo_ghost, lo_owned):.1f} ulp")
    return compared


def coupled_nodes(cs):
    """{-1: the tissue nodes with a coefficient that is not zero towards the plane below them, +1: towards the plane above}."""
    from oracle import fem

    out = {}
    for d in (-1, 1):
        ks = [k for k, (_, _, oz) in enumerate(fem.STENCIL_OFFSETS) if oz == d]
        out[d] = cs.tissue & ((cs.mass_rows[ks] != 0.0) | (cs.stiff_rows[ks] != 0.0)).any(axis=0)
    return out


def check_solves(c, data, base, r, cuts):
    """The plain solves of one case and loop: cut, uncut, records alike on all ranks, deferred flush."""
    for k in cuts:
        c.cut(f"{base}/k={k}", r, k)
        same_records(c, data, f"{base}/k={k}")
    for rtol in ref.RTOLS:
        c.uncut(f"{base}/rtol={rtol:g}", r, rtol)
        same_records(c, data, f"{base}/rtol={rtol:g}")
    for k in DEFER_CUTS:
        if k in cuts:
            c.same_bits(f"{base}/k={k}", f"{base}/defer/k={k}", True)
            same_records(c, data, f"{base}/defer/k={k}")


def check_guess(c, data, base, p, field):
    """As check_guess of tests/test_var_iterates_gpu.py: the device's own earlier, converged solves supply the increments."""
    v = field(ref.GUESS_SOLVES + 1)
    bL = ref.rhs_longdouble(p, v)
    for order in ref.GUESS_ORDERS:
        for k in ref.GUESS_CUTS:
            key = f"{base}/e/order={order}/k={k}"
            c.that(all(c.rec(f"{key}/solve={j}")[1] > 0 for j in range(1, ref.GUESS_SOLVES + 1)), key, "a solve in front of the cut did not converge")
            incs = [data[f"{key}/solve={j}|x"] - field(j) for j in range(ref.GUESS_SOLVES, 0, -1)]
            if not all(np.isfinite(i).all() for i in incs):
                c.that(False, key, "a solve in front of the cut left x not finite")
                continue
            x0 = v.astype(np.longdouble) + ref.guess_increment(order, incs)
            c.cut(key, ref.reference(p, bL, x0, k), k)
            same_records(c, data, key)


def check_const(data, child):
    """(route failures, value failures, figures per loop) of a constant-coefficient child."""
    ry = int(CHILDREN[child]["BEAT_RR_RY"])
    routes, figures = [], {}
    cases = const_cases(child)
    off_cn = [(shape, world, name) for (shape, world), sets in ref.DIST_OPSET_CASES.items() for name in sets] if child == "rr2" else []
    for shape, world, name in [(s, w, "cn") for s, w in cases] + off_cn:
        for loop in CONST_LOOPS[child]:
            base = f"{ref.case_key(shape, name)}/w{world}/{loop}"
            want, merged = expected_const(loop, ry)
            for rank in range(world):
                got = dict(zip(ROUTE_KEYS, (int(v) for v in data[f"{base}|rr_route"][rank])))
                if tuple(got[k] for k in ("available", "ry", "pd", "by_rows_mask", "guess_ry")) != want:
                    routes.append(f"{base} rank {rank}: beat_pde_rr_route {got}, expected (available, ry, pd, mask, guess_ry) = {want}")
                if tuple(data[f"{base}|tile"][rank]) != (0, 0):
                    routes.append(f"{base} rank {rank}: tile route {data[f'{base}|tile'][rank]} on constant coefficients")
                if int(data[f"{base}|merged"][rank][0]) != (int(data[f"{base}|nsolves"][rank]) if merged else 0):
                    routes.append(f"{base} rank {rank}: {int(data[f'{base}|merged'][rank][0])} single-reduction solves of {int(data[f'{base}|nsolves'][rank])}")
    if off_cn:
        shape, world = next(iter(ref.DIST_OPSET_CASES))
        for tag in ("live0", "live1", "live2", "fresh"):
            key = f"{ref.shape_key(shape)}/w{world}/R/retime/{tag}"
            for rank in range(world):
                got = dict(zip(ROUTE_KEYS, (int(v) for v in data[f"{key}|rr"][rank])))
                if tuple(got[k] for k in ("available", "ry", "pd", "by_rows_mask", "guess_ry")) != expected_const("R", ry)[0] or tuple(data[f"{key}|tile"][rank]) != (0, 0):
                    routes.append(f"{key} rank {rank}: beat_pde_rr_route {got}, tile route {data[f'{key}|tile'][rank]}")
    if routes:
        return routes, [], figures
    c = Check(data)
    c.failures.extend(str(s) for s in data["slips"])
    for loop in CONST_LOOPS[child]:
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        for shape, world in cases:
            base = f"{ref.shape_key(shape)}/w{world}/{loop}"
            check_solves(c, data, base, ref.plain_reference(shape), ref.CUTS)
            check_ghost_planes(c, data, base, shape, world)
            if loop in "RM" and (shape, world) in ref.DIST_GUESS_CASES:
                check_guess(c, data, base, ref.problem(shape), lambda j, s=shape: ref.field(s, j))
        figures[loop] = (c.worst, c.worst_norm)
    for name in ref.NEW_SETS if off_cn else ():
        for loop in CONST_LOOPS[child]:
            c.worst, c.worst_norm = (0.0, None), (0.0, None)
            for shape, world, _ in [t for t in off_cn if t[2] == name]:
                base = f"{ref.case_key(shape, name)}/w{world}/{loop}"
                check_solves(c, data, base, ref.plain_reference(shape, name), ref.CUTS)
                check_ghost_planes(c, data, base, shape, world)
                if loop in "RM" and name in ref.DIST_OPSET_GUESS.get((shape, world), ()):
                    check_guess(c, data, base, ref.problem(shape, name), lambda j, s=shape: ref.field(s, j))
            figures[f"{name}/{loop}"] = (c.worst, c.worst_norm)
    if off_cn:
        shape, world = next(iter(ref.DIST_OPSET_CASES))
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        check_retime(c, data, f"{ref.shape_key(shape)}/w{world}/R", lambda name, s=shape: ref.plain_reference(s, name), ref.CUTS)
        figures["retime"] = (c.worst, c.worst_norm)
        figures["off theta = 1/2: seconds, solves"] = (float(data["opsets_seconds"]), sum(k.endswith("|x") and ("@" in k or "/retime/" in k) for k in data))
    return [], c.failures, figures


def check_retime(c, data, base, reference_of, cuts):
    """The re-timed handles of one world (retime_solves of the child): the first cut of every stage from x0 = v_ -- the plain
    reference's iterate: the history was dropped --, re-timed to skew a handle created under skew bit for bit, and back under cn what
    the handles gave before; every rank's record alike."""
    for stage, name in enumerate(ref.RETIME):
        c.cut(f"{base}/retime/live{stage}/k={cuts[0]}", reference_of(name), cuts[0])
    c.cut(f"{base}/retime/fresh/k={cuts[0]}", reference_of(ref.RETIME[1]), cuts[0])
    for k in cuts:
        for mine, other in ((f"{base}/retime/live1/k={k}", f"{base}/retime/fresh/k={k}"), (f"{base}/retime/live2/k={k}", f"{base}/retime/live0/k={k}")):
            c.same_bits(other, mine, True)
            c.that(data[f"{mine}|recs"].tobytes() == data[f"{other}|recs"].tobytes(), mine, f"records {data[f'{mine}|recs'].tolist()}, {other} {data[f'{other}|recs'].tolist()}")
            same_records(c, data, mine)
        c.that(not np.array_equal(data[f"{base}/retime/live0/k={k}|x"], data[f"{base}/retime/live1/k={k}|x"]), f"{base}/retime/live1/k={k}", "the re-timing changed nothing")


def check_var(data, var_routes=VAR_ROUTES):
    """(route failures, value failures, figures per route) of the per-node children of the routes given."""
    routes, figures = [], {}
    cases = var_cases()
    off_cn = [(case, world, name) for (case, world), sets in vr.DIST_OPSET_CASES.items() for name in sets]
    off_cn_guess = [(case, world, name) for (case, world), sets in vr.DIST_OPSET_GUESS.items() for name in sets]
    retime_case, retime_world = next(iter(vr.DIST_OPSET_CASES))
    for case, world, name in [(c, w, "cn") for c, w in cases] + off_cn:
        cs = vr.case(case)
        for route in var_routes:
            base = f"{vr.opset_key(case, name)}/w{world}/{route}"
            want = expected_var(cs, world, route)
            keys = [f"{base}|tile"] + ([f"{base}/e/order={o}|tile" for o in ref.GUESS_ORDERS] if name == "cn" and route in "FS" and (case, world) in vr.DIST_GUESS_CASES else [])
            if name == "cn" and (case, world) == (retime_case, retime_world):
                keys += [f"{base}/retime/{tag}|tile" for tag in ("live0", "live1", "live2", "fresh")]
            if name == "cn" and route in "FS":
                keys += [f"{vr.opset_key(case, g)}/w{world}/{route}/e/order={o}|tile" for c2, w2, g in off_cn_guess if (c2, w2) == (case, world) for o in ref.GUESS_ORDERS]
            for key in keys:
                got = [tuple(int(v) for v in row) for row in data[key]]
                if got != want:
                    routes.append(f"{key}: (beat_pde_tile_route, beat_pde_fused_dist_pass) per rank {got}, expected {want}")
            if any(int(row[0]) for row in data[f"{base}|rr_route"]) or any(int(m[0]) for m in data[f"{base}|merged"]):
                routes.append(f"{base}: a register-row or single-reduction solve on per-node rows")
    if routes:
        return routes, [], figures
    c = Check(data)
    c.failures.extend(str(s) for s in data["slips"])
    for route in var_routes:
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        for case, world in cases:
            cs = vr.case(case)
            base = f"{vr.case_key(case)}/w{world}/{route}"
            check_solves(c, data, base, vr.plain_reference(case), vr.cuts_of(cs, vr.CUTS_SHORT))
            compared = check_ghost_planes(c, data, base, cs.shape, world, coupled=coupled_nodes(cs))
            if case[1] == "full":  # every node of a face couples to the plane behind it
                c.that(compared == 2 * (world - 1) * cs.shape[0] * cs.shape[1] * sum(k in vr.cuts_of(cs, vr.CUTS_SHORT) for k in GHOST_CUTS), base,
                       f"{compared} ghost nodes compared")
            if route in "FS" and (case, world) in vr.DIST_GUESS_CASES:
                check_guess(c, data, base, cs.problem, lambda j, s=cs: vr.field(s, j))
        figures[route] = (c.worst, c.worst_norm)
    for route in var_routes:
        for name in ref.NEW_SETS:
            c.worst, c.worst_norm = (0.0, None), (0.0, None)
            for case, world, _ in [t for t in off_cn if t[2] == name]:
                cs = vr.case(case)
                base = f"{vr.opset_key(case, name)}/w{world}/{route}"
                check_solves(c, data, base, vr.plain_reference(case, name), vr.cuts_of(cs, vr.CUTS_SHORT))
                check_ghost_planes(c, data, base, cs.shape, world, coupled=coupled_nodes(cs))
            for case, world, _ in [t for t in off_cn_guess if t[2] == name and route in "FS"]:
                cs = vr.case(case)
                check_guess(c, data, f"{vr.opset_key(case, name)}/w{world}/{route}", vr.problem_of(case, name), lambda j, s=cs: vr.field(s, j))
            figures[f"{name}/{route}"] = (c.worst, c.worst_norm)
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        cs = vr.case(retime_case)
        check_retime(c, data, f"{vr.case_key(retime_case)}/w{retime_world}/{route}", lambda name: vr.plain_reference(retime_case, name), vr.cuts_of(cs, vr.CUTS_SHORT))
        figures[f"retime/{route}"] = (c.worst, c.worst_norm)
    figures["off theta = 1/2: seconds, solves"] = (float(data["opsets_seconds"]), sum(k.endswith("|x") and ("@" in k or "/retime/" in k) for k in data))
    return [], c.failures, figures


def summary(failures):
    """case/world/loop: number of failures and the first solve that failed, one line each."""
    seen: dict = {}
    for f in failures:
        parts = f.split(":")[0].split("/")
        where = seen.setdefault("/".join(parts[:3]), [0, "/".join(parts[3:])])
        where[0] += 1
    return "\n".join(f"  {k}: {n} (first: {first})" for k, (n, first) in seen.items())


@pytest.mark.parametrize("child", list(CHILDREN))
def test_dist_iterates_match_host_pcg(tmp_path, child):
    out = tmp_path / "out.npz"
    print(run_child(out, child).strip())
    data = dict(np.load(out))
    routes, failures, figures = check_var(data, (child[3:],)) if child.startswith("var") else check_const(data, child)
    assert not routes, f"{len(routes)} solves did not run what they were meant to check ({child}), the first:\n" + "\n".join(routes[:40])
    print(f"{child}: {float(data['seconds']):.2f} s, {sum(k.endswith('|x') for k in data)} solves; per loop (worst err / max(delta_k, floor), key), "
          f"(worst norm err / yardstick, key): {figures}")
    assert not failures, f"{len(failures)} failures ({child}) on\n{summary(failures)}\nthe first:\n" + "\n".join(failures[:40])
