"""The per-node-coefficient diffusion solve -- the segment-list kernels of csrc/beat_pde_var.hip, the workgroup-tile kernel
vtl_spmv_kernel of csrc/beat_pde_vtl.hip in its single-slab modes (SPMV, fused PDOT, BV, RES) and the opt-in csrc/beat_pde_vrr.hip
-- iterate by iterate against a host PCG, on voxel masks with a fibre field.

A PCG corrects itself (see tests/test_rr_iterates_gpu.py): a doubled or dropped term of p.Ap or r.z, a direction formed wrongly on a
halo lane of the fused pass, a tile partial summed twice, a ring flush one direction short cost an iteration and still converge
to the right x, and tests/test_var_gpu.py's 1e-9 max|v| on a field near -80 hides the rest.  Here every solve of vr.CASES
(tests/_var_ref.py: the host expands the very coefficient rows the device is given, on the tissue nodes) is cut at max_it = 1, 2,
3 and 13 (RING + 1: a full ring of 12 directions flushed and the first direction of the second cycle; 7 under BEAT_VAR_RING=6) and
its ITERATE, iterations, converged_reason (-3), residual_norm and rhs_norm compared with the host's of the same k; uncut solves
(rtol 1e-6, 1e-9) must stop at the host's iteration.  Checks and bounds are those of the other two iterate tests
(tests/_pcg_check.py): err <= 16 max(delta_k, 2^-52 max|x|), delta_k the distance between the host's own float64 and longdouble
runs; no tolerance comes from the device.

Per case, in this process (the switches are read per operator):
  v        zero-mean O(1) noise on the tissue, 1000 + node index off it; x is filled with NaN before every out-of-place solve.
           Afterwards every tissue node is finite (Check.iterate), every node off the tissue holds EXACTLY its v (beat_var_rhs and
           the tile right-hand side copy v to x first; 'copied' and 'untouched' differ here) and v is unchanged;
  in place solve_single(fv, ..., fv, ...) at k = 3 and rtol 1e-9 equals the out-of-place x bit for bit, off-tissue nodes untouched;
  guess    on vr.GUESS_CASES the sequence of the other two tests: four converged solves of a moving field, then a cut solve from
           the extrapolated start, against ref.reference from the host's own extrapolation of the device's increments: the only
           place where the e operand of the tile RES pass and of var_rhs_kernel shows in an iterate;
  routes   each asserted through beat_pde_tile_route (1 tiles | 2 fused PDOT pass | 4 right-hand side on the tiles | 8 ring of 12),
           expected_route below: default 15 on a 3-D box with ny >= 16, 9 on a 3-D box with ny < 16 (tiles of 4 rows carry neither the
           fused pass nor the right-hand side passes), 8 on 2-D and 1-D boxes (the tile plan declines: vtl_sizes_declined, csrc/beat_var_plan.h);
           BEAT_VTL=0 (8: the segment-list kernels), BEAT_VTL_PDOT=0 (the three-kernel iteration), BEAT_VTL_RHS=0 (the gather
           right-hand side), BEAT_VTL_RY=4 (where ny >= 16), BEAT_VTL_RUN=5, BEAT_VTL_DYNAMIC=1, BEAT_VAR_RING=6, and BEAT_VRR=1 with
           BEAT_VRR_RY 2 and 4.  The marching kernel of beat_pde_vrr.hip serves beat_pde_spmv_dot only, which the fused pass
           replaces: its routes set BEAT_VTL_PDOT=0 as well, or on a box with ny >= 16 it would not run at all.
           All routes on vr.ALL_ROUTE_SHAPES with every mask, the default and BEAT_VTL=0 elsewhere.

What it found, on an MI355X: nothing.  All 21 cases passed on every route as the kernels were -- tissue on the box faces, a last
x-segment of one node, runs of planes with gaps of 1, 2 and 3, isolated voxels, solves cut behind a ring flush included.

Measured on an MI355X (1234 solves; the bound on err / max(delta_k, 2^-52 max|x|) is 16, the norms' ratio is to the yardstick of
their bound, which is 16 times it too), the worst over the cases a route runs on:

    route [beat_pde_tile_route on 125 x 18 x 20 / 62 x 9 x 5]    worst err / yardstick                    worst norm / yardstick
    default [15 / 9; 8 on 2-D and 1-D]   3.00  (6 x 4 x 71 layers, k = 1)                     0.37  (63 x 16 x 6 specks, k = 1)
    BEAT_VTL=0 [8]                       3.00  (6 x 4 x 71 layers, k = 1)                     0.35  (6 x 4 x 71 layers, k = 1)
    BEAT_VTL_PDOT=0 [13 / 9]             2.33  (62 x 9 x 5 layers, the stop of rtol 1e-6)     0.25  (62 x 9 x 5 specks, k = 1)
    BEAT_VTL_RHS=0 [11 / 9]              2.33  (the same)                                     0.36  (125 x 18 x 20 full, k = 1)
    BEAT_VTL_RY=4 [9]                    1.81  (125 x 18 x 20 cutshell, guess of order 3, k = 1)  0.16  (125 x 18 x 20 layers, k = 1)
    BEAT_VTL_RUN=5 [15 / 9]              2.33  (62 x 9 x 5 layers, the stop of rtol 1e-6)     0.27  (125 x 18 x 20 specks, k = 1)
    BEAT_VTL_DYNAMIC=1 [15 / 9]          2.33  (the same)                                     0.25  (62 x 9 x 5 specks, k = 1)
    BEAT_VAR_RING=6 [7 / 1]              2.41  (62 x 9 x 5 layers, k = 7)                     0.25  (62 x 9 x 5 specks, k = 1)
    BEAT_VRR=1, BEAT_VRR_RY=2 [13 / 9]   2.33  (62 x 9 x 5 layers, the stop of rtol 1e-6)     0.27  (125 x 18 x 20 cutshell, k = 1)
    BEAT_VRR=1, BEAT_VRR_RY=4 [13 / 9]   2.33  (the same)                                     0.27  (125 x 18 x 20 cutshell, k = 1)

Wall time of the module: 9.0 s, 1.9 s of it the device context; the longest case (125 x 18 x 20 cutshell: ten routes, each with
its guess sequences) 2.8 s, its 280 solves 0.59 s of it, the rest the host's references of the guess cuts; 125 x 18 x 20 full 1.2 s,
every other case under 0.8 s.

The same test against builds with one deliberate arithmetic slip each (wrong numbers; no address, bound or barrier changed):
  the last output lane (x = 61 of a segment) counted twice in a tile's partial of p.q in vtl_spmv_kernel -- the 12 cases on boxes at
      least 62 nodes wide fail on every tile route, from iterate 1 on (125 x 18 x 20 full: off by 9.3e-2; BEAT_VTL=0 passes), the 9
      cases on narrower, 2-D and 1-D boxes pass;
  beta dropped on the halo lanes (0 and 63) of the fused PDOT pass -- the 8 cases on 125 x 18 x 20 and 63 x 16 x 6 fail on the routes
      with the fused pass, from iterate 2 on (63 x 16 x 6 full: 1.4e-3; 125 x 18 x 20 specks: 7e-5), nothing else;
  e not added in the RES pass at the last node of each tile (last output lane, last row, last plane) -- the two guess cases on
      8-row tiles fail (63 x 16 x 6 full, 125 x 18 x 20 cutshell: iterate 1 of the cut behind the sequence off by 7.6 and 9.0), on
      every route with the tile right-hand side; 62 x 9 x 5 layers (gather kernel) and everything without a guess pass;
  the flush of a full ring skipping its oldest direction (var_flush_kernel) -- 20 cases fail at k = 13 (k = 7 under BEAT_VAR_RING=6)
      and at both stops, off by 5 - 6; 2 x 2 x 2, which is never cut behind a flush, passes.

Off theta = 1/2 (vr.OPSET_CASES under be and skew on vr.OPSET_ROUTES; tests/test_rr_iterates_gpu.py says why, and holds the
record of the builds with a deliberate slip): var_form_A_kernel forms the rows of A with theta dt and those of B with
(1 - theta) dt; beat_vtl_rhs reads the rows of B on 8-row tiles, the gather kernel takes c1 / c2.  Measured on an MI355X, the worst
over the three cases (err / yardstick, norm / yardstick):

    route                  be                                                   skew
    default [15 / 9]       2.55 (62 x 9 x 5 layers, guess order 3, k = 1), 0.36   2.29 (62 x 9 x 5 layers, k = 1), 0.14
    BEAT_VTL_PDOT=0        2.55, 0.36                                           2.29, 0.14
    BEAT_VTL=0 [8]         2.01 (62 x 9 x 5 layers, guess order 3, k = 3), 0.14   2.29, 0.14
    re-timed handle (cn, skew, cn) on 63 x 16 x 6 full: 2.01, 0.15 on the tile routes; 1.79, 0.14 under BEAT_VTL=0

The module: 8.7 s with the 9 new tests, 7.8 s for the 21 before them, same session.  What it found: nothing.
"""
import time

import numpy as np
import pytest

import _pcg_ref as ref
import _var_ref as vr
from _pcg_check import Check

pytestmark = pytest.mark.gpu

NO_STOP = dict(rtol=1e-30, atol=1e-300)  # nothing but max_it ends a cut solve
MAX_IT = 500
IN_PLACE = ("k=3", "rtol=1e-09")
SWITCHES = ("BEAT_VTL", "BEAT_VTL_RHS", "BEAT_VTL_PDOT", "BEAT_VTL_RY", "BEAT_VTL_RUN", "BEAT_VTL_DYNAMIC", "BEAT_VTL_ALIGN", "BEAT_VRR",
            "BEAT_VRR_RY", "BEAT_VRR_PF", "BEAT_VRR_RUN", "BEAT_VAR_RING")
ROUTES = {
    "default": {},
    "rows": {"BEAT_VTL": "0"},
    "three": {"BEAT_VTL_PDOT": "0"},
    "gather": {"BEAT_VTL_RHS": "0"},
    "ry4": {"BEAT_VTL_RY": "4"},
    "run5": {"BEAT_VTL_RUN": "5"},
    "dynamic": {"BEAT_VTL_DYNAMIC": "1"},
    "ring6": {"BEAT_VAR_RING": "6"},
    "vrr2": {"BEAT_VRR": "1", "BEAT_VRR_RY": "2", "BEAT_VTL_PDOT": "0"},
    "vrr4": {"BEAT_VRR": "1", "BEAT_VRR_RY": "4", "BEAT_VTL_PDOT": "0"},
}


def routes_of(shape) -> list:
    if tuple(shape) not in vr.ALL_ROUTE_SHAPES:
        return ["default", "rows"]
    return [r for r in ROUTES if r != "ry4" or shape[1] >= 16]


def expected_route(shape, route: str) -> int:
    """beat_pde_tile_route of a single slab, from beat_vtl_setup, beat_vtl_pdot_available, beat_vtl_rhs_available and
    beat_pde_create_var, written out."""
    tiles = min(shape) >= 2 and route != "rows"
    ry8 = tiles and shape[1] >= 16 and route != "ry4"
    pdot = ry8 and "BEAT_VTL_PDOT" not in ROUTES[route]
    rhs = ry8 and route != "gather"
    return (1 if tiles else 0) | (2 if pdot else 0) | (4 if rhs else 0) | (0 if route == "ring6" else 8)


def cuts_of(cs, route: str) -> tuple:
    return vr.cuts_of(cs, vr.CUTS_SHORT if route == "ring6" else vr.CUTS)


def make_ops(ctx, cs, route, monkeypatch, order=0, opset="cn"):
    from beat._engine import HipOps

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in ROUTES[route].items():
        monkeypatch.setenv(name, value)
    ops = HipOps(ctx, cs.shape, True, True, cs.mass_rows, cs.stiff_rows, per_node=True)  # the rows the host reference expands
    ops.set_guess_order(order)
    ops.set_timestep(*ref.opset(opset).triple)
    got, want = int(ctx.lib.beat_pde_tile_route(ops.handle)), expected_route(cs.shape, route)
    assert got == want, f"{vr.case_key((cs.shape, cs.mask))}/{route}: beat_pde_tile_route {got}, expected {want}"
    assert not ops.small_active()
    return ops


def stimuli(ops, cs):
    ws = []
    for w in vr.weights_on_box(cs):
        f = ops.new_field()
        f.set(w)
        ws.append(f)
    return ws


def record(data, slips, cs, key, res, fx, v_box):
    """x on the tissue and the solve's record; every node off the tissue must hold exactly its v."""
    x = fx.numpy().copy()
    off = ~cs.tissue
    if not np.array_equal(x[off], v_box[off]):
        bad = np.nonzero(off & ~(x == v_box))[0]
        slips.append(f"{key}: {len(bad)} nodes off the tissue do not hold their v, the first: node {bad[0]} holds {x[bad[0]]!r}")
    data[f"{key}|x"] = x[cs.tissue]
    data[f"{key}|rec"] = np.array([res.iterations, res.converged_reason, res.residual_norm, res.rhs_norm], dtype=np.float64)


def run_plain(ctx, cs, route, data, slips, monkeypatch, opset="cn"):
    ops = make_ops(ctx, cs, route, monkeypatch, opset=opset)
    base = f"{vr.opset_key((cs.shape, cs.mask), opset)}/{route}"
    v_box = vr.on_box(cs, vr.field(cs))
    fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, cs)
    fv.set(v_box)
    settings = {f"k={k}": dict(max_it=k, **NO_STOP) for k in cuts_of(cs, route)}
    settings.update({f"rtol={rtol:g}": dict(max_it=MAX_IT, rtol=rtol, atol=1e-300) for rtol in ref.RTOLS})
    assert set(IN_PLACE) <= set(settings)
    for tail, kw in settings.items():
        fx.fill(float("nan"))
        record(data, slips, cs, f"{base}/{tail}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, kw["rtol"], kw["atol"], kw["max_it"]), fx, v_box)
        if not np.array_equal(fv.numpy(), v_box):
            slips.append(f"{base}/{tail}: the solve changed v")
    for tail in IN_PLACE:
        kw = settings[tail]
        record(data, slips, cs, f"{base}/inplace/{tail}", ops.solve_single(fv, ws, ref.STIM_AMPS, fv, kw["rtol"], kw["atol"], kw["max_it"]), fv, v_box)
        fv.set(v_box)
    assert ops.pending is None


def run_guess(ctx, cs, route, data, slips, monkeypatch, opset="cn"):
    """Four converged solves of a field that moves between solves, then a cut solve that starts from their extrapolation."""
    for order in ref.GUESS_ORDERS:
        ops = make_ops(ctx, cs, route, monkeypatch, order=order, opset=opset)
        key = f"{vr.opset_key((cs.shape, cs.mask), opset)}/{route}/e/order={order}"
        fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, cs)
        for k in ref.GUESS_CUTS:
            ops.guess_reset()
            for j in range(1, ref.GUESS_SOLVES + 1):
                v_box = vr.on_box(cs, vr.field(cs, j))
                fv.set(v_box)
                fx.fill(float("nan"))
                record(data, slips, cs, f"{key}/k={k}/solve={j}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, ref.GUESS_RTOL, 1e-300, MAX_IT), fx, v_box)
            v_box = vr.on_box(cs, vr.field(cs, ref.GUESS_SOLVES + 1))
            fv.set(v_box)
            fx.fill(float("nan"))
            record(data, slips, cs, f"{key}/k={k}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP), fx, v_box)


def check_plain(c, cs, route, opset="cn"):
    base, r = f"{vr.opset_key((cs.shape, cs.mask), opset)}/{route}", vr.plain_reference((cs.shape, cs.mask), opset)
    for k in cuts_of(cs, route):
        c.cut(f"{base}/k={k}", r, k)
    for rtol in ref.RTOLS:
        c.uncut(f"{base}/rtol={rtol:g}", r, rtol)
    for tail in IN_PLACE:
        c.same_bits(f"{base}/{tail}", f"{base}/inplace/{tail}", True)


def check_guess(c, cs, route, references, opset="cn"):
    """As check_guess of tests/test_small_iterates_gpu.py: the device's own earlier, converged solves of the sequence supply the
    increments; they are not what is compared.  Routes whose earlier solves are the same bits share a reference."""
    p = vr.problem_of((cs.shape, cs.mask), opset)
    v = vr.field(cs, ref.GUESS_SOLVES + 1)
    for order in ref.GUESS_ORDERS:
        for k in ref.GUESS_CUTS:
            key = f"{vr.opset_key((cs.shape, cs.mask), opset)}/{route}/e/order={order}/k={k}"
            incs = [c.data[f"{key}/solve={j}|x"] - vr.field(cs, j) for j in range(ref.GUESS_SOLVES, 0, -1)]
            c.that(all(c.rec(f"{key}/solve={j}")[1] > 0 for j in range(1, ref.GUESS_SOLVES + 1)), key, "a solve in front of the cut did not converge")
            if not all(np.isfinite(i).all() for i in incs):
                c.that(False, key, "a solve in front of the cut left x not finite")
                continue
            memo = (order, k, *(i.tobytes() for i in incs[:order]))
            if memo not in references:
                if "bL" not in references:
                    references["bL"] = ref.rhs_longdouble(p, v)
                x0 = v.astype(np.longdouble) + ref.guess_increment(order, incs)
                references[memo] = ref.reference(p, references["bL"], x0, k)
            c.cut(key, references[memo], k)


WORST: dict = {}  # route -> (worst err / yardstick, key), (worst norm err / yardstick, key) over the cases run so far


@pytest.mark.parametrize("case", vr.CASES, ids=vr.case_key)
def test_per_node_iterates_match_host_pcg(hip_ctx, case, monkeypatch):
    cs = vr.case(case)
    vr.plain_reference(case)  # (not part of the device's time)
    data, slips = {}, []
    routes = routes_of(cs.shape)
    t0 = time.perf_counter()
    for route in routes:
        run_plain(hip_ctx, cs, route, data, slips, monkeypatch)
        if case in vr.GUESS_CASES:
            run_guess(hip_ctx, cs, route, data, slips, monkeypatch)
    hip_ctx.synchronize()
    seconds = time.perf_counter() - t0
    c = Check(data)
    c.failures.extend(slips)
    references: dict = {}
    lines = []
    for route in routes:
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        check_plain(c, cs, route)
        if case in vr.GUESS_CASES:
            check_guess(c, cs, route, references)
        lines.append(f"{route} [{expected_route(cs.shape, route)}] {c.worst[0]:.2f} ({c.worst[1]}), {c.worst_norm[0]:.2f} ({c.worst_norm[1]})")
        old = WORST.get(route, ((0.0, None), (0.0, None)))
        WORST[route] = (max(old[0], c.worst, key=lambda w: w[0]), max(old[1], c.worst_norm, key=lambda w: w[0]))
    print(f"var iterates {vr.case_key(case)}: {cs.n} of {cs.n_nodes} nodes, {sum(k.endswith('|x') for k in data)} solves in {1e3 * seconds:.1f} ms; "
          "route [beat_pde_tile_route] err / max(delta_k, floor) and norm err / yardstick:\n  " + "\n  ".join(lines))
    print("  so far, per route: " + "; ".join(f"{r} {w[0][0]:.2f} ({w[0][1]}), {w[1][0]:.2f} ({w[1][1]})" for r, w in WORST.items()))
    assert not c.failures, f"{len(c.failures)} failures on {vr.case_key(case)}, the first:\n" + "\n".join(c.failures[:40])


OFF_CN = [(case, name) for case in vr.OPSET_CASES for name in ref.NEW_SETS]
WORST_OFF_CN: dict = {}  # (set, route) -> as WORST


@pytest.mark.parametrize("pair", OFF_CN, ids=lambda pair: vr.opset_key(*pair))
def test_per_node_iterates_match_host_pcg_off_theta_one_half(hip_ctx, pair, monkeypatch):
    """The test above on vr.OPSET_CASES under be and skew, on vr.OPSET_ROUTES: the default route and BEAT_VTL_PDOT=0 form b on the
    8-row tiles from the rows of B that var_form_A_kernel wrote (beat_vtl_rhs), BEAT_VTL=0 -- and every route of a box with ny < 16 --
    by the gather kernel from c1 / c2 (beat_var_rhs).  The route is asserted (make_ops) before any value."""
    case, name = pair
    cs = vr.case(case)
    vr.plain_reference(case, name)  # (not part of the device's time)
    data, slips = {}, []
    guess = case in vr.OPSET_GUESS_CASES
    t0 = time.perf_counter()
    for route in vr.OPSET_ROUTES:
        run_plain(hip_ctx, cs, route, data, slips, monkeypatch, name)
        if guess:
            run_guess(hip_ctx, cs, route, data, slips, monkeypatch, name)
    hip_ctx.synchronize()
    seconds = time.perf_counter() - t0
    c = Check(data)
    c.failures.extend(slips)
    references: dict = {}
    lines = []
    for route in vr.OPSET_ROUTES:
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        check_plain(c, cs, route, name)
        if guess:
            check_guess(c, cs, route, references, name)
        lines.append(f"{route} [{expected_route(cs.shape, route)}] {c.worst[0]:.2f} ({c.worst[1]}), {c.worst_norm[0]:.2f} ({c.worst_norm[1]})")
        old = WORST_OFF_CN.get((name, route), ((0.0, None), (0.0, None)))
        WORST_OFF_CN[(name, route)] = (max(old[0], c.worst, key=lambda w: w[0]), max(old[1], c.worst_norm, key=lambda w: w[0]))
    print(f"var iterates {vr.opset_key(case, name)}: {cs.n} of {cs.n_nodes} nodes, {sum(k.endswith('|x') for k in data)} solves in {1e3 * seconds:.1f} ms; "
          "route [beat_pde_tile_route] err / max(delta_k, floor) and norm err / yardstick:\n  " + "\n  ".join(lines))
    print("  so far, per set and route: " + "; ".join(f"{r} {w[0][0]:.2f} ({w[0][1]}), {w[1][0]:.2f} ({w[1][1]})" for r, w in WORST_OFF_CN.items()))
    assert not c.failures, f"{len(c.failures)} failures on {vr.opset_key(case, name)}, the first:\n" + "\n".join(c.failures[:40])


def cut_sequence(ops, data, slips, cs, key, fv, fx, ws, v_box):
    """The cuts one after another with NO guess_reset between them: the first starts from x0 = v_ only if the history is empty."""
    for k in vr.cuts_of(cs, vr.CUTS):
        fx.fill(float("nan"))
        record(data, slips, cs, f"{key}/k={k}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP), fx, v_box)


@pytest.mark.parametrize("route", vr.OPSET_ROUTES)
def test_retimed_handle_equals_a_fresh_one(hip_ctx, route, monkeypatch):
    """beat_pde_set_timestep on a live per-node handle (ref.RETIME: cn, skew, cn) with a guess of order 3 and a full history:
    var_form_A_kernel runs again.  The cut sequence behind each re-timing starts from x0 = v_ (its first iterate is the plain
    reference's), equals that of a handle created under the set bit for bit, and back under cn what the handle gave before."""
    case = vr.OPSET_CASES[0]
    cs = vr.case(case)
    data, slips = {}, []
    v_box = vr.on_box(cs, vr.field(cs))
    ops = make_ops(hip_ctx, cs, route, monkeypatch, order=3, opset=ref.RETIME[0])
    fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, cs)
    fv.set(v_box)
    cut_sequence(ops, data, slips, cs, "live0", fv, fx, ws, v_box)
    for stage, name in enumerate(ref.RETIME[1:], start=1):
        for j in range(1, ref.GUESS_SOLVES + 1):
            fv.set(vr.on_box(cs, vr.field(cs, j)))
            assert ops.solve_single(fv, ws, ref.STIM_AMPS, fx, ref.GUESS_RTOL, 1e-300, MAX_IT).converged_reason > 0
        fv.set(v_box)
        ops.set_timestep(*ref.opset(name).triple)  # drops the history: no guess_reset here
        assert int(hip_ctx.lib.beat_pde_tile_route(ops.handle)) == expected_route(cs.shape, route)
        cut_sequence(ops, data, slips, cs, f"live{stage}", fv, fx, ws, v_box)
    fresh = make_ops(hip_ctx, cs, route, monkeypatch, order=3, opset=ref.RETIME[1])
    fv2, fx2, ws2 = fresh.new_field(), fresh.new_field(), stimuli(fresh, cs)
    fv2.set(v_box)
    cut_sequence(fresh, data, slips, cs, "fresh", fv2, fx2, ws2, v_box)
    c = Check(data)
    c.failures.extend(slips)
    k0 = vr.CUTS[0]
    for stage, name in enumerate(ref.RETIME):
        c.cut(f"live{stage}/k={k0}", vr.plain_reference(case, name), k0)
    c.cut(f"fresh/k={k0}", vr.plain_reference(case, ref.RETIME[1]), k0)
    for k in vr.cuts_of(cs, vr.CUTS):
        for mine, other in ((f"live1/k={k}", f"fresh/k={k}"), (f"live2/k={k}", f"live0/k={k}")):
            c.same_bits(other, mine, True)
            c.that(data[f"{mine}|rec"].tobytes() == data[f"{other}|rec"].tobytes(), mine, f"record {data[f'{mine}|rec'].tolist()}, {other} {data[f'{other}|rec'].tolist()}")
        c.that(not np.array_equal(data[f"live0/k={k}|x"], data[f"live1/k={k}|x"]), f"live1/k={k}", "the re-timing changed nothing")
    print(f"var retime {route}: err / yardstick {c.worst}, norm {c.worst_norm}")
    assert not c.failures, f"{len(c.failures)} failures, the first:\n" + "\n".join(c.failures[:40])
