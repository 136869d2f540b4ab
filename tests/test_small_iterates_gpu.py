"""The one-launch diffusion solve (pcg_small_kernel<M> of csrc/beat_pde_small.hip: right-hand side, every PCG iteration and the x
update in one 512-thread workgroup) iterate by iterate against a host PCG, and the multi-launch kernels on the same boxes.

A PCG corrects itself (see tests/test_rr_iterates_gpu.py): a doubled or dropped term of p.Ap or r.D^-1 r, a node owned by two
threads or by none, a partial-sum buffer read one barrier early cost an iteration and still converge to the right x, so comparing
the converged solution with the multi-launch kernels' cannot see them.  Here every solve of ref.SMALL_SHAPES is cut at max_it = 1,
2, 3, 7 and its ITERATE compared with the host's (tests/_pcg_ref.py, in longdouble) of the same k; uncut solves must stop at the
host's iteration.  The checks and bounds are those of the register-row test (tests/_pcg_check.py): err <= 16 max(delta_k, 2^-52
max|x|) with delta_k the distance between the host's own float64 and longdouble runs; no tolerance comes from the device.

Per shape, in this process (BEAT_SMALL is on by default), each operator given ref.tables(dim):
  route    small_active() is what ref.small_takes says: every template instance <2> ... <16> is launched, 64 x 95 x 1 (LDS) and the
           boxes with an axis of one node in front of a longer one (1 x 1 x 7, 1 x 5 x 4, 6 x 1 x 5, 1 x 9 x 1) are declined;
  one/     the operator as created -- the one-launch solve wherever it is taken: cut and uncut solves, x poisoned with NaN, two
           stimuli;
  multi/   the same after set_small(False): the route the declined boxes end up on must be right too;
  in place solve_single(fv, ..., fv, ...) at k = 3 and rtol 1e-9 equals the out-of-place x bit for bit (beat_split_steps only ever
           calls the kernel in place);
  guess    on ref.SMALL_GUESS_SHAPES the sequence (e) of the register-row test: four converged solves, then a cut solve from the
           extrapolated start (the kernel's use_e branch and its beat_guess_record), against ref.reference from the same start.

What it found, on an MI355X: with the four collapsed-axis boxes still taken by the one-launch solve, every check of theirs failed on
that route -- max|x_dev - x_1| = 0.52 (1 x 1 x 7), 0.87 (1 x 5 x 4), 0.37 (6 x 1 x 5), 0.74 (1 x 9 x 1) for max|x| of about 2,
rhs_norm off by 5 - 30 %, 7 - 39 iterations where the host takes 4 - 11 -- as the flat neighbour index predicts (the single linear
offset of a stencil point outside the box is that of a node inside it; tests/test_pcg_ref_cpu.py emulates it), while the multi-launch
kernels gave the host's iterates on all four.  beat_small_available now declines them; the other 14 boxes passed as they were.

Measured on an MI355X (448 solves; the bound on err / max(delta_k, 2^-52 max|x|) is 16, the norms' ratio is to the yardstick of
their bound, which is 16 times it too):

    route                         worst err / yardstick                         worst norm / yardstick
    one-launch, 13 boxes          2.15  (3 x 3 x 57, the stop of rtol 1e-9)     0.22  (64 x 32 x 1, guess of order 3, k = 1)
    multi-launch, those 13        2.10  (5 x 5 x 41, k = 1)                     0.21  (5 x 5 x 41, k = 1)
    the 5 declined boxes          2.09  (1 x 5 x 4, k = 7)                      0.50  (1 x 5 x 4, k = 1)

Per instance, one-launch: <2> 2.15, <4> 1.82, <6> 1.46, <8> 1.75, <10> 1.80, <12> 1.40, <16> 1.44.  Wall time of the module: 3.8 s,
1.8 s of it the device context; the longest case (32 x 16 x 16 with its guess sequences) 0.25 s, its 56 solves 30 ms.
The same test against builds with one deliberate slip each in the kernel: the last node counted twice in p.Ap -- the 13 one-launch
boxes fail (128 x 2 x 2: iterate 1 off by 8e-3); node 0 counted twice in r.r -- the same 13 fail (residual_norm); e not added to
the start at the last node -- the four guess boxes fail, nothing else.

Off theta = 1/2 (ref.SMALL_OPSET_SHAPES under be and skew; tests/test_rr_iterates_gpu.py says why, and holds the record of the
builds with a deliberate slip): the kernel forms b, ||b|| and A from its own LDS copies of tables A and B.  Measured on an MI355X
(worst err / yardstick, worst norm / yardstick; one-launch | multi-launch):

    41 x 15 x 7 <10>    be    1.74, 0.28 | 1.53, 0.19    skew  2.05, 0.22 | 1.90, 0.19     56 solves each, 22 - 25 ms
    64 x 32 x 1 <4>     be    1.96, 0.16 | 1.27, 0.14    skew  1.67, 0.28 | 1.53, 0.12     56 solves each, 17 - 24 ms
    1 x 5 x 4 declined  be    1.22, 0.16 on both         skew  2.36, 0.09 on both          16 solves each, 4 ms
    re-timed handle (cn, skew, cn) on 41 x 15 x 7: 2.05, 0.22 one-launch; 1.85, 0.12 multi-launch

The module: 4.0 s with the 8 new tests, 3.5 s for the 18 before them, same session.  What it found: nothing.
"""
import time

import numpy as np
import pytest

import _pcg_ref as ref
from _pcg_check import Check

pytestmark = pytest.mark.gpu

NO_STOP = dict(rtol=1e-30, atol=1e-300)  # nothing but max_it ends a cut solve
MAX_IT = 500
IN_PLACE = ("k=3", "rtol=1e-09")


def make_ops(ctx, shape, small, order=0, opset="cn"):
    from beat._engine import HipOps

    mt, kt = ref.tables(ref.dim_of(shape))  # the numbers the host reference expands into its matrices
    ops = HipOps(ctx, shape, True, True, mt, kt)
    if not small:
        ops.set_small(False)
    ops.set_guess_order(order)
    ops.set_timestep(*ref.opset(opset).triple)
    return ops


def stimuli(ops, shape):
    ws = []
    for w in ref.problem(shape).weights:
        f = ops.new_field()
        f.set(w)
        ws.append(f)
    return ws


def record(data, key, res, fx):
    data[f"{key}|x"] = fx.numpy().copy()
    data[f"{key}|rec"] = np.array([res.iterations, res.converged_reason, res.residual_norm, res.rhs_norm], dtype=np.float64)


def run_plain(ctx, shape, route, data, opset="cn"):
    ops = make_ops(ctx, shape, route == "one", opset=opset)
    assert ops.small_active() == (route == "one" and ref.small_takes(shape)), (shape, route, ops.small_active())
    base = f"{ref.case_key(shape, opset)}/{route}"
    v = ref.field(shape)
    fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, shape)
    fv.set(v)
    settings = {f"k={k}": dict(max_it=k, **NO_STOP) for k in ref.CUTS}
    settings.update({f"rtol={rtol:g}": dict(max_it=MAX_IT, rtol=rtol, atol=1e-300) for rtol in ref.RTOLS})
    assert set(IN_PLACE) <= set(settings)
    for tail, kw in settings.items():
        fx.fill(float("nan"))
        record(data, f"{base}/{tail}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, kw["rtol"], kw["atol"], kw["max_it"]), fx)
        assert np.array_equal(fv.numpy(), v), f"{base}/{tail}: the solve changed v"
    for tail in IN_PLACE:
        kw = settings[tail]
        record(data, f"{base}/inplace/{tail}", ops.solve_single(fv, ws, ref.STIM_AMPS, fv, kw["rtol"], kw["atol"], kw["max_it"]), fv)
        fv.set(v)
    assert ops.pending is None


def run_guess(ctx, shape, route, data, opset="cn"):
    """(e): four converged solves of a field that moves between solves, then a cut solve that starts from their extrapolation."""
    for order in ref.GUESS_ORDERS:
        ops = make_ops(ctx, shape, route == "one", order=order, opset=opset)
        assert ops.small_active() == (route == "one")
        key = f"{ref.case_key(shape, opset)}/{route}/e/order={order}"
        fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, shape)
        for k in ref.GUESS_CUTS:
            ops.guess_reset()
            for j in range(1, ref.GUESS_SOLVES + 1):
                fv.set(ref.field(shape, j))
                fx.fill(float("nan"))
                record(data, f"{key}/k={k}/solve={j}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, ref.GUESS_RTOL, 1e-300, MAX_IT), fx)
            fv.set(ref.field(shape, ref.GUESS_SOLVES + 1))
            fx.fill(float("nan"))
            record(data, f"{key}/k={k}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP), fx)


def check_plain(c, shape, route, opset="cn"):
    base, r = f"{ref.case_key(shape, opset)}/{route}", ref.plain_reference(shape, opset)
    for k in ref.CUTS:
        c.cut(f"{base}/k={k}", r, k)
    for rtol in ref.RTOLS:
        c.uncut(f"{base}/rtol={rtol:g}", r, rtol)
    for tail in IN_PLACE:
        c.same_bits(f"{base}/{tail}", f"{base}/inplace/{tail}", True)


def check_guess(c, shape, route, opset="cn"):
    """As check_results of tests/test_rr_iterates_gpu.py: the device's own earlier, converged solves of the sequence supply the
    increments; they are not what is compared."""
    p = ref.problem(shape, opset)
    v = ref.field(shape, ref.GUESS_SOLVES + 1)
    bL = ref.rhs_longdouble(p, v)
    for order in ref.GUESS_ORDERS:
        for k in ref.GUESS_CUTS:
            key = f"{ref.case_key(shape, opset)}/{route}/e/order={order}/k={k}"
            incs = [c.data[f"{key}/solve={j}|x"] - ref.field(shape, j) for j in range(ref.GUESS_SOLVES, 0, -1)]
            c.that(all(c.rec(f"{key}/solve={j}")[1] > 0 for j in range(1, ref.GUESS_SOLVES + 1)), key, "a solve in front of the cut did not converge")
            x0 = v.astype(np.longdouble) + ref.guess_increment(order, incs)
            c.cut(key, ref.reference(p, bL, x0, k), k)


@pytest.mark.parametrize("shape", list(ref.SMALL_SHAPES), ids=ref.shape_key)
def test_small_iterates_match_host_pcg(hip_ctx, shape):
    data: dict = {}
    ref.plain_reference(shape)  # (not part of the device's time)
    t0 = time.perf_counter()
    for route in ("one", "multi"):
        run_plain(hip_ctx, shape, route, data)
        if shape in ref.SMALL_GUESS_SHAPES:
            run_guess(hip_ctx, shape, route, data)
    hip_ctx.synchronize()
    seconds = time.perf_counter() - t0
    c = Check(data)
    worst = {}
    for route in ("one", "multi"):
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        check_plain(c, shape, route)
        if shape in ref.SMALL_GUESS_SHAPES:
            check_guess(c, shape, route)
        worst[route] = (c.worst, c.worst_norm)
    taken = ref.small_takes(shape)
    print(f"small iterates {ref.shape_key(shape)}: {'<%d>' % ref.small_instance(shape) if taken else 'declined'}, "
          f"{sum(k.endswith('|x') for k in data)} solves in {1e3 * seconds:.1f} ms; err / max(delta_k, floor) and norm err / yardstick: "
          + "; ".join(f"{route} {worst[route][0][0]:.2f} ({worst[route][0][1]}), {worst[route][1][0]:.2f} ({worst[route][1][1]})" for route in worst))
    assert not c.failures, f"{len(c.failures)} failures on {ref.shape_key(shape)}, the first:\n" + "\n".join(c.failures[:40])


OFF_CN = [(shape, name) for shape, sets in ref.SMALL_OPSET_SHAPES.items() for name in sets]


@pytest.mark.parametrize("pair", OFF_CN, ids=lambda pair: ref.case_key(*pair))
def test_small_iterates_match_host_pcg_off_theta_one_half(hip_ctx, pair):
    """The test above on the pairs of ref.SMALL_OPSET_SHAPES: the one-launch kernel forms b, ||b|| and A from its own copies of the
    two tables, and 1 x 5 x 4, which it declines, runs the multi-launch kernels on both routes."""
    shape, name = pair
    data: dict = {}
    ref.plain_reference(shape, name)  # (not part of the device's time)
    guess = shape in ref.SMALL_OPSET_GUESS_SHAPES
    t0 = time.perf_counter()
    for route in ("one", "multi"):
        run_plain(hip_ctx, shape, route, data, name)
        if guess:
            run_guess(hip_ctx, shape, route, data, name)
    hip_ctx.synchronize()
    seconds = time.perf_counter() - t0
    c = Check(data)
    worst = {}
    for route in ("one", "multi"):
        c.worst, c.worst_norm = (0.0, None), (0.0, None)
        check_plain(c, shape, route, name)
        if guess:
            check_guess(c, shape, route, name)
        worst[route] = (c.worst, c.worst_norm)
    print(f"small iterates {ref.case_key(shape, name)}: {'<%d>' % ref.small_instance(shape) if ref.small_takes(shape) else 'declined'}, "
          f"{sum(k.endswith('|x') for k in data)} solves in {1e3 * seconds:.1f} ms; err / max(delta_k, floor) and norm err / yardstick: "
          + "; ".join(f"{route} {worst[route][0][0]:.2f} ({worst[route][0][1]}), {worst[route][1][0]:.2f} ({worst[route][1][1]})" for route in worst))
    assert not c.failures, f"{len(c.failures)} failures on {ref.case_key(shape, name)}, the first:\n" + "\n".join(c.failures[:40])


def cut_sequence(ops, data, key, fv, fx, ws):
    """The cuts one after another with NO guess_reset between them: the first starts from x0 = v_ only if the history is empty."""
    for k in ref.CUTS:
        fx.fill(float("nan"))
        record(data, f"{key}/k={k}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP), fx)


@pytest.mark.parametrize("route", ("one", "multi"))
def test_retimed_handle_equals_a_fresh_one(hip_ctx, route):
    """beat_pde_set_timestep on a live handle (ref.RETIME: cn, skew, cn) with a guess of order 3 and a full history: the cut sequence
    behind each re-timing starts from x0 = v_ (its first iterate is the plain reference's), equals that of a handle created under the
    set bit for bit, and back under cn what the handle gave before."""
    shape = next(iter(ref.SMALL_OPSET_SHAPES))
    small = route == "one"
    data: dict = {}
    v = ref.field(shape)
    ops = make_ops(hip_ctx, shape, small, order=3, opset=ref.RETIME[0])
    assert ops.small_active() == small
    fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, shape)
    fv.set(v)
    cut_sequence(ops, data, "live0", fv, fx, ws)
    for stage, name in enumerate(ref.RETIME[1:], start=1):
        for j in range(1, ref.GUESS_SOLVES + 1):
            fv.set(ref.field(shape, j))
            assert ops.solve_single(fv, ws, ref.STIM_AMPS, fx, ref.GUESS_RTOL, 1e-300, MAX_IT).converged_reason > 0
        fv.set(v)
        ops.set_timestep(*ref.opset(name).triple)  # drops the history: no guess_reset here
        assert ops.small_active() == small
        cut_sequence(ops, data, f"live{stage}", fv, fx, ws)
    fresh = make_ops(hip_ctx, shape, small, order=3, opset=ref.RETIME[1])
    fv2, fx2, ws2 = fresh.new_field(), fresh.new_field(), stimuli(fresh, shape)
    fv2.set(v)
    cut_sequence(fresh, data, "fresh", fv2, fx2, ws2)
    c = Check(data)
    for stage, name in enumerate(ref.RETIME):
        c.cut(f"live{stage}/k={ref.CUTS[0]}", ref.plain_reference(shape, name), ref.CUTS[0])
    c.cut(f"fresh/k={ref.CUTS[0]}", ref.plain_reference(shape, ref.RETIME[1]), ref.CUTS[0])
    for k in ref.CUTS:
        for mine, other in ((f"live1/k={k}", f"fresh/k={k}"), (f"live2/k={k}", f"live0/k={k}")):
            c.same_bits(other, mine, True)
            c.that(data[f"{mine}|rec"].tobytes() == data[f"{other}|rec"].tobytes(), mine, f"record {data[f'{mine}|rec'].tolist()}, {other} {data[f'{other}|rec'].tolist()}")
        c.that(not np.array_equal(data[f"live0/k={k}|x"], data[f"live1/k={k}|x"]), f"live1/k={k}", "the re-timing changed nothing")
    print(f"small retime {route}: err / yardstick {c.worst}, norm {c.worst_norm}")
    assert not c.failures, f"{len(c.failures)} failures, the first:\n" + "\n".join(c.failures[:40])
