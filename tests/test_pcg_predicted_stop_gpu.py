"""The predicted stop of the register-row PCG (beat_pcg_predict, csrc/beat_pcg_scalar.h).

The pass that forms p_i and sums p.Ap also sums r.Ap and Ap.Ap; the scalar step behind it predicts r_{i+1}.r_{i+1} with a proven
error bound and, when that settles the stopping test, latches the solve so that the residual update of the last iteration is a
no-op.  The prediction feeds no iterate, so an operator created with BEAT_PCG_PREDICT_STOP=0 (the explicit test only) must give
the same iteration counts, reasons, solutions and guess history bit for bit; only the recorded residual norm may differ, in its
last digits.
"""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PR = 6  # the ring of search directions of constant-coefficient operators


@pytest.fixture(autouse=True)
def multi_launch():
    """The register-row loop: grids of a few thousand nodes would otherwise be solved in one launch of one workgroup."""
    from beat._engine import HipOps

    old = HipOps.default_small
    HipOps.default_small = False
    yield
    HipOps.default_small = old


def _ops(ctx, cells, order, predict, dt=0.05):
    from beat import _stencil
    from beat._engine import HipOps

    M = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.1], [0.0, 0.1, 0.5]]) * 1e-3
    old = os.environ.get("BEAT_PCG_PREDICT_STOP")
    os.environ["BEAT_PCG_PREDICT_STOP"] = "1" if predict else "0"  # read when the operator is created
    try:
        ops = HipOps(ctx, tuple(c + 1 for c in cells), True, True, *_stencil.stencil_tables(3, (0.1,) * 3, M))
    finally:
        if old is None:
            del os.environ["BEAT_PCG_PREDICT_STOP"]
        else:
            os.environ["BEAT_PCG_PREDICT_STOP"] = old
    ops.set_guess_order(order)
    ops.set_timestep(0.01, 0.5, dt)
    return ops


def _bump(cells, t):
    x = np.stack(np.meshgrid(*(0.1 * np.arange(c + 1) for c in cells[::-1]), indexing="ij")[::-1], -1).reshape(-1, 3)
    c = np.array([0.4 + 0.6 * t, 0.5, 0.3])
    return -85.0 + 100.0 * np.exp(-((x - c) ** 2).sum(axis=1) / (2 * 0.25**2))


def _history(ctx, ops):
    from beat import _hip

    h0, h1, cnt = C.c_void_p(), C.c_void_p(), C.c_int()
    _hip.check(ops.lib.beat_pde_guess_history(ops.handle, C.byref(h0), C.byref(h1), C.byref(cnt)))
    out = [cnt.value]
    for h in (h0.value, h1.value):
        if h:
            d = ctx.torch.empty(ops.n, dtype=ctx.torch.float64, device=ctx.device)
            _hip.check(ops.lib.beat_copy(ctx.handle, C.c_void_p(d.data_ptr()), C.c_void_p(h), ops.n))
            out.append(d.cpu().numpy())
    return out


def _same(a, b):
    """Two solve records: equal but for the residual norm's last digits."""
    assert a.iterations == b.iterations and a.converged_reason == b.converged_reason, (a, b)
    assert np.isfinite(a.residual_norm) and np.isfinite(b.residual_norm)
    assert a.residual_norm == pytest.approx(b.residual_norm, rel=1e-6, abs=1e-300)
    assert a.rhs_norm == b.rhs_norm


def _run(ctx, cells, order, rtol, atol=1e-50, max_it=500, defer=False, steps=8, t0=0.0):
    """The same sequence of solves on an operator with the predicted stop and one without: records, x, pending update and
    guess history compared after every solve.  Returns the iteration counts."""
    on, off = _ops(ctx, cells, order, True), _ops(ctx, cells, order, False)
    fields = [(ops, ops.new_field(), ops.new_field()) for ops in (on, off)]
    its = []
    for step in range(steps):
        v = _bump(cells, t0 + 0.02 * step)
        res, xs, pend, hist = [], [], [], []
        for ops, fv, fx in fields:
            fv.set(v)
            r = ops.solve_single(fv, [], [], fx, rtol, atol, max_it, defer_flush=defer)
            pend.append(None if ops.pending is None else ops.pending[1:])
            if defer:
                ops.flush_pending()
            res.append(r)
            xs.append(fx.numpy())
            hist.append(_history(ctx, ops))
        _same(*res)
        np.testing.assert_array_equal(xs[0], xs[1])
        assert pend[0] == pend[1]
        assert len(hist[0]) == len(hist[1]) and hist[0][0] == hist[1][0]
        for a, b in zip(hist[0][1:], hist[1][1:]):
            np.testing.assert_array_equal(a, b)
        its.append(res[0].iterations)
    return its


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, -1])
@pytest.mark.parametrize("rtol", [1e-6, 1e-8, 1e-10, 1e-12])
def test_predicted_stop_changes_nothing_but_the_norm(hip_ctx, order, rtol):
    its = _run(hip_ctx, (24, 20, 12), order, rtol, defer=order % 2 == 1)
    assert max(its) >= 1


@pytest.mark.parametrize("cells", [(13, 7, 5), (63, 9, 3), (65, 5, 11), (7, 66, 4)])
@pytest.mark.parametrize("defer", [False, True])
def test_predicted_stop_on_odd_boxes(hip_ctx, cells, defer):
    _run(hip_ctx, cells, 2, 1e-9, defer=defer, steps=5)


def test_predicted_stop_atol_dominated(hip_ctx):
    """atol above rtol ||b||: the stop (and reason 3) comes from the absolute threshold."""
    cells = (24, 20, 12)
    probe = _ops(hip_ctx, cells, 0, False)
    fv, fx = probe.new_field(), probe.new_field()
    fv.set(_bump(cells, 0.0))
    r = probe.solve_single(fv, [], [], fx, 1e-12, 1e-50, 500)
    atol = 1e-6 * r.rhs_norm
    on, off = _ops(hip_ctx, cells, 0, True), _ops(hip_ctx, cells, 0, False)
    res = []
    for ops in (on, off):
        fv, fx = ops.new_field(), ops.new_field()
        fv.set(_bump(cells, 0.0))
        res.append((ops.solve_single(fv, [], [], fx, 1e-12, atol, 500), fx.numpy()))
    _same(res[0][0], res[1][0])
    assert res[0][0].converged_reason == 3
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_predicted_stop_ring_lengths_and_max_it(hip_ctx):
    """Solves of PR - 1, PR, PR + 1 and 2 PR iterations (the ring flush next to the latched iteration), and max_it cut at, and one
    before, the iteration that converges."""
    cells = (24, 20, 12)
    counts = {}
    for rtol in np.logspace(-2, -15, 80):
        its = _run(hip_ctx, cells, 0, float(rtol), steps=1, t0=0.3)
        counts.setdefault(its[0], float(rtol))
    for k in (PR - 1, PR, PR + 1, 2 * PR):
        assert k in counts, sorted(counts)
    for k in (PR - 1, PR, 2 * PR):
        _run(hip_ctx, cells, 0, counts[k], max_it=k, steps=1, t0=0.3)  # converges on its last allowed iteration
        for defer in (False, True):
            recs = []
            for predict in (True, False):
                ops = _ops(hip_ctx, cells, 0, predict)
                fv, fx = ops.new_field(), ops.new_field()
                fv.set(_bump(cells, 0.3))
                fx.fill(0.0)
                r = ops.solve_single(fv, [], [], fx, counts[k], 1e-50, k - 1, defer_flush=defer)
                if defer:
                    ops.flush_pending()
                recs.append((r, fx.numpy()))
            _same(recs[0][0], recs[1][0])
            assert recs[0][0].converged_reason == -3 and recs[0][0].iterations == k - 1
            np.testing.assert_array_equal(recs[0][1], recs[1][1])


def _one_iteration(ctx, cells, predict, rtol, atol):
    ops = _ops(ctx, cells, 0, predict)
    fv, fx = ops.new_field(), ops.new_field()
    fv.set(_bump(cells, 0.5))
    ops.q.fill(float("nan"))  # the residual buffer iteration 0's update writes r_1 into
    r = ops.solve_single(fv, [], [], fx, rtol, atol, 500)
    return r, fx.numpy(), ops.q.numpy()


def test_predicted_stop_skips_the_last_update(hip_ctx):
    """A one-iteration solve: with the prediction conclusive the residual update never runs and leaves its output untouched."""
    cells = (24, 20, 12)
    for rtol in np.logspace(-1, -4, 13):
        r_off, x_off, q_off = _one_iteration(hip_ctx, cells, False, float(rtol), 1e-50)
        if r_off.iterations == 1:
            break
    assert r_off.iterations == 1
    assert np.isfinite(q_off).all()
    r_on, x_on, q_on = _one_iteration(hip_ctx, cells, True, float(rtol), 1e-50)
    _same(r_on, r_off)
    np.testing.assert_array_equal(x_on, x_off)
    assert np.isnan(q_on).all()


def test_predicted_stop_inconclusive_falls_back(hip_ctx):
    """rtol ||b|| placed on the explicit r_1.r_1 itself (atol above it decides convergence): the reason is not settled within the
    prediction's error bound, so the update runs, the explicit test decides and the records agree."""
    cells = (24, 20, 12)
    for rtol in np.logspace(-1, -4, 13):
        r_off, _, _ = _one_iteration(hip_ctx, cells, False, float(rtol), 1e-50)
        if r_off.iterations == 1:
            break
    assert r_off.iterations == 1
    rtol, atol = r_off.residual_norm / r_off.rhs_norm, 2.0 * r_off.residual_norm
    r_off, x_off, _ = _one_iteration(hip_ctx, cells, False, rtol, atol)
    r_on, x_on, q_on = _one_iteration(hip_ctx, cells, True, rtol, atol)
    assert r_off.iterations == 1
    assert np.isfinite(q_on).all()  # the update ran
    assert (r_on.iterations, r_on.converged_reason, r_on.residual_norm) == (r_off.iterations, r_off.converged_reason, r_off.residual_norm)
    np.testing.assert_array_equal(x_on, x_off)


def _bench(out_dir, predict):
    env = dict(os.environ, BEAT_PCG_PREDICT_STOP="1" if predict else "0")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--size", "48", "--nz", "16", "--warmup", "0", "--steps", "20", "--cpu-sample", "0",
           "--no-front", "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    return json.loads(lines[-1]), {f.stem: np.load(f) for f in sorted(Path(out_dir).glob("*.npy"))}


def test_predicted_stop_tp06_steps_bit_identical(tmp_path):
    """20 TP06 splitting steps on a 48 x 48 x 16 slab: the state array is the same bit for bit."""
    _, a = _bench(tmp_path / "on", True)
    _, b = _bench(tmp_path / "off", False)
    assert set(a) == set(b) == {"v", "states"}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
