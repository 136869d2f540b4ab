"""The cases of tests/_pcg_ref.py on the device, in a process of its own: BEAT_RR_RY, BEAT_RR_PD and BEAT_RR_BY_ROWS are read once
per process, so tests/test_rr_iterates_gpu.py starts one interpreter per setting, with the setting in the environment.

    python _rr_iterates_script.py out.npz

Every operator must report (beat_pde_rr_route) the instance of the register-row kernels the environment asked for, and be on the
register-row loop at all -- or the LDS-tiled loop would be tested in its place without anybody noticing.  Writes, per case key,
x, the solve's record (iterations, converged_reason, residual_norm, rhs_norm) and the route report.  Computes no reference.

The children of (RY 2, PD 1) and (RY 4, PD 1) without BEAT_RR_BY_ROWS also run the pairs of ref.OPSET_SHAPES -- the operator off
theta = 1/2, keys shape@set -- and the re-timing of a live handle (run_retime)."""
import os
import random
import socket
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import _pcg_ref as ref  # noqa: E402
from beat._device import Context  # noqa: E402
from beat._engine import DiffusionSolver, HipOps, Slab  # noqa: E402

WANT = {"ry": int(os.environ["BEAT_RR_RY"]), "pd": int(os.environ["BEAT_RR_PD"]), "by_rows_mask": int(os.environ.get("BEAT_RR_BY_ROWS", "0"))}
NO_STOP = dict(rtol=1e-30, atol=1e-300)  # nothing but max_it ends a cut solve
MAX_IT = 500
out: dict = {}
shared = {"libcomm": None}


def _free_port():
    for _ in range(64):  # below the kernel's ephemeral range (see tests/test_distributed_gpu.py)
        port = random.randint(20000, 32000)
        with socket.socket() as s:
            try:
                s.bind(("127.0.0.1", port))
            except OSError:
                continue
            return port
    raise RuntimeError("no free port")


def make_ops(ctx, shape, predict=True, order=0, opset="cn"):
    mt, kt = ref.tables(ref.SHAPES[shape])  # the numbers the host reference expands into its matrices
    os.environ["BEAT_PCG_PREDICT_STOP"] = "1" if predict else "0"  # read when the operator is created
    try:
        ops = HipOps(ctx, shape, True, True, mt, kt)
    finally:
        del os.environ["BEAT_PCG_PREDICT_STOP"]
    ops.set_small(False)  # the one-launch solve of small grids off: the multi-launch loop
    ops.set_guess_order(order)
    ops.set_timestep(*ref.opset(opset).triple)
    return ops


def check_route(ops, key, expect_zc=None):
    route = ops.rr_route()
    out[f"{key}|route"] = np.array([route[k] for k in HipOps.RR_ROUTE_KEYS])
    assert route["available"] == 1 and ops.can_open(), (key, route)
    assert {k: route[k] for k in WANT} == WANT, (key, route, WANT)
    assert route["guess_ry"] == 2, (key, route)  # the right-hand side with a guess keeps its own row count
    if expect_zc is not None:
        assert route["zc"] == expect_zc, (key, route)
    return route


def record(key, res, fx):
    out[f"{key}|x"] = fx.numpy()
    out[f"{key}|rec"] = np.array([res.iterations, res.converged_reason, res.residual_norm, res.rhs_norm], dtype=np.float64)


def solves(key, solve, fx, uncut=True):
    for k in ref.CUTS:
        fx.fill(float("nan"))
        record(f"{key}/k={k}", solve(max_it=k, **NO_STOP), fx)
    if uncut:
        for rtol in ref.RTOLS:
            fx.fill(float("nan"))
            record(f"{key}/rtol={rtol:g}", solve(max_it=MAX_IT, rtol=rtol, atol=1e-300), fx)


def stimuli(ops, shape):
    ws = []
    for w in ref.problem(shape).weights:
        f = ops.new_field()
        f.set(w)
        ws.append(f)
    return ws


def run_loops(ctx, shape, key, chunked, expect_zc=None, opset="cn"):
    """Loops (a) - (d) of one shape under the BEAT_RR_BLOCKS now in the environment, each on a fresh operator (the predicted stop's
    error constant, which depends on the chunking, is cached on the operator)."""
    v = ref.field(shape)
    for loop in "abcd":
        ops = make_ops(ctx, shape, predict=loop != "b", opset=opset)
        check_route(ops, f"{key}/{loop}", expect_zc)
        fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, shape)
        fv.set(v)
        if loop in "ab":
            solve = lambda max_it, rtol, atol: ops.solve_single(fv, ws, ref.STIM_AMPS, fx, rtol, atol, max_it)  # noqa: E731
        else:
            solver = DiffusionSolver(ops, Slab(shape[2]), force_distributed=True, libcomm=shared["libcomm"])
            assert solver.libcomm is not None, key
            shared["libcomm"] = solver.libcomm  # one communicator for the process
            if loop == "d":
                ops.set_single_reduction(True)
            solve = lambda max_it, rtol, atol: solver.solve(fv, ws, ref.STIM_AMPS, fx, rtol=rtol, atol=atol, max_it=max_it)  # noqa: E731
        solves(f"{key}/{loop}", solve, fx, uncut=loop != "b" or chunked)
        assert ops.pending is None


def chunk_settings(ctx, shape):
    """BEAT_RR_BLOCKS values (read at every call) for every z-chunk length the pass geometry can take on this shape: the smallest
    value for each, from one chunk (1) to a value far beyond what the slab can use (the shortest chunks)."""
    probe = make_ops(ctx, shape)
    found = {}
    for blocks in list(range(1, 2049)) + [1 << 20]:
        os.environ["BEAT_RR_BLOCKS"] = str(blocks)
        route = probe.rr_route()
        found.setdefault((route["zc"], route["available"]), blocks)
    del os.environ["BEAT_RR_BLOCKS"]
    return sorted((blocks, zc, avail) for (zc, avail), blocks in found.items())


def run_guess(ctx, shape, opset="cn"):
    """(e): four converged solves of a field that moves between solves, then a cut solve that starts from their extrapolation."""
    for order in ref.GUESS_ORDERS:
        ops = make_ops(ctx, shape, order=order, opset=opset)
        key = f"{ref.case_key(shape, opset)}/default/e/order={order}"
        check_route(ops, key)
        fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, shape)
        for k in ref.GUESS_CUTS:
            ops.guess_reset()
            for j in range(1, ref.GUESS_SOLVES + 1):
                fv.set(ref.field(shape, j))
                fx.fill(float("nan"))
                res = ops.solve_single(fv, ws, ref.STIM_AMPS, fx, ref.GUESS_RTOL, 1e-300, MAX_IT)
                assert res.converged_reason > 0, (key, j, res)
                record(f"{key}/k={k}/solve={j}", res, fx)
            fv.set(ref.field(shape, ref.GUESS_SOLVES + 1))
            fx.fill(float("nan"))
            record(f"{key}/k={k}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP), fx)


def cut_sequence(ops, key, fv, fx, ws):
    """The cuts one after another with NO guess_reset between them: the first starts from x0 = v_ only if the history is empty."""
    for k in ref.CUTS:
        fx.fill(float("nan"))
        record(f"{key}/k={k}", ops.solve_single(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP), fx)


def run_retime(ctx, shape):
    """A live handle with a guess of order 3 through ref.RETIME: the cut sequence under cn on the handle as created ("live0"),
    GUESS_SOLVES converged solves of the moving field (the history fills), set_timestep(skew) and the cut sequence ("live1"), back to
    cn and the cut sequence ("live2"); and the cut sequence of a fresh handle created under skew ("fresh")."""
    sk = ref.shape_key(shape)
    ops = make_ops(ctx, shape, order=3, opset=ref.RETIME[0])
    check_route(ops, f"{sk}/retime/live0")
    fv, fx, ws = ops.new_field(), ops.new_field(), stimuli(ops, shape)
    v = ref.field(shape)
    fv.set(v)
    cut_sequence(ops, f"{sk}/retime/live0", fv, fx, ws)
    for stage, name in enumerate(ref.RETIME[1:], start=1):
        for j in range(1, ref.GUESS_SOLVES + 1):
            fv.set(ref.field(shape, j))
            res = ops.solve_single(fv, ws, ref.STIM_AMPS, fx, ref.GUESS_RTOL, 1e-300, MAX_IT)
            assert res.converged_reason > 0, (sk, stage, j, res)
        fv.set(v)
        ops.set_timestep(*ref.opset(name).triple)  # re-forms A, B and 1 / diag and drops the history: no guess_reset here
        check_route(ops, f"{sk}/retime/live{stage}")
        cut_sequence(ops, f"{sk}/retime/live{stage}", fv, fx, ws)
    fresh = make_ops(ctx, shape, order=3, opset=ref.RETIME[1])
    check_route(fresh, f"{sk}/retime/fresh")
    fv2, fx2, ws2 = fresh.new_field(), fresh.new_field(), stimuli(fresh, shape)
    fv2.set(v)
    cut_sequence(fresh, f"{sk}/retime/fresh", fv2, fx2, ws2)


def run_opsets(ctx):
    for shape, sets in ref.OPSET_SHAPES.items():
        for name in sets:
            run_loops(ctx, shape, f"{ref.case_key(shape, name)}/default", False, opset=name)
            if shape in ref.OPSET_GUESS_SHAPES:
                run_guess(ctx, shape, opset=name)
    run_retime(ctx, next(iter(ref.OPSET_SHAPES)))


def main():
    import torch.distributed as dist

    t0 = time.perf_counter()
    ctx = Context(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=ctx.device)
    try:
        os.environ.pop("BEAT_RR_BLOCKS", None)
        for shape in ref.SHAPES:
            sk = ref.shape_key(shape)
            if shape in ref.CHUNK_SHAPES:
                declined = []
                for blocks, zc, avail in chunk_settings(ctx, shape):
                    os.environ["BEAT_RR_BLOCKS"] = str(blocks)
                    if not avail:  # too many block partials: the operator declines the register-row loop, and says so
                        probe = make_ops(ctx, shape)
                        assert probe.rr_route()["available"] == 0 and not probe.can_open(), (sk, blocks)
                        declined.append(blocks)
                        continue
                    run_loops(ctx, shape, f"{sk}/zc={zc}", True, expect_zc=zc)
                del os.environ["BEAT_RR_BLOCKS"]
                out[f"{sk}|declined"] = np.array(declined, dtype=np.int64)
            else:
                run_loops(ctx, shape, f"{sk}/default", False)
            if shape in ref.GUESS_SHAPES:
                run_guess(ctx, shape)
        out["opsets"] = np.array(WANT["pd"] == 1 and WANT["by_rows_mask"] == 0)
        if out["opsets"]:
            t1 = time.perf_counter()
            run_opsets(ctx)
            ctx.synchronize()
            out["opsets_seconds"] = np.array(time.perf_counter() - t1)
        ctx.synchronize()
    finally:
        if shared["libcomm"] is not None:
            shared["libcomm"].close()
        dist.destroy_process_group()
    out["seconds"] = np.array(time.perf_counter() - t0)
    np.savez(sys.argv[1], **out)
    print(f"rr iterates: {sum(k.endswith('|x') for k in out)} solves, {float(out['seconds']):.2f} s, want {WANT}")


if __name__ == "__main__":
    main()
