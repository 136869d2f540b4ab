"""The decomposition cases of tests/_pcg_ref.py and tests/_var_ref.py (DIST_CASES) on the device, in a process of its own: the in-library
decomposed solve (beat_pde_solve_dist over the callback transport) on 2 to 8 ranks played by threads (tests/_thread_world.py), every
slab with its live ghost planes.  tests/test_dist_iterates_gpu.py starts one interpreter per child, the register-row switches
(BEAT_RR_RY, BEAT_RR_PD: read once per process) in the environment:

    python _dist_iterates_script.py out.npz rr2 | rr4 | varF | varQ | varS

Switches that are read per operator or per solve (BEAT_RR, BEAT_VTL, BEAT_VTL_PDOT) are set here, between two thread worlds, never
while ranks run.  Writes, per case key, the ASSEMBLED x (the ranks' slabs concatenated; per-node rows: on the tissue nodes), rank 0's
record, all ranks' records, what every rank's library says it ran (beat_pde_rr_route, beat_pde_tile_route, beat_pde_fused_dist_pass,
beat_comm_merged_solves) and, behind the cuts at 2 and 7, each rank's last search direction with its ghost planes.  Computes no
reference and asserts no route: the parent does both.  A rank that raises aborts the barrier, so the others leave too; a rank that
does not come back within JOIN seconds ends the process (status 3)."""
import os
import sys
import threading
import time
import traceback
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import _pcg_ref as ref  # noqa: E402
import _var_ref as vr  # noqa: E402
from _thread_world import _ThreadWorld  # noqa: E402
from beat._device import Context  # noqa: E402
from beat._engine import DiffusionSolver, HipOps, LibComm, Slab  # noqa: E402

NO_STOP = dict(rtol=1e-30, atol=1e-300)  # nothing but max_it ends a cut solve
MAX_IT = 500
WAIT, JOIN = 20, 45          # seconds: a rank for another rank; the main thread for a world
DEFER_CUTS, GHOST_CUTS = (3, 7), (2, 7)
CONST_LOOPS = {"R": {}, "M": {}, "T": {"BEAT_RR": "0"}}  # (M: ops.set_single_reduction(True))
VAR_ROUTES = {"F": {}, "Q": {"BEAT_VTL_PDOT": "0"}, "S": {"BEAT_VTL": "0"}}
out: dict = {}
slips: list = []
contexts: dict = {}


def run_world(world, work):
    """work(rank, ctx, dist_view) on `world` threads; the list of what they returned."""
    tw = _ThreadWorld(world, timeout=WAIT)
    results, errors = [None] * world, []

    def run(rank):
        try:
            if rank not in contexts:
                contexts[rank] = Context(0)
            results[rank] = work(rank, contexts[rank], tw.rank_view(rank))
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, repr(exc), traceback.format_exc()))
            tw.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN
    for t in threads:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        print(f"a rank of {world} did not come back within {JOIN} s; errors so far: {errors}", file=sys.stderr, flush=True)
        os._exit(3)
    if errors:
        raise RuntimeError("\n".join(f"rank {r}: {e}\n{tb}" for r, e, tb in errors))
    return results


def rec_of(res):
    return np.array([res.iterations, res.converged_reason, res.residual_norm, res.rhs_norm], dtype=np.float64)


def fields_of(ops, arrays):
    fs = []
    for a in arrays:
        f = ops.new_field()
        f.set(a)
        fs.append(f)
    return fs


def report(ops, comm):
    return {"rr_route": np.array([ops.rr_route()[k] for k in HipOps.RR_ROUTE_KEYS]),
            "tile": np.array([int(ops.lib.beat_pde_tile_route(ops.handle)), int(ops.lib.beat_pde_fused_dist_pass(ops.handle))]),
            "merged": np.array([int(ops.lib.beat_comm_merged_solves(comm.handle))])}


def plain_solves(ops, solver, ctx, sl, v, weights, cuts, res):
    """The cut, uncut and deferred solves of one rank; res[tail] = (x of the slab, record), res[tail + "|p"] = a direction."""
    ring = int(ops.lib.beat_pde_ring_size())
    fv, fx = ops.new_field(), ops.new_field()
    ws = fields_of(ops, [w[sl] for w in weights])
    fv.set(v[sl])

    def solve(tail, defer=False, **kw):
        fx.fill(float("nan"))
        r = solver.solve(fv, ws, ref.STIM_AMPS, fx, defer_flush=defer, **kw)
        if defer:
            ops.flush_pending()
        ctx.synchronize()
        res[tail] = (fx.numpy().copy(), rec_of(r))

    for k in cuts:
        solve(f"k={k}", max_it=k, **NO_STOP)
        if k in GHOST_CUTS:  # the direction formed last, p_{k-1}, with the ghost planes this rank keeps of it
            f = ops.ring[(k - 1) % ring]
            res[f"k={k}|p"] = np.concatenate([f.ghost_lo.cpu().numpy(), f.numpy(), f.ghost_hi.cpu().numpy()])
    for rtol in ref.RTOLS:
        solve(f"rtol={rtol:g}", max_it=MAX_IT, rtol=rtol, atol=1e-300)
    for k in DEFER_CUTS:
        if k in cuts:
            solve(f"defer/k={k}", defer=True, max_it=k, **NO_STOP)
    res["|nsolves"] = len(cuts) + len(ref.RTOLS) + sum(k in cuts for k in DEFER_CUTS)
    res["|v_same"] = bool(np.array_equal(fv.numpy(), v[sl])) and ops.pending is None


def guess_solves(make, ctx, sl, fields, weights, res):
    """Four converged solves of a field that moves between solves, then a cut solve that starts from their extrapolation, whose
    increment's ghost planes travel with those of v_."""
    for order in ref.GUESS_ORDERS:
        ops, solver = make(order)
        fv, fx = ops.new_field(), ops.new_field()
        ws = fields_of(ops, [w[sl] for w in weights])
        for k in ref.GUESS_CUTS:
            ops.guess_reset()
            for j in range(1, ref.GUESS_SOLVES + 2):
                fv.set(fields[j][sl])
                fx.fill(float("nan"))
                last = j == ref.GUESS_SOLVES + 1
                kw = dict(max_it=k, **NO_STOP) if last else dict(max_it=MAX_IT, rtol=ref.GUESS_RTOL, atol=1e-300)
                r = solver.solve(fv, ws, ref.STIM_AMPS, fx, **kw)
                ctx.synchronize()
                res[f"e/order={order}/k={k}" + ("" if last else f"/solve={j}")] = (fx.numpy().copy(), rec_of(r))
        res[f"e/order={order}|tile"] = report(ops, solver.libcomm)["tile"]


def retime_solves(make, ctx, sl, fields, weights, cuts, res):
    """A live handle with a guess of order 3 through ref.RETIME on every rank: the cut sequence (NO guess_reset between the cuts) under
    cn on the handle as created ("live0"), GUESS_SOLVES converged solves of the moving field, set_timestep(skew) and the cut sequence
    ("live1"), back to cn ("live2"); and the cut sequence of a fresh handle created under skew ("fresh").  set_timestep is a call of
    each rank on its own handle, between two collective solves."""
    def sequence(ops, solver, tag):
        fv, fx = ops.new_field(), ops.new_field()
        ws = fields_of(ops, [w[sl] for w in weights])
        fv.set(fields[0][sl])
        for k in cuts:
            fx.fill(float("nan"))
            r = solver.solve(fv, ws, ref.STIM_AMPS, fx, max_it=k, **NO_STOP)
            ctx.synchronize()
            res[f"retime/{tag}/k={k}"] = (fx.numpy().copy(), rec_of(r))
        said = report(ops, solver.libcomm)
        res[f"retime/{tag}|tile"], res[f"retime/{tag}|rr"] = said["tile"], said["rr_route"]
        return fv, fx, ws

    ops, solver = make(3, ref.RETIME[0])
    fv, fx, ws = sequence(ops, solver, "live0")
    for stage, name in enumerate(ref.RETIME[1:], start=1):
        for j in range(1, ref.GUESS_SOLVES + 1):
            fv.set(fields[j][sl])
            r = solver.solve(fv, ws, ref.STIM_AMPS, fx, max_it=MAX_IT, rtol=ref.GUESS_RTOL, atol=1e-300)
            assert r.converged_reason > 0, (stage, j, r)
        ops.set_timestep(*ref.opset(name).triple)  # drops the history: no guess_reset here
        sequence(ops, solver, f"live{stage}")
    sequence(*make(3, ref.RETIME[1]), "fresh")


def gather(base, results, keep=None):
    """The ranks' results under the keys of the parent: x assembled (on the nodes of `keep`), records, reports, directions."""
    for tail in results[0]:
        vals = [r[tail] for r in results]
        if tail == "|v_same":
            if not all(vals):
                slips.append(f"{base}: a solve changed v on rank {vals.index(False)}, or left an update pending")
        elif tail.startswith("|"):
            out[base + tail] = np.array(vals)
        elif tail.endswith("|tile") or tail.endswith("|rr"):
            out[f"{base}/{tail}"] = np.array(vals)
        elif tail.endswith("|p"):
            for rank, p in enumerate(vals):
                out[f"{base}/{tail}{rank}"] = p
        else:
            x = np.concatenate([v[0] for v in vals])
            out[f"{base}/{tail}|x"] = x if keep is None else x[keep]
            out[f"{base}/{tail}|recs"] = np.stack([v[1] for v in vals])
            out[f"{base}/{tail}|rec"] = vals[0][1]
            if keep is not None:
                out[f"{base}/{tail}|off"] = x[~keep]  # what the nodes off the tissue hold


def set_switches(switches):
    for name in ("BEAT_RR", "BEAT_VTL", "BEAT_VTL_PDOT"):
        os.environ.pop(name, None)
    os.environ.update(switches)


def run_const(shape, world, loop, guess, opset="cn", plain=True, retime=False):
    nx, ny, nz = shape
    plane = nx * ny
    mt, kt = ref.tables(3)
    weights = ref.problem(shape).weights
    fields = [ref.field(shape, j) for j in range(ref.GUESS_SOLVES + 2)] if guess or retime else [ref.field(shape)]

    def work(rank, ctx, view):
        slab = Slab(nz, rank, world)
        sl = slice(slab.z0 * plane, slab.z1 * plane)
        comm = LibComm(ctx, slab, view, None, "callbacks")

        def make(order, name=opset):
            ops = HipOps(ctx, (nx, ny, slab.nz), slab.lo_phys, slab.hi_phys, mt, kt)
            ops.set_small(False)
            ops.set_guess_order(order)
            ops.set_timestep(*ref.opset(name).triple)
            if loop == "M":
                ops.set_single_reduction(True)
            return ops, DiffusionSolver(ops, slab, force_distributed=True, libcomm=comm)

        res = {}
        try:
            if plain:
                ops, solver = make(0)
                plain_solves(ops, solver, ctx, sl, fields[0], weights, ref.CUTS, res)
                for name, value in report(ops, comm).items():
                    res[f"|{name}"] = value
            if guess:
                guess_solves(make, ctx, sl, fields, weights, res)
            if retime:
                retime_solves(make, ctx, sl, fields, weights, ref.CUTS, res)
        finally:
            comm.close()
        return res

    set_switches(CONST_LOOPS[loop])
    gather(f"{ref.case_key(shape, opset)}/w{world}/{loop}", run_world(world, work))


def run_var(case, world, route, guess, opset="cn", plain=True, retime=False):
    cs = vr.case(case)
    nx, ny, nz = cs.shape
    plane = nx * ny
    weights = vr.weights_on_box(cs)
    fields = [vr.on_box(cs, vr.field(cs, j)) for j in range(ref.GUESS_SOLVES + 2 if guess or retime else 1)]
    cuts = vr.cuts_of(cs, vr.CUTS_SHORT)

    def work(rank, ctx, view):
        slab = Slab(nz, rank, world)
        sl = slice(slab.z0 * plane, slab.z1 * plane)
        # the slab's columns of the very rows the host reference expands
        mrows, krows = np.ascontiguousarray(cs.mass_rows[:, sl]), np.ascontiguousarray(cs.stiff_rows[:, sl])
        comm = LibComm(ctx, slab, view, None, "callbacks")

        def make(order, name=opset):
            ops = HipOps(ctx, (nx, ny, slab.nz), slab.lo_phys, slab.hi_phys, mrows, krows, per_node=True)
            ops.set_guess_order(order)
            ops.set_timestep(*ref.opset(name).triple)
            return ops, DiffusionSolver(ops, slab, force_distributed=True, libcomm=comm)

        res = {}
        try:
            if plain:
                ops, solver = make(0)
                plain_solves(ops, solver, ctx, sl, fields[0], weights, cuts, res)
                for name, value in report(ops, comm).items():
                    res[f"|{name}"] = value
            if guess:
                guess_solves(make, ctx, sl, fields, weights, res)
            if retime:
                retime_solves(make, ctx, sl, fields, weights, cuts, res)
        finally:
            comm.close()
        return res

    set_switches(VAR_ROUTES[route])
    base = f"{vr.opset_key(case, opset)}/w{world}/{route}"
    gather(base, run_world(world, work), keep=cs.tissue)
    # off the tissue every node holds exactly its v: 1000 + node index (for the guess sequences too: the marks do not move)
    marks = vr.off_tissue_marks(cs)
    for key in [k for k in out if k.startswith(base + "/") and k.endswith("|off")]:
        got = out.pop(key)
        if not np.array_equal(got, marks):
            bad = np.nonzero(got != marks)[0]
            slips.append(f"{key[:-4]}: {len(bad)} nodes off the tissue do not hold their v, the first: mark {marks[bad[0]]!r} holds {got[bad[0]]!r}")


def main():
    t0 = time.perf_counter()
    child = sys.argv[2]
    if child in ("rr2", "rr4"):
        assert os.environ["BEAT_RR_RY"] == child[2:] and os.environ["BEAT_RR_PD"] == "1"
        for shape, worlds in ref.DIST_CASES.items():
            if child == "rr4" and shape[1] < ref.DIST_RY4_MIN_NY:
                continue
            for world in worlds:
                for loop in ("R", "M", "T") if child == "rr2" else ("R", "M"):
                    run_const(shape, world, loop, guess=loop in "RM" and (shape, world) in ref.DIST_GUESS_CASES)
        t1 = time.perf_counter()
        if child == "rr2":  # off theta = 1/2 (keys shape@set), and the re-timing of live handles on loop R
            for (shape, world), sets in ref.DIST_OPSET_CASES.items():
                for name in sets:
                    for loop in ("R", "M", "T"):
                        run_const(shape, world, loop, guess=loop in "RM" and name in ref.DIST_OPSET_GUESS.get((shape, world), ()), opset=name)
            shape, world = next(iter(ref.DIST_OPSET_CASES))
            run_const(shape, world, "R", guess=False, opset="cn", plain=False, retime=True)
        out["opsets_seconds"] = np.array(time.perf_counter() - t1)
    else:
        assert child[:3] == "var" and child[3:] in VAR_ROUTES  # one route per child: each stays at a few seconds
        route = child[3:]
        for case, worlds in vr.DIST_CASES:
            for world in worlds:
                run_var(case, world, route, guess=route in "FS" and (case, world) in vr.DIST_GUESS_CASES)
        t1 = time.perf_counter()
        for (case, world), sets in vr.DIST_OPSET_CASES.items():  # off theta = 1/2 (keys case@set)
            for name in sets:
                run_var(case, world, route, guess=False, opset=name)
        for (case, world), sets in vr.DIST_OPSET_GUESS.items():
            for name in sets:
                if route in "FS":
                    run_var(case, world, route, guess=True, opset=name, plain=False)
        case, world = next(iter(vr.DIST_OPSET_CASES))
        run_var(case, world, route, guess=False, opset="cn", plain=False, retime=True)  # re-forms v_gc0 on route F
        out["opsets_seconds"] = np.array(time.perf_counter() - t1)
    set_switches({})
    for ctx in contexts.values():
        ctx.synchronize()
    out["seconds"] = np.array(time.perf_counter() - t0)
    out["slips"] = np.array(slips, dtype=str)
    np.savez(sys.argv[1], **out)
    print(f"dist iterates {child}: {sum(k.endswith('|x') for k in out)} solves, {float(out['seconds']):.2f} s")


if __name__ == "__main__":
    main()
