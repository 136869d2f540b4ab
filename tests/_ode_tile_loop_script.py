"""Every launch form of the ionic step kernel (ode_step_kernel, csrc/beat_ode_kernel.h) on seeded states, written to <out.npz> with
the inputs each case started from and the blocks beat_ode_launch_blocks reports for every (n, num_states) launched.  Run by
tests/test_ode_tile_loop_gpu.py once per launch shape -- BEAT_ODE_GRID / BEAT_ODE_BALANCE are read once per process, so each shape
is a fresh interpreter -- and compared there: bit for bit between the shapes, and the one-block-per-tile run against the oracle.

usage: _ode_tile_loop_script.py <out.npz>

The cases (A - J as the test's docstring lists them) go through beat.odesolver._DeviceODE and HipOps, so the kernel's arguments are
the ones the Python layer passes.  The cases with a pending update (F, G, H, and I's) run twice in this process: with the update
left to the ionic launch, and with it flushed in a pass of its own ahead of a plain step (the twin)."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from beat import _hip, _stencil, telemetry  # noqa: E402
from beat._device import Context  # noqa: E402
from beat._engine import HipOps  # noqa: E402
from beat.models import fhn, from_ode, torord, tp06  # noqa: E402
from beat.odesolver import _DeviceODE  # noqa: E402

CELLS, NN, H = (16, 12, 12), (17, 13, 13), 0.1
N, PLANE = 17 * 13 * 13, 17 * 13  # 2873 = 11 * 256 + 57 nodes: 12 tiles, the last one a partial wave and three waves past n
T0, DT = 1.0, 0.05
M_COND = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.1], [0.0, 0.1, 0.5]]) * 1e-3
# Stopping tolerances of the diffusion solves, chosen so that each solve leaves the number of search directions its case is about
# (asserted per step below: 1..6 for the ring of six, above 6 for the ring of twelve)
RTOL = {"F": 3.16e-9, "G": 3.16e-9, "Igenp": 3.16e-9, "H": 1e-8, "Hm": 1e-8}
SMALL = ROOT / "tests" / "data" / "small_cell.ode"

OUT = {}
BLOCKS = {}


def random_tp06_states(n, seed):
    """Random physiological TP06 states (tests/test_gpu_kernels.py: _random_tp06_states)."""
    rng = np.random.default_rng(seed)
    S = np.repeat(tp06.init_state_values()[:, None], n, axis=1)
    idx = tp06.state_index
    S[idx("V")] = rng.uniform(-95, 50, n)
    for g in ["Xr1", "Xr2", "Xs", "m", "h", "j", "d", "f", "f2", "fCass", "s", "r", "R_prime"]:
        S[idx(g)] = rng.uniform(0, 1, n)
    S[idx("Ca_i")] = 10 ** rng.uniform(-4.2, -2.8, n)
    S[idx("Ca_ss")] = 10 ** rng.uniform(-4, -2, n)
    S[idx("Ca_SR")] = rng.uniform(1, 4.5, n)
    S[idx("Na_i")] = rng.uniform(6, 12, n)
    S[idx("K_i")] = rng.uniform(125, 145, n)
    return S


def random_small_cell_states(model, n, seed):
    """Random states of tests/data/small_cell.ode (tests/test_ode_file_gpu.py: _states)."""
    rng = np.random.default_rng(seed)
    y = np.repeat(model.init_state_values()[:, None], n, axis=1)
    y[model.state_index("V")] = rng.uniform(-95.0, 45.0, n)
    for g in ("m", "h", "n"):
        y[model.state_index(g)] = rng.uniform(0.0, 1.0, n)
    y[model.state_index("ca")] = 10.0 ** rng.uniform(-4.5, -2.5, n)
    return y


def smooth_potential(n=N):
    """A potential the diffusion solve has work with: a depolarised bump on rest, plus noise."""
    i = np.arange(n)
    x, y, z = (i % NN[0]) * H, (i // NN[0] % NN[1]) * H, (i // PLANE) * H
    rng = np.random.default_rng(77)
    return -85.0 + 110.0 * np.exp(-((x - 0.5) ** 2 + (y - 0.6) ** 2 + (z - 0.4) ** 2) / 0.08) + 0.5 * rng.standard_normal(n)


def new_ode(ctx, model, n, plane, parameters):
    ode = _DeviceODE(ctx, model, model.num_states, n, plane, parameters, telemetry.NullMonitor())
    b = int(ctx.lib.beat_ode_launch_blocks(n, model.num_states))
    assert b >= 1, (n, model.num_states, b)
    BLOCKS[(n, model.num_states)] = b
    return ode


def mirror(ctx, ode, vi, n, plane):
    """A v_copy field that holds the potential row as the step finds it."""
    vc = ctx.field(n, plane)
    vc.copy_from(ode.states.row_field(vi))
    return vc


def d_markers(n=N):
    """Three classes with boundaries inside waves (nodes 100, 700), one wave holding all three (1280..1343), a run of 255 -- no
    class -- from 500 to 530 and another across the tile boundary at 1024."""
    m = np.zeros(n, dtype=np.uint8)
    m[100:700] = 1
    m[700:] = 2
    m[1280:1300], m[1300:1320], m[1320:1344] = 0, 1, 2
    m[500:531] = 255
    m[1010:1041] = 255
    return m


def node_active():
    """The voxel mask of the compact cases (cells within 1.15 of the box's ellipsoid) and the nodes its cells touch."""
    cz, cy, cx = np.meshgrid(*(np.arange(c) + 0.5 for c in CELLS[::-1]), indexing="ij")
    act = np.sqrt(((cx - 8) / 8) ** 2 + ((cy - 6) / 6) ** 2 + ((cz - 6) / 6) ** 2) < 1.15
    node = np.zeros(NN[::-1], dtype=bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                node[dz:dz + CELLS[2], dy:dy + CELLS[1], dx:dx + CELLS[0]] |= act
    return act.ravel(), node.ravel()


def compact_layout():
    """What DolfinMultiODESolver._setup_one_launch builds for three markers on the tissue of ``node_active`` (layers in x; the
    tissue beyond y = 10 carries no marker): per class a run of whole 256-entry tiles, nodes ascending, padded with class 254 and
    map entry 0, then the tissue without a model as class 255.  Returns (int32 map, class bytes, entries that are nodes)."""
    _, tissue = node_active()
    i = np.arange(N)
    x, y = i % NN[0], i // NN[0] % NN[1]
    cls_full = np.full(N, 255, dtype=np.uint8)
    cls_full[tissue & (x < 6)] = 0
    cls_full[tissue & (x >= 6) & (x < 11)] = 1
    cls_full[tissue & (x >= 11)] = 2
    cls_full[tissue & (y >= 10)] = 255
    marked = cls_full != 255
    held = marked | tissue
    assert held.mean() < 0.9  # (the layout the solver chooses by itself)
    runs = [(k, np.nonzero(cls_full == k)[0]) for k in range(3)] + [(255, np.nonzero(held & ~marked)[0])]
    node_parts, cls_parts, real = [], [], []
    off = 0
    for k, nodes in runs:
        pad = (-nodes.size) % 256
        node_parts += [nodes, np.zeros(pad, dtype=np.int64)]
        cls_parts += [np.full(nodes.size, k, dtype=np.uint8), np.full(pad, 254, dtype=np.uint8)]
        real.append(off + np.arange(nodes.size))
        off += nodes.size + pad
    node_idx, cls = np.concatenate(node_parts).astype(np.int32), np.concatenate(cls_parts)
    assert node_idx.size == 2816 < N and (cls == 254).sum() > 256
    return node_idx, cls, np.concatenate(real)


def tp06_class_sets():
    P = tp06.init_parameter_values(stim_amplitude=0.0)
    sets = [P.copy() for _ in range(3)]
    sets[1][tp06.parameter_index("g_Ks")] *= 0.25
    sets[2][tp06.parameter_index("g_CaL")] *= 1.4
    sets[2][tp06.parameter_index("g_to")] *= 0.3
    return sets


def guess_fields(ctx, ops, tag):
    d, e, cnt = C.c_void_p(), C.c_void_p(), C.c_int()
    _hip.check(ops.lib.beat_pde_guess_history(ops.handle, C.byref(d), C.byref(e), C.byref(cnt)))
    OUT[tag + "_guess_count"] = np.array([cnt.value])
    for name, p in (("d", d), ("e", e)):
        if p.value:
            host = np.empty(ops.n)
            _hip.check(ctx.lib.beat_memcpy_d2h(ctx.handle, host.ctypes.data_as(C.c_void_p), p, 8 * ops.n))
            OUT[f"{tag}_guess_{name}"] = host


# ---- A, B, C: the plain step on uniform parameters, all rows, sparse rows ---------------------------------------------------------
def case_a(ctx):
    vi = tp06.state_index("V")
    P = tp06.init_parameter_values(stim_amplitude=0.0)
    for n in (N, 2048, 2049, 63):
        plane = PLANE if n == N else 0
        ode = new_ode(ctx, tp06.generalized_rush_larsen, n, plane, P)
        if n == N:
            assert ode.states.ld == 3328 and ode.states.base == PLANE  # stride and offset differ from n and 0
        S0 = random_tp06_states(n, 11)
        ode.set_initial(S0)
        vc = mirror(ctx, ode, vi, n, plane)
        OUT[f"A{n}_s0"] = S0
        for k in (1, 2):
            ode.step(T0 + (k - 1) * DT, DT, v_index=vi, v_copy=vc)
            ctx.synchronize()
            OUT[f"A{n}_s{k}"], OUT[f"A{n}_vc{k}"] = ode.states.numpy(), vc.numpy()
        assert ode.routes.current.kind == "uniform"


def per_node_parameters(rows, seed):
    rng = np.random.default_rng(seed)
    P = np.repeat(tp06.init_parameter_values(stim_amplitude=0.0)[:, None], N, axis=1)
    for name in rows:
        P[tp06.parameter_index(name)] *= rng.uniform(0.5, 1.5, N)
    return P


def rows_step(ctx, tag, P, sparse, jit):
    """One step on the per-node parameters P: all 53 rows (sparse = "0"), or the varying rows alone on the run-time-index kernel
    (jit = "0") or the instance compiled for their indices ("1").  Both switches are read per call."""
    vi = tp06.state_index("V")
    os.environ["BEAT_PARAM_SPARSE"], os.environ["BEAT_JIT"] = sparse, jit
    try:
        ode = new_ode(ctx, tp06.generalized_rush_larsen, N, PLANE, P)
        ode.set_initial(random_tp06_states(N, 12))
        vc = mirror(ctx, ode, vi, N, PLANE)
        stats0 = (C.c_longlong * 4)()
        usable = ctx.lib.beat_ode_jit_stats(stats0)
        ode.step(T0, DT, v_index=vi, v_copy=vc)
        ctx.synchronize()
        stats1 = (C.c_longlong * 4)()
        ctx.lib.beat_ode_jit_stats(stats1)
        kind = ode.routes.current.kind
        assert kind == ("per_node" if sparse == "0" else "rows"), kind
        if sparse == "1" and jit == "1":  # the compiled instance did run: loaded now or earlier in this process, and no failure
            assert usable == 1 and stats1[3] == 0 and stats1[0] >= 1, list(stats1)
        if jit == "0":
            assert list(stats0) == list(stats1)
        OUT[tag + "_s1"], OUT[tag + "_vc1"] = ode.states.numpy(), vc.numpy()
    finally:
        del os.environ["BEAT_PARAM_SPARSE"], os.environ["BEAT_JIT"]


def case_b_c(ctx):
    OUT["BC_s0"] = random_tp06_states(N, 12)
    P = per_node_parameters(["g_Kr", "g_CaL"], 21)
    OUT["B_P"] = P
    rows_step(ctx, "B", P, "0", "1")
    for count, names in ((1, ["g_CaL"]), (4, ["g_Na", "g_CaL", "g_to", "g_Ks"])):
        P = per_node_parameters(names, 30 + count)
        OUT[f"C{count}_P"] = P
        rows_step(ctx, f"C{count}_all", P, "0", "1")
        rows_step(ctx, f"C{count}_rt", P, "1", "0")
        rows_step(ctx, f"C{count}_jit", P, "1", "1")


# ---- D, E: parameter classes, on the grid's nodes and in the compact layout -------------------------------------------------------
def class_ode(ctx, model, sets, markers, n, plane):
    ode = new_ode(ctx, model, n, plane, None)
    ode.set_classes(ctx.from_numpy(markers), sets)
    return ode


def case_d(ctx):
    vi = tp06.state_index("V")
    markers = d_markers()
    ode = class_ode(ctx, tp06.generalized_rush_larsen, tp06_class_sets(), markers, N, PLANE)
    S0 = random_tp06_states(N, 13)
    ode.set_initial(S0)
    vc = mirror(ctx, ode, vi, N, PLANE)
    ode.step(T0, DT, v_index=vi, v_copy=vc)
    ctx.synchronize()
    OUT["D_s0"], OUT["D_markers"], OUT["D_sets"] = S0, markers, np.stack(tp06_class_sets())
    OUT["D_s1"], OUT["D_vc1"] = ode.states.numpy(), vc.numpy()


def compact_ode(ctx, model, sets, S_real, v_field_values):
    """The compact state array as _setup_one_launch leaves it: the real entries hold ``S_real`` (the potential row of the marked
    ones is their field value), the entries of tissue without a model hold zeros, and -- for this test -- the padding entries NaN."""
    node_idx, cls, real = compact_layout()
    n_c = node_idx.size
    ode = class_ode(ctx, model, sets, cls, n_c, 0)
    home = ctx.field(N, PLANE)
    home.set(v_field_values)
    S = np.zeros((model.num_states, n_c))
    marked = real[cls[real] != 255]
    S[:, marked] = S_real[:, : marked.size]
    S[model.state_index(model.v_name), marked] = v_field_values[node_idx[marked]]
    S[:, cls == 254] = np.nan
    ode.set_initial(S)
    ode.node_map = (ctx.from_numpy(node_idx), home)
    return ode, home, S, node_idx, cls


def case_e(ctx):
    vi = tp06.state_index("V")
    v0 = np.random.default_rng(14).uniform(-95, 50, N)
    ode, home, S, node_idx, cls = compact_ode(ctx, tp06.generalized_rush_larsen, tp06_class_sets(), random_tp06_states(2816, 15), v0)
    ode.step(T0, DT, v_index=vi)
    ctx.synchronize()
    OUT["E_s0"], OUT["E_field0"], OUT["E_map"], OUT["E_cls"], OUT["E_sets"] = S, v0, node_idx, cls, np.stack(tp06_class_sets())
    OUT["E_s1"], OUT["E_field1"] = ode.states.numpy(), home.numpy()


# ---- F, G, H: the pending update ---------------------------------------------------------------------------------------------------
def table_operator(ctx, order):
    ops = HipOps(ctx, NN, True, True, *_stencil.stencil_tables(3, (H,) * 3, M_COND))
    ops.set_small(False)
    ops.set_guess_order(order)
    ops.set_timestep(0.01, 1.0, DT)
    assert not ops.small_active() and len(ops.ring) == 6
    return ops


def rows_operator(ctx):
    """Per-node rows on the voxel mask of the compact cases: the ring of twelve search directions."""
    act, _ = node_active()
    ops = HipOps(ctx, NN, True, True, *_stencil.stencil_fields(3, CELLS, (H,) * 3, M_COND, act), per_node=True)
    ops.set_small(False)
    ops.set_timestep(0.01, 1.0, DT)
    assert not ops.small_active() and len(ops.ring) == 12
    return ops


def pending_steps(ctx, tag, ops, ode, row, vc, steps, mode, rtol, count_range, twin):
    """``steps`` split steps, the diffusion solve first: in place on ``row`` with its last update deferred (mode "host": the host
    knows the count; "open": the solve is left open and the ionic launch goes behind it), then the ionic step that applies it.
    ``twin``: the update is flushed in a pass of its own and a plain step follows.  Stores the states before and after each ionic
    step of the twin (what the oracle is asked about), and after each step of both."""
    vi = ode.model.state_index(ode.model.v_name)
    ops.ksp_log = []
    counts = []
    for s in range(steps):
        if mode == "open":
            assert ops.can_open()
            ops.solve_begin(row, [], [], row, rtol, 1e-50, 500)
            assert ops.open_x is not None
        else:
            res = ops.solve_single(row, [], [], row, rtol, 1e-50, 500, defer_flush=True)
            assert res.converged_reason > 0, res
            assert ops.pending is not None, (tag, s, res)
            counts.append(ops.pending[2])
            assert count_range[0] <= ops.pending[2] <= count_range[1], (tag, s, ops.pending[2], res)
        t = T0 + s * DT
        if twin:
            ops.flush_pending()
            ctx.synchronize()
            OUT[f"{tag}_twin_pre{s}"] = ode.states.numpy()
            if ode.node_map is not None:
                OUT[f"{tag}_twin_prefield{s}"] = row.numpy()
            ode.step(t, DT, v_index=vi, v_copy=vc)
        else:
            flushes = ops.flushes
            ode.step(t, DT, v_index=vi, v_copy=vc, pending_ops=ops, v_row=row)
            assert ops.flushes == flushes and ops.pending is None and ops.open_x is None  # the launch took the update
        ctx.synchronize()
        kind = "twin" if twin else "pend"
        OUT[f"{tag}_{kind}_s{s}"] = ode.states.numpy()
        OUT[f"{tag}_{kind}_row{s}"] = row.numpy()
        if vc is not None:
            OUT[f"{tag}_{kind}_vc{s}"] = vc.numpy()
    kind = "twin" if twin else "pend"
    OUT[f"{tag}_{kind}_iters"] = np.array([r.iterations for r in ops.ksp_log])
    assert len(ops.ksp_log) == steps
    guess_fields(ctx, ops, f"{tag}_{kind}")
    if counts:
        print(tag, kind, "pending counts", counts, "iterations", [r.iterations for r in ops.ksp_log], flush=True)


def tp06_grid_ode(ctx, S0):
    ode = new_ode(ctx, tp06.generalized_rush_larsen, N, PLANE, tp06.init_parameter_values(stim_amplitude=0.0))
    ode.set_initial(S0)
    return ode


def case_f_g(ctx):
    vi = tp06.state_index("V")
    S0 = random_tp06_states(N, 16)
    S0[vi] = smooth_potential()
    OUT["FG_s0"] = S0
    for tag, mode, steps in (("F", "host", 4), ("G", "open", 3)):
        for twin in (False, True):
            ops = table_operator(ctx, 2)
            ode = tp06_grid_ode(ctx, S0)
            pending_steps(ctx, tag, ops, ode, ode.states.row_field(vi), mirror(ctx, ode, vi, N, PLANE), steps, mode, RTOL[tag], (1, 6), twin)


def case_h(ctx):
    vi = tp06.state_index("V")
    S0 = random_tp06_states(N, 17)
    S0[vi] = smooth_potential()
    OUT["H_s0"], OUT["H_markers"], OUT["H_sets"] = S0, d_markers(), np.stack(tp06_class_sets())
    for twin in (False, True):
        ops = rows_operator(ctx)
        ode = class_ode(ctx, tp06.generalized_rush_larsen, tp06_class_sets(), d_markers(), N, PLANE)
        ode.set_initial(S0)
        pending_steps(ctx, "H", ops, ode, ode.states.row_field(vi), None, 2, "host", RTOL["H"], (7, 12), twin)
    # ... and in the compact layout: the solve works on the field the node map points into
    for twin in (False, True):
        ops = rows_operator(ctx)
        ode, home, S, node_idx, cls = compact_ode(ctx, tp06.generalized_rush_larsen, tp06_class_sets(), random_tp06_states(2816, 18), smooth_potential())
        OUT["Hm_s0"], OUT["Hm_map"], OUT["Hm_cls"] = S, node_idx, cls
        pending_steps(ctx, "Hm", ops, ode, home, None, 2, "host", RTOL["Hm"], (7, 12), twin)


# ---- I, J: the small models, which loop by default at size, and the register-tight ToR-ORd instances -------------------------------
def case_i(ctx):
    model = fhn.forward_euler_readme
    st = np.stack([np.random.default_rng(1).uniform(-0.5, 2, N), np.random.default_rng(2).uniform(-90, 45, N)])
    P = np.array([0.26, 0.1, 1.0, 0.13, 0.013, 125.0, -85.0, 40.0, 100.0, 1.0, 0.0])
    ode = new_ode(ctx, model, N, PLANE, P)
    ode.set_initial(st)
    vc = mirror(ctx, ode, 1, N, PLANE)
    ode.step(0.5, 0.01, v_index=1, v_copy=vc)
    ctx.synchronize()
    OUT["Ifhn_s0"], OUT["Ifhn_P"], OUT["Ifhn_s1"], OUT["Ifhn_vc1"] = st, P, ode.states.numpy(), vc.numpy()

    gen = from_ode(SMALL)
    vi = gen.state_index("V")
    y0 = random_small_cell_states(gen, N, 5)
    p_uni = gen.init_parameter_values(stim_amplitude=30.0)
    rng = np.random.default_rng(3)
    p_rows = np.repeat(p_uni[:, None], N, axis=1)
    p_rows[gen.parameter_index("g_in")] *= rng.uniform(0.5, 1.5, N)
    p_rows[gen.parameter_index("g_out")] *= rng.uniform(0.5, 1.5, N)
    p_cls = np.repeat(p_uni[:, None], N, axis=1)  # three parameter sets, boundaries inside waves
    p_cls[gen.parameter_index("g_in"), 1000:] *= 0.5
    p_cls[gen.parameter_index("g_out"), 1900:] = 0.0
    OUT["Igen_s0"] = y0
    for tag, p, kind in (("uni", p_uni, "uniform"), ("rows", p_rows, "per_node"), ("cls", p_cls, "classes")):
        ode = new_ode(ctx, gen, N, PLANE, p)
        ode.set_initial(y0)
        vc = mirror(ctx, ode, vi, N, PLANE)
        ode.step(0.3, 0.02, v_index=vi, v_copy=vc)
        ctx.synchronize()
        assert ode.routes.current.kind == kind and (kind != "classes" or ode.classes[2] == 3)
        OUT[f"Igen_{tag}_P"], OUT[f"Igen_{tag}_s1"], OUT[f"Igen_{tag}_vc1"] = p, ode.states.numpy(), vc.numpy()
    y0 = y0.copy()
    y0[vi] = smooth_potential()
    OUT["Igenp_s0"], OUT["Igenp_P"] = y0, p_uni
    for twin in (False, True):
        ops = table_operator(ctx, 2)
        ode = new_ode(ctx, gen, N, PLANE, p_uni)
        ode.set_initial(y0)
        pending_steps(ctx, "Igenp", ops, ode, ode.states.row_field(vi), mirror(ctx, ode, vi, N, PLANE), 4, "host", RTOL["Igenp"], (1, 6), twin)


def case_j(ctx):
    model = torord.generalized_rush_larsen
    vi = model.state_index(model.v_name)
    rng = np.random.default_rng(19)
    S0 = np.repeat(model.init_state_values()[:, None], N, axis=1) * (1.0 + 0.01 * rng.uniform(-1, 1, (model.num_states, N)))
    S0[vi] = rng.uniform(-90, 40, N)
    P = model.init_parameter_values()
    sets = [P.copy() for _ in range(3)]
    sets[1][model.parameter_index("GKr_b")] *= 0.5
    sets[2][model.parameter_index("GKs_b")] *= 1.5
    for tag, make in (("uni", lambda: new_ode(ctx, model, N, PLANE, P)), ("cls", lambda: class_ode(ctx, model, sets, d_markers(), N, PLANE))):
        ode = make()
        ode.set_initial(S0)
        vc = mirror(ctx, ode, vi, N, PLANE)
        ode.step(T0, 0.01, v_index=vi, v_copy=vc)
        ctx.synchronize()
        out = ode.states.numpy()
        assert np.isfinite(out).all() and np.abs(out - S0).max() > 0.0
        OUT[f"J_{tag}_s1"], OUT[f"J_{tag}_vc1"] = out, vc.numpy()
    OUT["J_s0"], OUT["J_markers"] = S0, d_markers()


def main(path):
    import time

    ctx = Context(0)
    for case in (case_a, case_b_c, case_d, case_e, case_f_g, case_h, case_i, case_j):
        t0 = time.perf_counter()
        case(ctx)
        ctx.synchronize()
        print(f"{case.__name__}: {time.perf_counter() - t0:.2f} s", flush=True)
    OUT["blocks"] = np.array([(n, ns, b) for (n, ns), b in sorted(BLOCKS.items())], dtype=np.int64)
    print("blocks", OUT["blocks"].tolist(), flush=True)
    np.savez(path, **OUT)


if __name__ == "__main__":
    main(sys.argv[1])
