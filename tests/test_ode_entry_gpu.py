"""The host-side argument contract of the ionic step's entry points: every case here is rejected on the host, before any
launch, with the library's own message.  beat_ode_step_pending, beat_ode_step_rows and beat_ode_step_classes share the
pending-update protocol (a deferred solve's search directions or guess increment, applied by the next ionic launch; pending = -1:
behind a solve that is still open); the built-in model switch rejects an id that is neither built in nor registered as source."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NN = (8, 8, 8)
UNUSED_MODEL_ID = 50  # below BEAT_MODEL_CUSTOM_BASE (100), no built-in model


@pytest.fixture(scope="module")
def env(hip_ctx):
    import torch

    from beat import _hip, _stencil
    from beat._device import StateArray
    from beat._engine import HipOps
    from beat.models import tp06

    ctx = hip_ctx
    cells = tuple(k - 1 for k in NN)
    n, plane = int(np.prod(NN)), NN[0] * NN[1]
    vi = tp06.state_index("V")
    states = StateArray(ctx, 19, n, plane)
    states.set(np.repeat(tp06.init_state_values()[:, None], n, axis=1))
    P = np.ascontiguousarray(tp06.init_parameter_values(stim_amplitude=0.0), dtype=np.float64)
    M = np.diag([1e-3, 1e-3, 1e-3])
    # an operator with the plain ring of 6 and no open solve
    ops = HipOps(ctx, NN, True, True, *_stencil.stencil_tables(3, tuple(0.1 for _ in cells), M))
    ops.set_timestep(0.01, 0.5, 0.01)
    # a per-node-row operator on a single slab: the ring of 12; its solve is left open (beat_pde_solve_begin)
    var = HipOps(ctx, NN, True, True, *_stencil.stencil_fields(3, cells, (0.1,) * 3, M), per_node=True)
    var.set_timestep(0.01, 0.5, 0.01)
    var.set_small(False)
    assert len(ops.ring) == _hip.load().beat_pde_ring_size() == 6 and len(var.ring) == 12
    assert var.can_open()
    fv, fx = var.new_field(), var.new_field()
    fv.fill(-85.0)
    fx.fill(-85.0)
    var.solve_begin(fv, [], [], fx, 1e-8, 1e-50, 50)
    assert ctx.lib.beat_pde_solve_is_open(var.handle) == 1

    rc = C.c_int(0)
    _hip.check(ctx.lib.beat_ode_class_table_doubles(_hip.MODEL_TP06_GRL1, C.byref(rc)))
    table = ctx.zeros(rc.value)
    markers = torch.zeros(n, dtype=torch.uint8, device=ctx.device)
    row_idx = np.array([0], dtype=np.int32)
    rows = ctx.zeros(n)
    e = dict(ctx=ctx, n=n, vi=vi, states=states, P=P, ops=ops, var=var, table=table, markers=markers, row_idx=row_idx, rows=rows)
    yield e
    var.solve_finish()
    ctx.synchronize()


def _pending(e, pde, ring, fld, pending):
    from beat import _hip

    s = e["states"]
    return e["ctx"].lib.beat_ode_step_pending(
        e["ctx"].handle, _hip.MODEL_TP06_GRL1, s.ptr, e["n"], s.ld, e["P"].ctypes.data_as(C.c_void_p), len(e["P"]), None, 0, 0.0, 0.01,
        e["vi"], None, pde, ring, fld, pending)


def _rows(e, pde, ring, fld, pending):
    from beat import _hip

    s = e["states"]
    return e["ctx"].lib.beat_ode_step_rows(
        e["ctx"].handle, _hip.MODEL_TP06_GRL1, s.ptr, e["n"], s.ld, e["P"].ctypes.data_as(C.c_void_p), len(e["P"]),
        e["row_idx"].ctypes.data_as(C.c_void_p), 1, C.c_void_p(e["rows"].data_ptr()), e["n"], 0.0, 0.01, e["vi"], None,
        pde, ring, fld, pending)


def _classes(e, pde, ring, fld, pending):
    from beat import _hip

    s = e["states"]
    return e["ctx"].lib.beat_ode_step_classes(
        e["ctx"].handle, _hip.MODEL_TP06_GRL1, s.ptr, e["n"], s.ld, C.c_void_p(e["table"].data_ptr()), 1,
        C.c_void_p(e["markers"].data_ptr()), 0.0, 0.01, e["vi"], None, None, None, pde, ring, fld, pending)


def _rejected(rc, text):
    from beat import _hip

    with pytest.raises(_hip.BeatHipError) as exc:
        _hip.check(rc)
    assert str(exc.value).split(": ", 1)[1] == text


ENTRIES = {"pending": _pending, "rows": _rows, "classes": _classes}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_pending_count_above_the_maximum(env, entry):
    ops = env["ops"]
    _rejected(ENTRIES[entry](env, ops.handle, ops.ring[0].ptr, ops.fld, 13), "pending count 13 out of range")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_pending_without_operator_or_ring(env, entry):
    ops = env["ops"]
    _rejected(ENTRIES[entry](env, None, ops.ring[0].ptr, ops.fld, 2), "bad pending update")
    _rejected(ENTRIES[entry](env, ops.handle, None, ops.fld, 2), "bad pending update")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_behind_an_operator_without_an_open_solve(env, entry):
    ops = env["ops"]
    _rejected(ENTRIES[entry](env, ops.handle, ops.ring[0].ptr, ops.fld, -1), "pending = -1 needs an operator with an open solve")


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("pending", [0, 3])
def test_pending_while_the_operator_has_an_open_solve(env, entry, pending):
    var = env["var"]
    _rejected(ENTRIES[entry](env, var.handle, var.ring[0].ptr, var.fld, pending),
              "the operator has an open solve: finish it (beat_pde_solve_end) or pass pending = -1")


@pytest.mark.parametrize("entry", ["pending", "rows"])
def test_behind_a_solve_with_the_ring_of_12(env, entry):
    var = env["var"]
    _rejected(ENTRIES[entry](env, var.handle, var.ring[0].ptr, var.fld, -1),
              "this kernel's pending path takes 6 directions: finish the solve first")


def test_unknown_model_id(env):
    ctx, s, P, n = env["ctx"], env["states"], env["P"], env["n"]
    text = f"unknown model id {UNUSED_MODEL_ID}"
    ns, npar, per_class = C.c_int(0), C.c_int(0), C.c_int(0)
    hp = P.ctypes.data_as(C.c_void_p)
    _rejected(ctx.lib.beat_ode_model_info(UNUSED_MODEL_ID, C.byref(ns), C.byref(npar)), text)
    _rejected(ctx.lib.beat_ode_step(ctx.handle, UNUSED_MODEL_ID, s.ptr, n, s.ld, hp, len(P), None, 0, 0.0, 0.01, env["vi"], None), text)
    _rejected(ctx.lib.beat_ode_run(ctx.handle, UNUSED_MODEL_ID, s.ptr, n, s.ld, hp, len(P), None, 0, 0.0, 0.01, 1, 1, 1, None, 0, None), text)
    _rejected(ctx.lib.beat_ode_class_table_doubles(UNUSED_MODEL_ID, C.byref(per_class)), text)
    _rejected(ctx.lib.beat_ode_class_table_fill(ctx.handle, UNUSED_MODEL_ID, hp, len(P), 1, C.c_void_p(env["table"].data_ptr())), text)
