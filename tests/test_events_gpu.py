"""Event maps on the device (csrc/beat_events.hip, beat.EventRecorder): the kernel against the NumPy restatement of its rule
(tests/_events_ref.py), the pass that is also the deferred update of the potential against the two passes it replaces, and the
recorder against the host loop of the reference's demos (demos/irksome_model_gotranx.py:251-254: read the potential after every
step, ``crossed = (v >= threshold) & (tact < 0); tact[crossed] = t``)."""
import ctypes as C
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _events_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MARK = 7.25e11  # what the ghost planes of every operand hold
EPS = np.finfo(np.float64).eps
T_START = 3.0


def _field(ctx, n, plane, values):
    f = ctx.field(n, plane)
    f.buf.fill_(MARK)
    f.set(values)
    return f


def _ghosts_untouched(f):
    return bool((f.ghost_lo == MARK).all().item()) and bool((f.ghost_hi == MARK).all().item())


def _changed(a, b):
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def _initial(key, n):
    return np.full(n, np.nan if key in ref.TIME_MAPS else -np.inf)


def _needs_prev(keys, mode):
    return bool({"act_last", "repol", "apd", "dvdt_max"} & set(keys)) or (mode == 1 and "act_first" in keys)


def _event_maps(fields, thr_up, thr_down, mode, strict):
    from beat import _hip

    return _hip.EventMaps(thr_up=thr_up, thr_down=thr_down, mode=mode, strict=strict, **{k: f.ptr.value for k, f in fields.items()})


@functools.lru_cache(maxsize=None)
def _reference(n, mode, strict):
    V, special = ref.sequence(n)
    m, ups, downs = ref.run(V, mode, bool(strict), t_start=T_START)
    return V, special, m, ups, downs


# which maps a run keeps: (selected, kept beside them because a selected one needs it)
FAMILIES = {
    "no_v_prev": (("act_first", "v_max"), ()),  # (step mode: no v_prev at all; linear mode: act_first needs it)
    "all": (ref.ALL_MAPS, ()),
    "act_first": (("act_first",), ()),
    "act_last": (("act_last",), ()),
    "repol": (("repol",), ("act_last",)),
    "apd": (("apd",), ("act_last",)),
    "dvdt_max": (("dvdt_max",), ()),
    "v_max": (("v_max",), ()),
}
SIZES = {"1": (1, 1), "257": (257, 257), "70x9x5": (70 * 9 * 5, 70 * 9)}  # (nodes, ghost plane)


def _assert_map(key, got, m, mode):
    want = m[key]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{key}: NaN pattern")
    ok = ~np.isnan(want)
    if mode == 0 or key not in ref.TIME_MAPS:
        # a copy of t1, or one correctly rounded subtraction and division
        np.testing.assert_array_equal(got[ok], want[ok], err_msg=key)
        return
    # a linear time: three roundings on a quotient in [0, 1] times dt, added to t0 -- 8 eps (|t0| + dt), with t0 the start of the
    # step that wrote the entry (for an APD: of the step of its repolarisation)
    tol = 8 * EPS * (np.abs(m["t0_" + key][ok]) + ref.DT)
    err = np.abs(got[ok] - want[ok])
    print(key, "linear: largest error", float(err.max(initial=0.0)), "smallest bound", float(tol.min(initial=np.inf)))
    assert (err <= tol).all(), (key, float(err.max()), float(tol.min()))


@pytest.mark.parametrize("compare", [">=", ">"])
@pytest.mark.parametrize("mode", ["step", "linear"])
@pytest.mark.parametrize("size", list(SIZES))
def test_kernel_matches_the_restatement(hip_ctx, size, mode, compare):
    """beat_field_events over 40 steps of a synthetic potential: every family of maps (none that needs v_prev, all, each alone),
    both modes, both compares, on 1, 257 and 70 x 9 x 5 nodes (nx > 64, not a multiple of 256, first node not on a 512-byte
    boundary).  Step-mode times, v_max and dvdt_max are equal, linear times within 8 eps (|t0| + dt), the NaN pattern identical,
    v_prev ends as the last potential and no ghost plane of any operand changes."""
    from beat import _hip

    n, plane = SIZES[size]
    imode, strict = {"step": 0, "linear": 1}[mode], {">=": 0, ">": 1}[compare]
    V, special, m, ups, downs = _reference(n, imode, strict)
    # the sequence holds every kind of node the rule distinguishes (checked on the host, before anything runs on the device)
    kinds = ref.kinds(V, m, ups, downs, bool(strict))
    print(size, mode, compare, kinds)
    if n >= 257:
        assert kinds["start_above"] >= 1 and kinds["never"] >= 1 and kinds["twice"] >= 1 and kinds["recross"] >= 1
        assert kinds["vn_on_threshold"] >= 1 and kinds["vp_on_threshold"] >= 1 and kinds["repolarised"] >= 1
        assert ups[special["never"]] == 0 and ups[special["recross"]] >= 10 and ups[special["stays"]] == 1
        # the node that sits on thr_up: activated by the step that reaches it (>=; its linear time is that step's end) or by the
        # one that leaves it upwards (>; vp is not below thr_up: the linear time is that step's start)
        exact_step = 5 if strict == 0 else (7 if imode == 0 else 6)
        assert ups[special["exact"]] == 1 and abs(m["act_first"][special["exact"]] - (T_START + exact_step * ref.DT)) < 1e-12
    else:  # the one node: both pulses pass it
        assert ups[0] >= 2 and downs[0] >= 2
    Vdev = hip_ctx.from_numpy(V)
    for family, (selected, helpers) in FAMILIES.items():
        keys = tuple(selected) + tuple(helpers)
        fields = {k: _field(hip_ctx, n, plane, _initial(k, n)) for k in keys}
        if _needs_prev(keys, imode):
            fields["v_prev"] = _field(hip_ctx, n, plane, V[0])
        assert ("v_prev" in fields) == (family != "v_max" and not (imode == 0 and family in ("no_v_prev", "act_first")))
        v = _field(hip_ctx, n, plane, V[0])
        args = _event_maps(fields, ref.THR_UP, ref.THR_DOWN, imode, strict)
        for k in range(1, ref.NSTEPS + 1):
            v.data.copy_(Vdev[k])
            t0 = T_START + (k - 1) * ref.DT
            _hip.check(hip_ctx.lib.beat_field_events(hip_ctx.handle, v.ptr, n, C.byref(args), t0, t0 + ref.DT))
        for k in keys:
            _assert_map(k, fields[k].numpy(), m, imode)
        if "v_prev" in fields:
            np.testing.assert_array_equal(fields["v_prev"].numpy(), V[-1])
        np.testing.assert_array_equal(v.numpy(), V[-1])
        for k, f in list(fields.items()) + [("v", v)]:
            assert _ghosts_untouched(f), (family, k)


# ---- the pass that is also the deferred update of the potential -------------------------------------------------------------
CELLS = (69, 8, 4)  # 70 x 9 x 5 nodes
NN = tuple(c + 1 for c in CELLS)
H = 0.1


def _bump(t):
    iz, iy, ix = np.meshgrid(*(np.arange(k) for k in NN[::-1]), indexing="ij")
    x = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) * H
    c = np.array([1.5 + 3.0 * t, 0.4, 0.2])
    return -85.0 + 100.0 * np.exp(-((x - c) ** 2).sum(axis=1) / (2 * 0.25**2))


def _deferred_solve(ctx, order):
    """A constant-coefficient operator on the multi-launch kernels with one theta-step solved and its last directions pending
    (with ``order``: after three recorded solves, so that the update carries the initial guess's bookkeeping)."""
    from beat import _stencil
    from beat._engine import HipOps

    M = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.1], [0.0, 0.1, 0.5]]) * 1e-3
    ops = HipOps(ctx, NN, True, True, *_stencil.stencil_tables(3, (H,) * 3, M))
    ops.set_small(False)
    ops.set_guess_order(order)
    ops.set_timestep(0.01, 0.5, 0.05)
    assert not ops.small_active()
    fv, fx = ops.new_field(), ops.new_field()
    if order:
        for s in range(3):
            fv.set(_bump(0.02 * s))
            assert ops.solve_single(fv, [], [], fx, 1e-9, 1e-50, 500).converged_reason > 0
    fv.set(_bump(0.5))
    res = ops.solve_single(fv, [], [], fx, 1e-9, 1e-50, 500, defer_flush=True)
    assert res.converged_reason > 0 and ops.pending is not None and ops.pending[2] > 0  # directions are pending
    assert bool(ops.lib.beat_pde_guess_pending(ops.handle)) == bool(order)  # (which branch of x_flush_kernel the update takes)
    return ops, fv, fx


def _guess_fields(ctx, ops, n):
    from beat import _hip

    d, e, cnt = C.c_void_p(), C.c_void_p(), C.c_int()
    _hip.check(ops.lib.beat_pde_guess_history(ops.handle, C.byref(d), C.byref(e), C.byref(cnt)))
    out = []
    for p in (d, e):
        host = np.empty(n)
        _hip.check(ctx.lib.beat_memcpy_d2h(ctx.handle, host.ctypes.data_as(C.c_void_p), p, 8 * n))
        out.append(host)
    return out


def _maps_with_history(ctx, fv, mode):
    """All maps of a field like ``fv``, with a history that makes the step under test find events of both kinds whatever the
    solve does: every node was activated by an earlier observation (of a field that lies above the threshold everywhere), and the
    potential a step ago is -65 mV everywhere -- below thr_up = -60, which the bump's core exceeds, and above thr_down = -70, which
    the resting far field lies under."""
    from beat import _hip

    n = fv.n
    fields = {k: _field(ctx, n, fv.plane, _initial(k, n)) for k in ref.ALL_MAPS}
    fields["v_prev"] = _field(ctx, n, fv.plane, np.full(n, -80.0))
    args = _event_maps(fields, -60.0, -70.0, mode, 0)
    above = _field(ctx, n, fv.plane, np.zeros(n))
    _hip.check(ctx.lib.beat_field_events(ctx.handle, above.ptr, n, C.byref(args), 0.0, 0.05))
    fields["v_prev"].set(np.full(n, -65.0))
    return fields, args


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("order", [0, 2])
def test_fused_flush_equals_flush_then_events(hip_ctx, order, mode):
    """beat_pde_x_flush_events against beat_pde_x_flush followed by beat_field_events on two copies of the same state, with
    ksp_guess_order 0 (the plain branch of x_flush_kernel) and 2 after three recorded solves (the branch that records the
    increment): x, the guess's d and e and every map bit for bit.  What it refuses (null v, a down map without act_last, a mode
    out of range) returns BEAT_EINVAL and leaves x, the maps and what is pending as they were."""
    from beat import _hip

    lib = hip_ctx.lib
    n = int(np.prod(NN))
    a, av, ax = _deferred_solve(hip_ctx, order)
    b, bv, bx = _deferred_solve(hip_ctx, order)
    np.testing.assert_array_equal(ax.numpy(), bx.numpy())
    assert a.pending[1:] == b.pending[1:]
    fa, args_a = _maps_with_history(hip_ctx, av, mode)
    fb, args_b = _maps_with_history(hip_ctx, bv, mode)
    before = {k: f.numpy() for k, f in fa.items()}
    x_before = ax.numpy()

    def fused(x_ptr, args):
        return lib.beat_pde_x_flush_events(a.handle, C.c_void_p(a.st_ptr_for_flush), x_ptr, a.ring[0].ptr, a.fld, a.pending[1],
                                           C.byref(args), 0.05, 0.1)

    no_last = _hip.EventMaps.from_buffer_copy(args_a)
    no_last.act_last = None
    bad_mode = _hip.EventMaps.from_buffer_copy(args_a)
    bad_mode.mode = 2
    for rc in (fused(None, args_a), fused(ax.ptr, no_last), fused(ax.ptr, bad_mode)):
        assert rc == -1  # BEAT_EINVAL
    hip_ctx.synchronize()
    np.testing.assert_array_equal(ax.numpy(), x_before)
    for k, f in fa.items():
        np.testing.assert_array_equal(f.numpy(), before[k], err_msg=k)
    assert bool(lib.beat_pde_guess_pending(a.handle)) == bool(order)

    _hip.check(fused(ax.ptr, args_a))
    b.flush_pending()
    _hip.check(lib.beat_field_events(hip_ctx.handle, bx.ptr, n, C.byref(args_b), 0.05, 0.1))
    assert not lib.beat_pde_guess_pending(a.handle) and not lib.beat_pde_guess_pending(b.handle)
    xa = ax.numpy()
    assert np.abs(xa - x_before).max() > 0.0  # the update was due
    np.testing.assert_array_equal(xa, bx.numpy())
    if order:
        for ga, gb in zip(_guess_fields(hip_ctx, a, n), _guess_fields(hip_ctx, b, n)):
            assert np.abs(ga).max() > 0.0
            np.testing.assert_array_equal(ga, gb)
    for k in fa:
        np.testing.assert_array_equal(fa[k].numpy(), fb[k].numpy(), err_msg=k)
        assert _ghosts_untouched(fa[k]), k
    np.testing.assert_array_equal(fa["v_prev"].numpy(), xa)
    # the step had something to find: activations in the bump's core, repolarisations in the far field
    assert _changed(fa["act_last"].numpy(), before["act_last"]).sum() > 0
    assert _changed(fa["repol"].numpy(), before["repol"]).sum() > 0


def test_refused_arguments(hip_ctx):
    """Both entry points return BEAT_EINVAL before anything is enqueued: an open solve on the handle, and what beat_field_events
    checks by itself (null v, n = 0, an empty step, a map that needs v_prev without it)."""
    from beat import _hip

    lib = hip_ctx.lib
    ops, fv, fx = _deferred_solve(hip_ctx, 0)
    ops.flush_pending()
    fields, args = _maps_with_history(hip_ctx, fv, 0)
    before = {k: f.numpy() for k, f in fields.items()}
    assert ops.can_open()
    ops.solve_begin(fv, [], [], fx, 1e-9, 1e-50, 500)
    rc = lib.beat_pde_x_flush_events(ops.handle, None, fx.ptr, ops.ring[0].ptr, ops.fld, 0, C.byref(args), 0.05, 0.1)
    assert rc == -1 and b"open solve" in lib.beat_last_error()
    assert ops.solve_finish().converged_reason > 0
    ops.flush_pending()
    n = fv.n
    no_prev = _hip.EventMaps.from_buffer_copy(args)
    no_prev.v_prev = None
    assert lib.beat_field_events(hip_ctx.handle, None, n, C.byref(args), 0.05, 0.1) == -1
    assert lib.beat_field_events(hip_ctx.handle, fx.ptr, 0, C.byref(args), 0.05, 0.1) == -1
    assert lib.beat_field_events(hip_ctx.handle, fx.ptr, n, C.byref(args), 0.1, 0.1) == -1
    assert lib.beat_field_events(hip_ctx.handle, fx.ptr, n, C.byref(no_prev), 0.05, 0.1) == -1
    assert lib.beat_field_events(hip_ctx.handle, fx.ptr, n, None, 0.05, 0.1) == -1
    hip_ctx.synchronize()
    for k, f in fields.items():
        np.testing.assert_array_equal(f.numpy(), before[k], err_msg=k)


# ---- the recorder against the reference demos' host loop ----------------------------------------------------------------------
def _steps(T0, T, dt):
    """The steps MonodomainSplittingSolver.solve makes."""
    steps, t0, t1 = [], T0, T0 + dt
    while t1 < T + 1e-12:
        steps.append((t0, t1))
        t0 = t1
        t1 = t0 + dt
    return steps


def _host_loop(solver, f, steps, threshold, strict, v_max=False):
    """demos/irksome_model_gotranx.py:244-254 (not-yet-activated is NaN here, -1 there)."""
    tact = np.full(f.x.array.size, np.nan)
    vmax = np.full(f.x.array.size, -np.inf)
    for t0, t1 in steps:
        solver.step((t0, t1))
        v = np.asarray(f.x.array)
        crossed = ((v > threshold) if strict else (v >= threshold)) & np.isnan(tact)
        tact[crossed] = t1
        vmax = np.where(v > vmax, v, vmax)
    return (tact, vmax) if v_max else tact


def _tp06_slab(Lx, Ly, Lz, dx):
    import beat
    from beat import grid as g
    from beat.models import tp06

    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=Lx, Ly=Ly, Lz=Lz, dx=dx)
    mesh = geo.mesh
    cond = beat.conductivities.default_conductivities("Niederer")
    C_m = (1.0 * beat.units.ureg("uF/cm**2")).to("uF/mm**2").magnitude
    time = g.Constant(mesh, 0.0)
    cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 1.5 + 1e-10) & (x[1] <= 1.5 + 1e-10) & (x[2] <= 1.5 + 1e-10))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                           mesh_unit="mm", amplitude=50_000.0)
    M = beat.conductivities.define_conductivity_tensor(f0=geo.f0, **cond)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=C_m, dx=I_s.dZ)
    ic = tp06.init_state_values()
    ode = beat.odesolver.DolfinODESolver(
        v_ode=g.Function(g.functionspace(mesh, ("Lagrange", 1))), v_pde=pde.state, fun=tp06.generalized_rush_larsen,
        init_states=ic, parameters=tp06.init_parameter_values(stim_amplitude=0.0), num_states=len(ic),
        v_index=tp06.state_index("V"))
    return beat.MonodomainSplittingSolver(pde=pde, ode=ode)


@pytest.mark.parametrize("slab,nodes,fused,nsteps", [((9.6, 4.8, 1.6, 0.2), 11025, True, 200), ((20.0, 7.0, 3.0, 0.5), 4305, False, 500)])
def test_recorder_equals_the_host_loop_on_a_tp06_slab(slab, nodes, fused, nsteps):
    """TP06 on a slab with a corner stimulus, steps of 0.05 ms, twice from the same inputs: solve(..., recorder=...) against
    the reference demo's loop (step, read the potential, mask).  48 x 24 x 8 cells are above the one-launch limit: the
    observations are the deferred update of the potential as well (beat_pde_x_flush_events); 20 x 7 x 3 mm at dx = 0.5 is the
    one-launch solve, which leaves nothing pending.  The maps are equal, and so are the final states.  T = 10 ms and 25 ms: at the
    Niederer table's conduction velocities (0.6 / 0.25 mm/ms along / across the fibres at dx = 0.2, 0.57 / 0.14 at dx = 0.5) the
    front has then passed some 40 % of either slab."""
    import beat

    dt = 0.05
    steps = _steps(0.0, nsteps * dt, dt)
    assert len(steps) == nsteps
    a = _tp06_slab(*slab)
    assert a.pde.state.x.array.size == nodes and a.pde._ops.small_active() == (not fused)
    rec = beat.EventRecorder(a.pde.state, 0.0, compare=">")
    assert not a._can_batch(rec)
    a.solve((0.0, nsteps * dt), dt, recorder=rec)
    b = _tp06_slab(*slab)
    tact = _host_loop(b, b.pde.state, steps, 0.0, True)
    got = np.asarray(rec.activation.x.array)
    done = ~np.isnan(tact)
    print(f"{nodes} nodes: {done.sum()} activated, fused passes {rec.fused_passes}")
    assert done.sum() >= nodes / 4 and (~done).sum() >= 1
    np.testing.assert_array_equal(got, tact)
    np.testing.assert_array_equal(np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array))
    np.testing.assert_array_equal(a.ode.values, b.ode.values)
    # (a solve that leaves neither directions nor a guess increment behind has nothing to fuse with; on a travelling front few do)
    assert rec.fused_passes > nsteps // 2 if fused else rec.fused_passes == 0
    if fused:
        assert a.pde._ops.flushes == rec.fused_passes  # no other pass over the potential: the reads above found it complete


def test_recorder_on_the_literal_sequence_with_an_irksome_model():
    """IrksomeMonodomainModel + DolfinODESolver (FitzHugh-Nagumo scaled to [0, 1]) on a 24 x 24 unit square, started from v = 1 on
    a strip as demos/irksome_model_gotranx.py:128-130 does: the splitting solver takes the literal sequence, nothing is ever
    pending, and the recorder holds what the demo's loop (>= 0.02, :251-254) computes.  All maps are kept beside the activation; a
    list of recorders is accepted."""
    import beat
    from beat import butcher, grid as g

    def build():
        mesh = g.create_unit_square(g.COMM_WORLD, 24, 24, g.CellType.triangle)
        time = g.Constant(mesh, 0.0)
        pde = beat.IrksomeMonodomainModel(time=time, mesh=mesh, M=0.004, butcher_tableau=butcher.BackwardEuler(), I_s=None,
                                          params={"petsc_options": {"ksp_type": "cg", "ksp_rtol": 1e-6}})
        v_ode = g.Function(g.functionspace(mesh, ("P", 1)))
        v_ode.interpolate(lambda x: np.where(x[0] <= 0.05, 1.0, 0.0))
        init = np.zeros((2, v_ode.x.array.size))
        init[1] = np.asarray(v_ode.x.array)
        # (c_1, c_2, c_3, a, b, v_amp, v_rest, v_peak, stimulus amplitude, duration, start)
        parameters = np.array([0.26, 0.1, 1.0, 0.13, 0.013, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0])
        ode = beat.odesolver.DolfinODESolver(v_ode=v_ode, v_pde=pde.state, fun=beat.models.fhn.forward_euler_readme,
                                             init_states=init, parameters=parameters, num_states=2, v_index=1)
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode, theta=1.0)

    dt, nsteps = 0.1, 40
    steps = _steps(0.0, nsteps * dt, dt)
    a = build()
    assert not a._can_fuse()
    rec = beat.EventRecorder(a.pde.state, 0.02)
    rec_all = beat.EventRecorder(a.pde.state, 0.02, repolarisation_threshold=0.01, maps=tuple(beat.events.MAPS), mode="linear")
    a.solve((0.0, nsteps * dt), dt, recorder=[rec, rec_all])
    b = build()
    tact, vmax = _host_loop(b, b.pde.state, steps, 0.02, False, v_max=True)
    done = ~np.isnan(tact)
    print(f"{done.sum()} of {done.size} nodes activated")
    assert 0 < done.sum() < done.size
    np.testing.assert_array_equal(np.asarray(rec.activation.x.array), tact)
    np.testing.assert_array_equal(np.asarray(rec_all.v_max.x.array), vmax)
    np.testing.assert_array_equal(np.isnan(np.asarray(rec_all.activation.x.array)), ~done)
    first = np.asarray(rec_all.activation.x.array)[done]
    assert (first <= tact[done]).all() and (first >= tact[done] - dt - 1e-12).all()  # the crossing lies inside the step that found it
    assert rec.fused_passes == 0 and rec_all.fused_passes == 0
    rec.reset()
    assert np.isnan(np.asarray(rec.activation.x.array)).all()


def _shell_geometry(n, h):
    """A truncated ellipsoidal shell voxelised on a box, with a fibre field that rotates through the wall (the shape of
    test_var_gpu._shell_geometry): active voxels, transmural depth per voxel centre, fibres."""
    cx, cy, cz = n
    ax = [(np.arange(c) + 0.5) * h for c in n]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    c = np.array([cx, cy, cz]) * h / 2.0
    semi_o = 0.48 * np.array(n) * h
    semi_i = 0.62 * semi_o
    P = np.stack([X - c[0], Y - c[1], Z - c[2]], axis=-1)
    ro = np.sqrt(((P / semi_o) ** 2).sum(-1))
    ri = np.sqrt(((P / semi_i) ** 2).sum(-1))
    mask = (ro < 1.0) & (ri > 1.0) & (Z < 0.8 * cz * h)
    depth = np.clip((ri - 1.0) / np.maximum(ri - ro, 1e-12), 0.0, 1.0)
    rad = P / np.maximum(np.linalg.norm(P, axis=-1, keepdims=True), 1e-12)
    circ = np.cross(np.array([0.0, 0.0, 1.0]), rad)
    circ /= np.maximum(np.linalg.norm(circ, axis=-1, keepdims=True), 1e-12)
    longi = np.cross(rad, circ)
    ang = np.deg2rad(60.0 - 120.0 * depth)[..., None]
    f0 = np.cos(ang) * circ + np.sin(ang) * longi
    return mask, depth.reshape(-1), f0.reshape(-1, 3)


def test_recorder_on_a_voxel_shell():
    """Per-node operator rows on a voxelised shell, three TP06 cell types, endocardial stimulus: the potential's update is pending
    on the per-node-row operator, whose observation is its flush followed by the events pass.  Nodes outside the tissue (they
    hold 0 mV and never change: the threshold is compared with >) keep the NaN, the others equal the host loop."""
    import beat
    from beat import grid as g
    from beat.models import tp06

    n, h = (20, 18, 14), 0.5
    mask, depth, f0 = _shell_geometry(n, h)

    def build():
        mesh = g.create_voxel_mesh(g.COMM_WORLD, mask, h)
        cond = beat.conductivities.default_conductivities("Bishop")
        M = beat.conductivities.define_conductivity_tensor(f0=g.CellField(mesh, f0), **cond)
        time = g.Constant(mesh, 0.0)
        stim_cells = np.nonzero(np.repeat(mask.ravel() & (depth < 0.3), 6))[0]
        tags = g.meshtags(mesh, 3, stim_cells, np.full(len(stim_cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=cond["chi"], time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, start=0.0, duration=1.0)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=M, I_s=I_s, C_m=0.01, dx=I_s.dZ)
        V = g.functionspace(mesh, ("P", 1))
        active = mesh.node_active()
        z = mesh.node_coordinates(pad3=True)[:, 2]
        markers = g.Function(V)
        markers.x.array[:] = np.where(~active, -1.0, np.where(z < 2.5, 0.0, np.where(z < 4.5, 1.0, 2.0)))
        keys = (0, 1, 2)
        params = {0: tp06.init_parameter_values(stim_amplitude=0.0, g_Ks=0.098), 1: tp06.init_parameter_values(stim_amplitude=0.0),
                  2: tp06.init_parameter_values(stim_amplitude=0.0, g_to=0.073, g_Ks=0.392 * 1.2)}
        ic = tp06.init_state_values()
        ode = beat.odesolver.DolfinMultiODESolver(
            v_ode=g.Function(V), v_pde=pde.state, markers=markers, num_states={k: len(ic) for k in keys},
            fun={k: tp06.generalized_rush_larsen for k in keys}, init_states={k: ic for k in keys},
            parameters=params, v_index={k: tp06.state_index("V") for k in keys})
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode), active

    dt, nsteps = 0.05, 60  # the stimulus lasts 1 ms; the stimulated layer has fired by 3 ms, the rest of the wall has not
    steps = _steps(0.0, nsteps * dt, dt)
    a, active = build()
    assert a.pde._ops.per_node
    rec = beat.EventRecorder(a.pde.state, 0.0, maps=("activation", "v_max"), compare=">")
    a.solve((0.0, nsteps * dt), dt, recorder=rec)
    b, _ = build()
    tact, vmax = _host_loop(b, b.pde.state, steps, 0.0, True, v_max=True)
    got = np.asarray(rec.activation.x.array)
    print(f"{(~np.isnan(tact)).sum()} of {active.sum()} tissue nodes activated, fused passes {rec.fused_passes}")
    assert np.isnan(got[~active]).all() and 0 < (~np.isnan(got[active])).sum() < active.sum()
    np.testing.assert_array_equal(got, tact)
    np.testing.assert_array_equal(np.asarray(rec.v_max.x.array), vmax)
    np.testing.assert_array_equal(np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array))


def test_demo_runs_at_a_reduced_size():
    run = subprocess.run([sys.executable, str(ROOT / "demos" / "activation_map.py"), "--lx", "6", "--ly", "3", "--lz", "1", "--dx", "0.25",
                          "--T", "3"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "activation" in run.stdout
