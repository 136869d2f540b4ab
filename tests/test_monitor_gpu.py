"""GPU: monitored values of a model generated from an ``.ode`` file, evaluated on the device (``ode_monitor_kernel``, compiled per
selection at first use) -- through the model handle (``monitor_values``), the solver's resident states (``_DeviceODE.monitor``,
``DolfinODESolver.monitor``) and the C entry point itself -- against ``numpy_monitor``, the NumPy evaluation of the same
expressions (held against the file's formulas in tests/test_monitor_cpu.py).

The error of a value is |dev - ref| / max(|ref|, S_k), S_k the largest finite |ref| of its row over the samples (dV_dt and its
like are sums of currents that cancel), and the bound 1e-11: what tests/test_ode_file_gpu.py holds the generated step to against
the NumPy evaluation of its expressions (the two sides take exp, log and pow from different libraries)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DATA = ROOT / "tests" / "data"
SMALL, LANGUAGE, BIG = DATA / "small_cell.ode", DATA / "language_cell.ode", DATA / "big_cell.ode"
BOUND = 1e-11
BIG_EIGHT = ["I_0", "E_3", "tau_x1_1", "dV_dt", "x5_2_inf", "dc_6_dt", "I_9", "dx11_0_dt"]  # one or two of every kind of component


def _error(dev, ref):
    dev, ref = np.atleast_2d(dev), np.atleast_2d(ref)
    ok = np.isfinite(ref)
    assert dev.shape == ref.shape and np.isfinite(dev[ok]).all()
    scale = np.where(ok, np.abs(ref), 0.0).max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        err = np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), scale), 1e-300)
    return np.where(ok, err, 0.0)


def _check(dev, ref, names, what):
    err = _error(dev, ref)
    worst = err.max(axis=1)
    k = int(worst.argmax())
    print(f"{what}: worst row {names[k]} {worst[k]:.3e}")
    assert worst[k] <= BOUND, (what, {nm: float(e) for nm, e in zip(names, worst) if e > BOUND})


@pytest.fixture(scope="module")
def small():
    from beat.models import from_ode

    return from_ode(SMALL)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_all_names_at_the_tile_edges(hip_ctx, small, n):
    """One node, one short of a tile, a tile, one more (the second block holds a single node: the bounds guard must come after
    the block's table set-up), several tiles; outside and inside the stimulus window."""
    model = small
    names = list(model.monitor_names)
    y = model._sample_states(n)
    p = model.init_parameter_values(stim_amplitude=30.0)
    for t in (0.2, 1.0):
        dev = model.monitor_values(t, y, p)
        assert dev.shape == (len(names), n)
        _check(dev, model.numpy_monitor(y, t, p), names, f"n={n} t={t}")
    assert model.monitor_values(1.0, y, p, ["i_stim"]).max() == 30.0 and model.monitor_values(0.2, y, p, ["i_stim"]).max() == 0.0
    one = model.monitor_values(1.0, y[:, 0], p, ["i_in", "dV_dt"])  # (S,) states give (M,)
    assert one.shape == (2,)
    np.testing.assert_array_equal(one, model.monitor_values(1.0, y, p, ["i_in", "dV_dt"])[:, 0])


def test_per_node_rows(hip_ctx, small):
    model = small
    n = 257
    names = list(model.monitor_names)
    y = model._sample_states(n, seed=3)
    p = np.repeat(model.init_parameter_values(stim_amplitude=30.0)[:, None], n, axis=1)
    p[model.parameter_index("g_in")] *= np.linspace(0.5, 1.5, n)
    for t in (0.2, 1.0):
        _check(model.monitor_values(t, y, p), model.numpy_monitor(y, t, p), names, f"per-node t={t}")
    # the gradient is in the result: i_in of two nodes with the same states differs by the ratio of their g_in
    y2 = np.repeat(y[:, 5:6], n, axis=1)
    i_in = model.monitor_values(0.2, y2, p, ["i_in"])[0]
    np.testing.assert_allclose(i_in / i_in[0], p[model.parameter_index("g_in")] / p[model.parameter_index("g_in"), 0], rtol=1e-14)


def test_classes_and_nodes_of_no_class(hip_ctx, small):
    """Two parameter sets and a marker byte per node, 255 on about a tenth of the nodes: NaN in every row exactly there, the
    class's values elsewhere -- through the solver's resident array and its class table (_DeviceODE)."""
    import beat
    from beat._device import StateArray
    from beat.odesolver import _DeviceODE

    model = small
    n = 1000
    names = list(model.monitor_names)
    rng = np.random.default_rng(8)
    y = model._sample_states(n, seed=4)
    sets = [model.init_parameter_values(stim_amplitude=30.0), model.init_parameter_values(stim_amplitude=12.0, g_in=7.0, v_pump=0.03)]
    marks = np.where(np.arange(n) < 430, 0, 1).astype(np.uint8)  # the boundary inside a wavefront (430 = 6 * 64 + 46)
    none = rng.random(n) < 0.1
    marks[none] = 255
    assert 50 < none.sum() < 150
    ode = _DeviceODE(hip_ctx, model, model.num_states, n, 0, None, beat.telemetry.NullMonitor())
    ode.set_initial(y)
    ode.explicit_classes = True
    ode.set_classes(hip_ctx.from_numpy(marks), sets)
    out = StateArray(hip_ctx, len(names), n)
    p_node = np.stack([sets[0] if m != 1 else sets[1] for m in marks], axis=1)
    for t in (0.2, 1.0):
        ode.monitor_rows(names, t, out.ptr, out.ld)
        dev = out.numpy()
        assert np.isnan(dev[:, none]).all() and np.isfinite(dev[:, ~none]).all()
        ref = model.numpy_monitor(y, t, p_node)
        _check(dev[:, ~none], ref[:, ~none], names, f"classes t={t}")
    k = names.index("i_stim")
    assert set(np.unique(dev[k, ~none])) == {12.0, 30.0}
    np.testing.assert_array_equal(ode.states.numpy(), y)


def test_the_pass_is_read_only_and_keeps_to_its_rows(hip_ctx, small):
    """beat_ode_monitor on a resident array: every byte of the state buffer (rows, padding between them, ghost planes) is what it
    was, and with out_ld = n + 64 the 64 doubles behind each output row keep the sentinel the buffer was filled with."""
    from beat._device import StateArray

    model = small
    n, plane = 777, 37
    names = ["i_in", "dV_dt", "j_pump", "beta_h"]
    sa = StateArray(hip_ctx, model.num_states, n, plane)
    rng = np.random.default_rng(1)
    sa.buf.copy_(hip_ctx.from_numpy(rng.uniform(-1.0, 1.0, sa.buf.numel())))  # (the padding too holds something to lose)
    y = model._sample_states(n, seed=6)
    sa.set(y)
    before = sa.buf.cpu().numpy().tobytes()
    out_ld, sentinel = n + 64, -12345.678
    out = hip_ctx.from_numpy(np.full(len(names) * out_ld + 64, sentinel))
    p = model.init_parameter_values(stim_amplitude=30.0)
    model.monitor_on_device(hip_ctx, names, sa.ptr, n, sa.ld, 1.0, C.c_void_p(out.data_ptr() + 8 * 32), out_ld, host_params=p)
    hip_ctx.synchronize()
    assert sa.buf.cpu().numpy().tobytes() == before
    o = out.cpu().numpy()
    assert (o[:32] == sentinel).all() and (o[32 + len(names) * out_ld:] == sentinel).all()
    rows = o[32:32 + len(names) * out_ld].reshape(len(names), out_ld)
    assert (rows[:, n:] == sentinel).all()
    _check(rows[:, :n], model.numpy_monitor(y, 1.0, p, names), names, "resident array")
    # what the entry point refuses: out_ld < n, a parameter count that is not the model's, output rows inside the state array
    from beat import _hip

    mid = model._monitor_launches(names)[0][0]
    hp = np.ascontiguousarray(p)
    good = dict(ctx=hip_ctx.handle, mid=mid, states=sa.ptr, n=n, ld=sa.ld, host_params=hp.ctypes.data_as(C.c_void_p), num_params=len(hp),
                per_node=None, params_ld=0, table=None, num_classes=0, markers=None, t=1.0, out=C.c_void_p(out.data_ptr()), out_ld=out_ld)
    for bad in (dict(out_ld=n - 1), dict(num_params=len(hp) - 1), dict(out=sa.row_field(2).ptr), dict(mid=10_000),
                dict(markers=C.c_void_p(out.data_ptr()))):  # (markers without a table)
        with pytest.raises(_hip.BeatHipError):
            _hip.check(hip_ctx.lib.beat_ode_monitor(*{**good, **bad}.values()))
    hip_ctx.synchronize()
    assert sa.buf.cpu().numpy().tobytes() == before


def test_every_function_of_the_language(hip_ctx):
    from beat.models import from_ode

    model = from_ode(LANGUAGE)
    names = list(model.monitor_names)
    assert len(names) == 65
    y = model._sample_states(1000)
    p = model.init_parameter_values()
    for t in (0.2, 1.0):
        dev = model.monitor_values(t, y, p)
        _check(dev, model.numpy_monitor(y, t, p), names, f"language t={t}")


def test_eight_names_of_the_big_model(hip_ctx):
    from beat.models import from_ode

    model = from_ode(BIG)
    y = model._sample_states(1000)
    p = model.init_parameter_values(stim_amplitude=30.0)
    for t in (0.2, 1.0):
        _check(model.monitor_values(t, y, p, BIG_EIGHT), model.numpy_monitor(y, t, p, BIG_EIGHT), BIG_EIGHT, f"big t={t}")
    pn = np.repeat(p[:, None], 1000, axis=1)
    pn[model.parameter_index("g_3")] *= np.linspace(0.5, 1.5, 1000)
    _check(model.monitor_values(1.0, y, pn, BIG_EIGHT), model.numpy_monitor(y, 1.0, pn, BIG_EIGHT), BIG_EIGHT, "big per-node")


def test_a_list_longer_than_one_launch_is_split(hip_ctx):
    """33 names: two launches, of 32 names and of one -- the same bits as those 32 and that one asked for in two calls (the rows of
    the second launch land behind the first's).  Asked for in two OTHER runs, 20 + 13, the names are other selections: common
    subexpressions are eliminated per selection, which may associate a product differently, so those agree to rounding -- held
    to the bound of this file -- and not bit for bit."""
    from beat import _hip
    from beat.models import from_ode

    model = from_ode(LANGUAGE)
    names = list(model.monitor_names[:_hip.MAX_MONITORS + 1])
    assert len(names) == 33 and [m for _, m in model._monitor_launches(names)] == [32, 1]
    y = model._sample_states(300, seed=2)
    p = model.init_parameter_values()
    whole = model.monitor_values(0.7, y, p, names)
    assert whole.shape == (33, 300)
    np.testing.assert_array_equal(whole, np.concatenate([model.monitor_values(0.7, y, p, names[:32]), model.monitor_values(0.7, y, p, names[32:])]))
    other = np.concatenate([model.monitor_values(0.7, y, p, names[:20]), model.monitor_values(0.7, y, p, names[20:])])
    _check(other, whole, names, "33 names as 20 + 13")
    _check(whole, model.numpy_monitor(y, 0.7, p, names), names, "33 names")


def _slab_solver(model, **kw):
    import beat
    from beat import grid as g

    # 41 x 21 x 11 = 9471 nodes: more than the one-workgroup solve of small grids takes (8192), which defers nothing
    geo = beat.geometry.get_3D_slab_geometry(comm=g.COMM_WORLD, Lx=6.0, Ly=3.0, Lz=1.5, dx=0.15)
    mesh = geo.mesh
    time = g.Constant(mesh, 0.0)
    cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 1.0 + 1e-10) & (x[1] <= 1.0 + 1e-10))
    tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
    I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=1400.0 * beat.units.ureg("cm**-1"), time=time, subdomain_data=tags, marker=1,
                                           mesh_unit="mm", amplitude=50_000.0, start=0.0, duration=1.5)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([9.5e-4, 2.5e-4, 2.5e-4]), I_s=I_s, C_m=0.01, dx=I_s.dZ,
                               params={"petsc_options": {"ksp_rtol": 1e-12}})
    ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state, fun=model,
                                         init_states=model.init_state_values(), parameters=model.init_parameter_values(stim_amplitude=0.0),
                                         num_states=model.num_states, v_index=model.state_index("V"), **kw)
    return beat.MonodomainSplittingSolver(pde=pde, ode=ode)


def test_solver_monitor_reads_a_complete_potential_and_leaves_the_run_alone(hip_ctx, small):
    """A split step leaves its diffusion solve open and the last update of the potential to the next ionic launch: monitor()
    between steps must finish both before it reads the row -- its functions equal numpy_monitor of the states as full_values
    gives them -- and a run that monitors after steps 3 and 8 ends on the bits of one that does not."""
    model = small
    names = ["i_in", "dV_dt", "j_pump"]
    dt, nsteps = 0.05, 12
    import beat

    telemetry = beat.telemetry.NullMonitor()
    a, b = _slab_solver(model), _slab_solver(model, monitor=telemetry)
    assert a.ode.on_device and a._can_fuse()
    ivs, t0 = [], 0.0
    for _ in range(nsteps):
        ivs.append((t0, t0 + dt))
        t0 = t0 + dt
    for iv in ivs:
        a.step(iv)
    reuse = None
    for i, iv in enumerate(ivs):
        b.step(iv)
        if i + 1 in (3, 8):
            assert b.pde._ops.open_x is not None or b.pde._ops.pending is not None  # the row is NOT complete as the step left it
            t = iv[1]
            funs = b.ode.monitor(names, t, out=reuse)  # (first call: new functions; second: the caller's own)
            assert b.ode.monitor.telemetry is telemetry  # `monitor` is still the dataclass's telemetry field, too
            assert [f.function_space for f in funs] == [b.ode.v_ode.function_space] * 3
            dev = np.array([np.asarray(f.x.array) for f in funs])
            ref = model.numpy_monitor(b.ode.full_values, t, b.ode.parameters, names)
            _check(dev, ref, names, f"solver, after step {i + 1}")
            assert reuse is None or all(f is r for f, r in zip(funs, reuse))
            reuse = funs
    va, vb = np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array)
    assert va.max() > model.state_defaults["V"] + 10.0  # the stimulus acts: the corner has left rest (-84 mV)
    assert va.tobytes() == vb.tobytes()
    assert np.asarray(a.ode.full_values).tobytes() == np.asarray(b.ode.full_values).tobytes()


def test_what_is_out_of_scope_says_so(hip_ctx, small):
    import beat
    from beat import grid as g
    from beat.models import tp06

    with pytest.raises(NotImplementedError, match="from_ode"):
        tp06.generalized_rush_larsen.monitor_values(0.0, tp06.init_state_values(), tp06.init_parameter_values())
    mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([1.0, 1.0, 1.0])], [4, 4, 4])
    V = g.functionspace(mesh, ("P", 1))
    markers = g.Function(V)
    markers.x.array[:] = np.where(V.tabulate_dof_coordinates()[:, 0] < 0.5, 0.0, 1.0)
    multi = beat.odesolver.DolfinMultiODESolver(
        v_ode=g.Function(V), v_pde=g.Function(V), markers=markers, num_states={k: small.num_states for k in (0, 1)},
        fun={k: small for k in (0, 1)}, init_states={k: small.init_state_values() for k in (0, 1)},
        parameters={k: small.init_parameter_values() for k in (0, 1)}, v_index={k: small.state_index("V") for k in (0, 1)})
    with pytest.raises(NotImplementedError, match="DolfinMultiODESolver"):
        multi.monitor(["i_in"], 0.0)
    shipped = beat.odesolver.DolfinODESolver(v_ode=g.Function(V), v_pde=g.Function(V), fun=tp06.generalized_rush_larsen,
                                             init_states=tp06.init_state_values(), parameters=tp06.init_parameter_values(),
                                             num_states=19, v_index=tp06.state_index("V"))
    with pytest.raises(NotImplementedError, match="from_ode"):
        shipped.monitor(["i_Na"], 0.0)
    with pytest.raises(KeyError, match="Unknown monitor"):
        small.monitor_values(0.0, small.init_state_values(), small.init_parameter_values(), ["i_nope"])


def test_monitor_currents_demo(hip_ctx, capsys):
    """demos/monitor_currents.py: i_in and j_pump across the front of a wave started in a corner, from the device."""
    import importlib.util

    demos = ROOT / "demos"
    sys.path.insert(0, str(demos))
    try:
        spec = importlib.util.spec_from_file_location("demo_monitor_currents", demos / "monitor_currents.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(str(demos))
    out, v, solver = mod.main(["--dx", "0.5", "--steps", "40"])
    text = capsys.readouterr().out
    assert "i_in in [" in text and "j_pump in [" in text
    assert v.max() > -40.0 > v.min()  # a front: part of the slab is up, part at rest
    assert out["i_in"].min() < -1.0 and abs(out["i_in"].max()) < 1.0  # the inward current flows where the front is, and only there
    assert (out["j_pump"] > 0.0).all()
