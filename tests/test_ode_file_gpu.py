"""GPU: a cell model generated from a gotran ``.ode`` file (``beat.models.from_ode``) runs ON THE DEVICE through every route a
shipped model takes -- the reference hands any gotranx-generated ``fun`` to its solvers (/root/reference/demos/niederer_benchmark.py:82-99,
src/beat/odesolver.py:67-79); here an unknown model used to run on the host with a state round trip per step (VERDICT round 4,
item 8).  The file is tests/data/small_cell.ode, written for these tests; the checker is the generated NumPy evaluation, itself
held against an independent evaluation of the file in the CPU suite (tests/test_ode_file_cpu.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
BIG = ROOT / "tests" / "data" / "big_cell.ode"  # written by tests/data/make_big_cell.py


def _states(model, n, seed):
    rng = np.random.default_rng(seed)
    y = np.repeat(model.init_state_values()[:, None], n, axis=1)
    y[model.state_index("V")] = rng.uniform(-95.0, 45.0, n)
    for g in ("m", "h", "n"):
        y[model.state_index(g)] = rng.uniform(0.0, 1.0, n)
    y[model.state_index("ca")] = 10.0 ** rng.uniform(-4.5, -2.5, n)
    return y


def test_generated_kernel_equals_the_generated_numpy_evaluation(hip_ctx):
    """One step of 20 000 random states, inside and outside the stimulus window, GRL1 and forward Euler: <= 1e-11 relative
    (exp comes from different libms on the two sides); the kernel was compiled by the library at run time (beat_ode_jit_stats)."""
    import ctypes as C

    from beat import _hip
    from beat.models import from_ode

    lib = _hip.load()
    for scheme in ("generalized_rush_larsen", "forward_euler"):
        model = from_ode(SMALL, scheme=scheme)
        y = _states(model, 20_000, 5)
        p = model.init_parameter_values(stim_amplitude=30.0)
        for t in (0.2, 0.9):
            dev = model(states=y, t=t, parameters=p, dt=0.02)
            ref = model.numpy_step(y, t, p, 0.02)
            assert dev.shape == ref.shape and np.isfinite(dev).all()
            # (relative to the state before or after the step, whichever is larger: y + dt f may cancel)
            assert (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y)), 1e-12)).max() < 1e-11, (scheme, t)
        assert model.model_id >= 100
        ns, npar = C.c_int(), C.c_int()
        _hip.check(lib.beat_ode_model_info(model.model_id, C.byref(ns), C.byref(npar)))
        assert (ns.value, npar.value) == (5, 14)
    stats = (C.c_longlong * 4)()
    assert lib.beat_ode_jit_stats(stats) == 1 and stats[0] >= 2 and stats[3] == 0


def test_generated_model_takes_per_node_rows_classes_and_the_in_kernel_time_loop(hip_ctx):
    """What round 5 first left to the shipped models (VERDICT round 4 item 8's "every entry point"): (P, N) parameters of a
    generated model -- all rows read per node (a smooth field), or a class byte per node when the columns are few -- and
    `run` (beat_ode_run: nbeats x nsteps steps in one launch, tracked states), each against the NumPy evaluation."""
    from beat.models import from_ode
    from beat.odesolver import _DeviceODE

    model = from_ode(SMALL)
    n = 5000
    y = _states(model, n, 11)
    rng = np.random.default_rng(3)
    p = np.repeat(model.init_parameter_values(stim_amplitude=30.0)[:, None], n, axis=1)
    p[model.parameter_index("g_in")] *= rng.uniform(0.5, 1.5, n)  # a smooth (here: random) field in two conductances
    p[model.parameter_index("g_out")] *= rng.uniform(0.5, 1.5, n)
    dev = model(states=y, t=0.3, parameters=p, dt=0.02)
    ref = model.numpy_step(y, 0.3, p, 0.02)
    assert (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y)), 1e-12)).max() < 1e-11
    # the solver's routes: the same array through _DeviceODE (all rows: no sparse-row instance for a generated model), then a
    # piecewise-constant one (three parameter sets -> the class kernel)
    ode = _DeviceODE(hip_ctx, model, model.num_states, n, 0, p, __import__("beat").telemetry.NullMonitor())
    ode.set_initial(y)
    ode.step(0.3, 0.02)
    assert ode.classes is None and ode._sparse is None
    np.testing.assert_array_equal(ode.states.numpy(), dev)
    pc = np.repeat(model.init_parameter_values(stim_amplitude=30.0)[:, None], n, axis=1)
    pc[model.parameter_index("g_in"), n // 3:] *= 0.5
    pc[model.parameter_index("g_out"), 2 * n // 3:] = 0.0
    ode.parameters = pc
    ode.set_initial(y)
    ode.step(0.3, 0.02)
    assert ode.classes is not None and ode.classes[2] == 3
    refc = model.numpy_step(y, 0.3, pc, 0.02)
    got = ode.states.numpy()
    assert (np.abs(got - refc) / np.maximum(np.maximum(np.abs(refc), np.abs(y)), 1e-12)).max() < 1e-11
    # the in-kernel time loop: 2 beats x 150 steps with V and ca tracked every 10th step, uniform and per-node parameters
    p1 = model.init_parameter_values(stim_amplitude=30.0, stim_start=0.5, stim_duration=1.0)
    y0 = np.repeat(model.init_state_values()[:, None], 6, axis=1)
    y0[model.state_index("V")] += np.linspace(0.0, 5.0, 6)
    track = [model.state_index("V"), model.state_index("ca")]
    pn = np.repeat(p1[:, None], 6, axis=1)
    pn[model.parameter_index("g_out")] *= np.linspace(1.0, 1.1, 6)
    for params in (p1, pn):
        out, tr = model.run(y0, params, 0.02, 150, nbeats=2, t0=0.0, track_indices=track, save_freq=10)
        yy, rows = y0.copy(), []
        for _ in range(2):
            for j in range(150):
                if j % 10 == 0:
                    rows.append(yy[track].copy())
                yy = model.numpy_step(yy, 0.0 + j * 0.02, params, 0.02)
        assert tr.shape == (30, 2, 6)
        assert (np.abs(out - yy) / np.abs(yy).max(axis=1, keepdims=True)).max() < 1e-7  # (300 steps through an upstroke)
        rows = np.array(rows)  # (tracked through the upstroke, which amplifies the last-bit differences of the two exp()s: relative to the state's range)
        assert (np.abs(tr - rows) / np.abs(rows).max(axis=(0, 2), keepdims=True)).max() < 1e-7
        assert rows[:, 0].max() > 0.0  # it fired


def test_generated_model_as_cell_types_in_one_launch(hip_ctx):
    """DolfinMultiODESolver with ONE generated model behind three markers (parameter sets per layer, the shape of
    /root/reference/demos/biv_endocardial.py:124-173): one state array, a class byte per node, one launch per step
    (beat_ode_step_classes on the model compiled at run time) -- against the per-marker layout (BEAT_MULTI_ONE_LAUNCH=0), fused
    split steps on a slab, to 1e-9 after 30 steps."""
    import os

    import beat
    from beat import grid as g
    from beat.models import from_ode

    def build():
        model = from_ode(SMALL)  # (a fresh handle per build: two handles of one file share the registered model)
        mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([4.0, 2.0, 1.0])], [32, 16, 8])
        V = g.functionspace(mesh, ("P", 1))
        x = V.tabulate_dof_coordinates()
        markers = g.Function(V)
        markers.x.array[:] = np.where(x[:, 0] < 1.3, 0.0, np.where(x[:, 0] < 2.6, 1.0, 2.0))
        time = g.Constant(mesh, 0.0)
        cells = g.locate_entities(mesh, 3, lambda x: x[0] <= 0.5 + 1e-10)
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=1400.0 * beat.units.ureg("cm**-1"), time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, start=0.0, duration=1.5)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([9.5e-4, 2.5e-4, 2.5e-4]), I_s=I_s, C_m=0.01, dx=I_s.dZ,
                                   params={"petsc_options": {"ksp_rtol": 1e-12}})
        keys = (0, 1, 2)
        scale = {0: 1.0, 1: 0.7, 2: 1.4}
        ode = beat.odesolver.DolfinMultiODESolver(
            v_ode=g.Function(V), v_pde=pde.state, markers=markers, num_states={k: model.num_states for k in keys},
            fun={k: model for k in keys}, init_states={k: model.init_state_values() for k in keys},
            parameters={k: model.init_parameter_values(stim_amplitude=0.0, g_out=model.parameter_defaults["g_out"] * scale[k]) for k in keys},
            v_index={k: model.state_index("V") for k in keys})
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode), model

    a, model = build()
    assert a.ode._marked and a.ode._dev.model.model_id >= 100
    os.environ["BEAT_MULTI_ONE_LAUNCH"] = "0"
    try:
        b, _ = build()
    finally:
        del os.environ["BEAT_MULTI_ONE_LAUNCH"]
    assert not b.ode._marked
    t0, dt = 0.0, 0.05
    for _ in range(30):
        a.step((t0, t0 + dt))
        b.step((t0, t0 + dt))
        t0 = t0 + dt
    va, vb = np.asarray(a.pde.state.x.array), np.asarray(b.pde.state.x.array)
    assert va.max() > -40.0  # the stimulated end is on its upstroke
    assert np.abs(va - vb).max() < 1e-12 * np.abs(vb).max() * 1e3  # (1e-9 relative: two routes of the potential, same arithmetic per node)
    for k in (0, 1, 2):
        sa, sb = np.asarray(a.ode.values(k)), np.asarray(b.ode.values(k))
        assert sa.shape == sb.shape
        assert (np.abs(sa - sb) / np.maximum(np.abs(sb), 1e-9 * np.abs(sb).max(axis=1, keepdims=True))).max() < 1e-8


def test_generated_model_in_the_fused_split_step_stays_on_the_device(hip_ctx):
    """DolfinODESolver + MonodomainSplittingSolver with a generated model on a slab: the fused route (one ionic kernel with the
    previous solve's pending update, the solve in place on the V row, the solve left open for the next launch), `step` and the
    library's own loop (`solve`), against the same run with the model's NumPy evaluation as a plain Python ``fun`` (the
    reference's literal sequence on host arrays): potentials and every state to 1e-9 after 40 steps in which the stimulated
    corner fires."""
    import beat
    from beat import grid as g
    from beat.models import from_ode

    model = from_ode(SMALL)

    def build(fun):
        mesh = g.create_box(g.COMM_WORLD, [np.zeros(3), np.array([6.0, 3.0, 1.5])], [40, 20, 10])
        time = g.Constant(mesh, 0.0)
        cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 1.0 + 1e-10) & (x[1] <= 1.0 + 1e-10))
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        I_s = beat.stimulation.define_stimulus(mesh=mesh, chi=1400.0 * beat.units.ureg("cm**-1"), time=time, subdomain_data=tags, marker=1,
                                               mesh_unit="mm", amplitude=50_000.0, start=0.0, duration=1.5)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=np.diag([9.5e-4, 2.5e-4, 2.5e-4]), I_s=I_s, C_m=0.01, dx=I_s.dZ,
                                   params={"petsc_options": {"ksp_rtol": 1e-11}})
        ode = beat.odesolver.DolfinODESolver(v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state, fun=fun,
                                             init_states=model.init_state_values(), parameters=model.init_parameter_values(stim_amplitude=0.0),
                                             num_states=model.num_states, v_index=model.state_index("V"))
        return beat.MonodomainSplittingSolver(pde=pde, ode=ode)

    dt, nsteps = 0.05, 40
    a = build(model)
    assert a.ode.on_device and a._can_fuse()

    def host_fun(states, t, parameters, dt):  # a plain callable: the reference's route on host arrays
        return model.numpy_step(states, t, parameters, dt)

    b = build(host_fun)
    assert not b.ode.on_device
    va = vb = None
    ivs, t0 = [], 0.0  # (the intervals as solve() forms them: t1 = t0 + dt accumulated)
    for i in range(nsteps + 1):
        ivs.append((t0, t0 + dt))
        t0 = t0 + dt
    for i in range(nsteps):
        a.step(ivs[i])
        b.step(ivs[i])
        if i in (5, nsteps - 1):
            va, vb = np.asarray(a.ode.values).copy(), np.asarray(b.ode.values).copy()
            scale = np.maximum(np.abs(vb), 1e-6 * np.abs(vb).max(axis=1, keepdims=True))
            # six steps in: the two routes agree to the solver tolerance; after 40 -- the stimulated corner has fired, and an
            # upstroke amplifies any difference in its timing by orders of magnitude -- to 1e-5 (what the long trajectories of the
            # shipped models are held to against the oracle, too)
            assert (np.abs(va - vb) / scale).max() < (1e-10 if i == 5 else 1e-5), i
    assert a.pde._ops.open_x is None  # (ode.values finished the open solve)
    a.step(ivs[nsteps])
    assert a.pde._ops.open_x is not None  # the step leaves its solve open: nobody has asked for its result
    assert va[0].max() > 0.0  # the corner fired
    # the library's own step loop takes the generated model too (beat_split_steps_big through beat_ode_step_pending)
    c = build(model)
    assert c._can_batch(None)
    c.solve((0.0, nsteps * dt), dt)
    vc = np.asarray(c.ode.values)
    np.testing.assert_array_equal(vc, va)  # same kernels, same arguments as the step() loop


@pytest.mark.parametrize("emit", ["by_state", "global"])
def test_generated_kernel_of_a_big_model_with_spilled_registers(hip_ctx, emit, monkeypatch):
    """A user's big model does to the generator what the reference's ToR-ORd files do (45 / 52 states: 256 VGPRs + 256 AGPRs and
    1.8 KB of scratch per lane when generated): hundreds of temporaries alive at once, registers spilled.  tests/data/big_cell.ode
    (48 states, synthetic) in the order the generator emits by default (state by state, the potential last: 215 VGPRs, nothing
    spilled) and with every temporary ahead of every update (BEAT_ODE_EMIT=global: 256 + 256 registers, 450 B of scratch, 116
    spilled VGPRs on gfx950) through the step kernel -- uniform and per-node parameters, 8000 random states -- and through the
    in-kernel time loop, whose states live in registers across steps (round 1 saw a heavily spilled generated kernel go wrong
    exactly there): against the NumPy evaluation of the same expressions."""
    from beat.models import from_ode

    if emit == "global":
        monkeypatch.setenv("BEAT_ODE_EMIT", "global")
    model = from_ode(BIG)
    assert model.num_states == 48 and model.v_name == "V"
    rng = np.random.default_rng(17)
    n = 8000
    y = np.repeat(model.init_state_values()[:, None], n, axis=1)
    y[0] = rng.uniform(-95.0, 40.0, n)
    for k, name in enumerate(model.state_names):
        if name.startswith("x"):
            y[k] = rng.uniform(0.0, 1.0, n)
        elif name.startswith("c_"):
            y[k] *= rng.uniform(0.7, 1.4, n)
    p = model.init_parameter_values(stim_amplitude=30.0)
    for t in (0.3, 1.4):
        dev = model(states=y, t=t, parameters=p, dt=0.02)
        ref = model.numpy_step(y, t, p, 0.02)
        assert np.isfinite(dev).all()
        assert (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y)), 1e-12)).max() < 1e-11, t
    pn = np.repeat(p[:, None], n, axis=1)
    pn[model.parameter_index("g_3")] *= rng.uniform(0.5, 1.5, n)
    pn[model.parameter_index("k_5")] *= rng.uniform(0.5, 1.5, n)
    dev = model(states=y, t=1.4, parameters=pn, dt=0.02)
    ref = model.numpy_step(y, 1.4, pn, 0.02)
    assert (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y)), 1e-12)).max() < 1e-11
    # the in-kernel loop: 300 steps through the stimulus, V and one gate tracked
    y0 = y[:, :256].copy()
    track = [0, model.state_index("x4_1")]
    out, tr = model.run(y0, p, 0.02, 300, nbeats=1, t0=0.0, track_indices=track, save_freq=25)
    yy, rows = y0.copy(), []
    for j in range(300):
        if j % 25 == 0:
            rows.append(yy[track].copy())
        yy = model.numpy_step(yy, j * 0.02, p, 0.02)
    rows = np.array(rows)
    assert np.isfinite(out).all() and tr.shape == (12, 2, 256)
    assert (np.abs(out - yy) / np.abs(yy).max(axis=1, keepdims=True)).max() < 1e-8
    assert (np.abs(tr - rows) / np.abs(rows).max(axis=(0, 2), keepdims=True)).max() < 1e-8


def test_self_checks_catch_a_miscompiled_generated_kernel(hip_ctx, monkeypatch):
    """The generator's former output -- `c ? a : b` with the arms inline, every temporary ahead of every update -- makes hipcc
    (ROCm 7.2) build a heavily spilled kernel with divergent branches, ONE instance of which reloads registers under another lane
    mask than it spilled them under: at -O3 the per-node-rows instance is wrong on the nodes that take the other arm of a branch,
    the plain one right; at -O1 the plain one is wrong (tools/diag_spill.py, profiles/r05_generated_spills.md).  Where that still
    reproduces, the two self checks must refuse the instance LOUDLY: the library's cross-check of a variant instance against the
    plain one (BeatHipError at the first launch) and the registration's check of the plain instance against the NumPy evaluation
    (RuntimeError).  Where the compiler no longer does it, there is nothing to catch (skip)."""
    from beat import _hip
    from beat.models import from_ode

    monkeypatch.setenv("BEAT_ODE_BRANCHES", "1")
    monkeypatch.setenv("BEAT_ODE_EMIT", "global")

    def sample(model, n=4096):
        y = model._sample_states(n, seed=5)
        p = model.init_parameter_values(stim_amplitude=30.0)
        return y, p, np.repeat(p[:, None], n, axis=1)

    def wrong(dev, ref, y):
        return (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y)), 1e-12)).max() > 1e-8

    # is the miscompilation still there?  (checks off; a distinct model name per stage: the library checks an instance once)
    monkeypatch.setenv("BEAT_JIT_SELF_CHECK", "0")
    probe = from_ode(BIG, name="big_probe")
    y, p, pn = sample(probe)
    per_node_wrong = wrong(probe(states=y, t=1.4, parameters=pn, dt=0.02), probe.numpy_step(y, 1.4, pn, 0.02), y)
    monkeypatch.setenv("BEAT_JIT_EXTRA_FLAGS", "-O1")
    probe1 = from_ode(BIG, name="big_probe_o1")
    plain_wrong = wrong(probe1(states=y, t=1.4, parameters=p, dt=0.02), probe1.numpy_step(y, 1.4, p, 0.02), y)
    monkeypatch.delenv("BEAT_JIT_EXTRA_FLAGS")
    if not (per_node_wrong or plain_wrong):
        pytest.skip("this compiler does not miscompile the branchy form")
    monkeypatch.setenv("BEAT_JIT_SELF_CHECK", "1")
    if per_node_wrong:
        model = from_ode(BIG, name="big_checked")
        model.register()  # the plain instance passes its check against NumPy
        with pytest.raises(_hip.BeatHipError, match="differs from the model's plain instance"):
            model(states=y, t=1.4, parameters=pn, dt=0.02)
        np.testing.assert_allclose(model(states=y, t=1.4, parameters=p, dt=0.02), model.numpy_step(y, 1.4, p, 0.02), rtol=1e-9, atol=1e-12)
    if plain_wrong:
        monkeypatch.setenv("BEAT_JIT_EXTRA_FLAGS", "-O1")
        model = from_ode(BIG, name="big_checked_o1")
        with pytest.raises(RuntimeError, match="differs from the NumPy evaluation"):
            model.register()
        # a caller that catches the error and asks again gets the check again, not the id of the wrong kernel
        assert model._registered is None and model.model_id == -1
        with pytest.raises(RuntimeError, match="differs from the NumPy evaluation"):
            model.register()


MONITOR_BOUND = 1e-11  # what tests/test_monitor_gpu.py holds a monitored value to, relative to its row's scale


@pytest.mark.parametrize("n", [1, 9, 1025])
def test_first_launches_of_the_variant_instances_at_the_edges_of_the_check(hip_ctx, n):
    """The library holds a variant instance against the plain one at its FIRST launch, on min(n, 1024) nodes and with scratch it
    lays out itself: two result blocks, per-node rows, a class table and a marker byte per node behind it.  Its edges: one node; 9
    (marker bytes that do not fill a double); 1025 (more nodes than the check takes, a second block).  A model name of its own per
    n, so that each case IS the first launch of its four variant instances -- per-node step, class step, per-node monitor, class
    monitor: none may be refused, each gives the NumPy evaluation's values, and the monitors leave the state array as it was."""
    import ctypes as C

    import beat
    from beat._device import StateArray
    from beat.models import from_ode
    from beat.odesolver import _DeviceODE

    model = from_ode(SMALL, name=f"small_first_launch_{n}")
    names = list(model.monitor_names)
    y = _states(model, n, 21)
    t, dt = 1.0, 0.02  # (inside the stimulus window)
    sets = [model.init_parameter_values(stim_amplitude=30.0), model.init_parameter_values(stim_amplitude=12.0, g_in=7.0, v_pump=0.03)]
    marks = (np.arange(n) % 2).astype(np.uint8)
    p_class = np.stack([sets[m] for m in marks], axis=1)
    p_node = np.repeat(sets[0][:, None], n, axis=1)
    p_node[model.parameter_index("g_in")] *= np.linspace(0.5, 1.5, n)

    def step_error(dev, ref, y0):
        assert dev.shape == ref.shape and np.isfinite(dev).all()
        return (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y0)), 1e-12)).max()

    def monitor_error(dev, ref):
        assert dev.shape == ref.shape and np.isfinite(ref).all() and np.isfinite(dev).all()
        return (np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(ref).max(axis=1, keepdims=True)), 1e-300)).max()

    err = step_error(model(states=y, t=t, parameters=p_node, dt=dt), model.numpy_step(y, t, p_node, dt), y)
    print(f"n={n}: per-node step {err:.3e}")
    assert err < 1e-11
    ode = _DeviceODE(hip_ctx, model, model.num_states, n, 0, None, beat.telemetry.NullMonitor())
    ode.set_initial(y)
    ode.explicit_classes = True
    ode.set_classes(hip_ctx.from_numpy(marks), sets)
    ode.step(t, dt, v_index=model.state_index("V"))
    y1 = ode.states.numpy()
    err = step_error(y1, model.numpy_step(y, t, p_class, dt), y)
    print(f"n={n}: class step {err:.3e}")
    assert err < 1e-11
    # the monitors on the resident array, every byte of which (padding included) must stay what it is
    before = ode.states.buf.cpu().numpy().tobytes()
    out = StateArray(hip_ctx, len(names), n)
    rows = hip_ctx.from_numpy(np.ascontiguousarray(p_node))
    model.monitor_on_device(hip_ctx, names, ode.states.ptr, n, ode.states.ld, t, out.ptr, out.ld, per_node=(C.c_void_p(rows.data_ptr()), n))
    hip_ctx.synchronize()
    err = monitor_error(out.numpy(), model.numpy_monitor(y1, t, p_node))
    print(f"n={n}: per-node monitor {err:.3e}")
    assert err <= MONITOR_BOUND
    ode.monitor_rows(names, t, out.ptr, out.ld)
    hip_ctx.synchronize()
    err = monitor_error(out.numpy(), model.numpy_monitor(y1, t, p_class))
    print(f"n={n}: class monitor {err:.3e}")
    assert err <= MONITOR_BOUND
    assert ode.states.buf.cpu().numpy().tobytes() == before


def test_registration_hands_out_no_id_until_the_self_check_has_passed(hip_ctx, monkeypatch):
    """``register()`` used to set the id before ``_self_check()`` ran, so a second call after a failed check returned
    the id of a kernel known to be wrong.  With a check made to fail once: no id, the check runs again at the next call, and only
    then is the model usable; the source went to the library once."""
    from beat.models import from_ode
    from beat.models.ode_file import OdeFileModel

    model = from_ode(SMALL, name="small_retry")
    calls = []
    real = OdeFileModel._self_check

    def flaky(self):
        calls.append(self.model_id)
        if len(calls) == 1:
            raise RuntimeError("made to fail")
        return real(self)

    monkeypatch.setattr(OdeFileModel, "_self_check", flaky)
    with pytest.raises(RuntimeError, match="made to fail"):
        model.register()
    assert model._registered is None and model.model_id == -1 and model._library_id is not None
    first = model._library_id
    mid = model.register()
    assert mid == first == model.model_id and len(calls) == 2 and calls[0] == calls[1] == first
    assert model.register() == mid and len(calls) == 2  # verified: not checked a third time
    y = _states(model, 256, 1)
    p = model.init_parameter_values()
    np.testing.assert_allclose(model(states=y, t=0.0, parameters=p, dt=0.02), model.numpy_step(y, 0.0, p, 0.02), rtol=1e-10, atol=1e-300)


def test_generated_exp_keeps_nan_and_overflow(hip_ctx, tmp_path):
    """the generated step's ``exp`` clamps its argument into the range the table-driven routine takes
    (fmin(fmax(x, -745), 709)) -- which turned a NaN argument into exp(-745) ~ 0 and an overflowing one into 8e307, where NumPy
    (the reference's way of evaluating ``fun``) gives NaN and inf: a cell that has diverged must stay visibly diverged.  Forward
    Euler on  dx/dt = exp(a x) - 1  with x in {finite, > 709.78, < -745, NaN, +inf, -inf}."""
    from beat.models import from_ode

    f = tmp_path / "expo.ode"
    f.write_text('parameters("P", a = 1.0)\nstates("S", x = 0.5, y = 0.25)\nexpressions("S")\n'
                 'dx_dt = exp(a*x) - 1\ndy_dt = -y*exp(-a*x)\n')
    for scheme in ("forward_euler", "generalized_rush_larsen"):
        model = from_ode(f, name=f"expo_{scheme}", scheme=scheme, v_name="x")
        x = np.array([0.5, -3.0, 709.0, 709.9, 800.0, -744.0, -800.0, np.nan, np.inf, -np.inf, 1e-3, 30.0])
        y = np.vstack([x, np.full_like(x, 0.25)])
        p = model.init_parameter_values()
        dev = model(states=y, t=0.0, parameters=p, dt=0.01)
        with np.errstate(all="ignore"):
            ref = model.numpy_step(y, 0.0, p, 0.01)
        np.testing.assert_array_equal(np.isnan(dev), np.isnan(ref))
        np.testing.assert_array_equal(np.isposinf(dev), np.isposinf(ref))
        np.testing.assert_array_equal(np.isneginf(dev), np.isneginf(ref))
        ok = np.isfinite(ref)
        np.testing.assert_allclose(dev[ok], ref[ok], rtol=1e-10, atol=1e-300)
        assert np.isnan(dev[0, 7]) and (scheme != "forward_euler" or np.isposinf(dev[0, 4]))
