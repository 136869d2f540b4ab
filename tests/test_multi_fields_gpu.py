"""State rows of DolfinMultiODESolver as functions of the grid, through the public API, in every layout the solver keeps its states
in: one array over the grid (BEAT_MULTI_COMPACT=0), one compact array (=1), one array per marker (BEAT_MULTI_ONE_LAUNCH=0), two
different models behind two markers, and a masked box (compact by default).  The reference is always the array assembled on the
host from ``values(marker)`` and ``_inds[marker]``; all values are copies, so every comparison is exact."""
import os
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
DT = 0.05
LAYOUTS = ("grid", "compact", "per_marker", "two_models", "masked")
ENV = {"grid": {"BEAT_MULTI_COMPACT": "0"}, "compact": {"BEAT_MULTI_COMPACT": "1"}, "per_marker": {"BEAT_MULTI_ONE_LAUNCH": "0"}}


def _build(layout, host_callable=False):
    """A split solver on a 41 x 21 x 13-node slab (no one-launch solve: the potential's last update is deferred), stimulated in a
    corner; three TP06 cell types by thirds along x with a tenth of the nodes under a marker that has no model -- or TP06 and the
    generated small_cell model behind two markers, or a masked box."""
    import beat
    from beat import grid as g
    from beat.models import from_ode, tp06

    saved = {k: os.environ.get(k) for k in ("BEAT_MULTI_COMPACT", "BEAT_MULTI_ONE_LAUNCH")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(ENV.get(layout, {}))
    try:
        if layout == "masked":
            mask = np.ones((12, 20, 40), dtype=bool)  # (cz, cy, cx)
            mask[:, 6:14, 12:30] = False
            mask[8:, :, :10] = False
            mesh = g.create_voxel_mesh(g.COMM_WORLD, mask, 0.05)
        else:
            mesh = g.create_box(g.COMM_WORLD, [(0.0, 0.0, 0.0), (2.0, 1.0, 0.6)], (40, 20, 12))
        time = g.Constant(mesh, 0.0)
        cells = g.locate_entities(mesh, 3, lambda x: (x[0] <= 0.3) & (x[1] <= 0.3))
        tags = g.meshtags(mesh, 3, cells, np.full(len(cells), 1, dtype=np.int32))
        dx = g.Measure("dx", domain=mesh, subdomain_data=tags)
        stim = g.conditional(g.And(g.ge(time, 0.0), g.le(time, 1.0)), 1.0, 0.0)  # (C_m = 0.01: 100 mV/ms)
        pde = beat.MonodomainModel(time=time, mesh=mesh, M=0.001, I_s=beat.Stimulus(expr=stim, dZ=dx, marker=1), dx=dx, C_m=0.01)
        V = g.functionspace(mesh, ("P", 1))
        x = mesh.node_coordinates(pad3=True)[:, 0]
        n = x.size
        rng = np.random.default_rng(3)
        if layout == "two_models":
            models = {0: tp06.generalized_rush_larsen, 1: from_ode(SMALL)}
            marker_arr = np.where(x < 1.0, 0.0, 1.0)
        else:
            models = {k: tp06.generalized_rush_larsen for k in (0, 1, 2)}
            marker_arr = np.minimum(np.floor(x * 3 / 2.0), 2.0)
        marker_arr[rng.random(n) < 0.1] = 9.0  # tissue without a cell model
        if layout == "masked":
            marker_arr[~mesh.node_active()] = -1.0
        markers = g.Function(V)
        markers.x.array[:] = marker_arr
        init, params = {}, {}
        for k, m in models.items():
            nk = int((marker_arr == k).sum())
            init[k] = np.repeat(np.asarray(m.init_state_values())[:, None], nk, axis=1) * (1.0 - 0.01 * rng.random((m.num_states, nk)))
            params[k] = m.init_parameter_values(stim_amplitude=0.0) if m is tp06.generalized_rush_larsen else m.init_parameter_values()
        fun = models
        if host_callable:
            fun = {k: (lambda states, t, parameters, dt: states) for k in models}
        ode = beat.odesolver.DolfinMultiODESolver(
            v_ode=g.Function(V), v_pde=pde.state, markers=markers, num_states={k: m.num_states for k, m in models.items()}, fun=fun,
            init_states=init, parameters=params, v_index={k: m.state_index("V") for k, m in models.items()})
        solver = beat.MonodomainSplittingSolver(pde=pde, ode=ode)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    if not host_callable:
        marked, compact = ode._marked, ode._marked and ode._node_idx is not None
        assert (marked, compact) == {"grid": (True, False), "compact": (True, True), "per_marker": (False, False),
                                     "two_models": (False, False), "masked": (True, True)}[layout]
    return solver


def _steps(solver, k0, count):
    for k in range(k0, k0 + count):
        solver.step((k * DT, (k + 1) * DT))


NSTEPS = 6


def _stepped(layout):
    """A solver of its own for every test, after NSTEPS split steps: met as a step leaves it."""
    solver = _build(layout)
    _steps(solver, 0, NSTEPS)
    if solver.ode._marked:  # the fused step: the solve is open or its last update pending on the potential row
        d = solver.pde._ops.deferred
        assert d.open_x is not None or d.pending is not None
    return solver


def _assembly(ode, key, prior):
    """The array the reference's loop assembles on the host: arr[inds[marker]] = values(marker)[row]."""
    arr = np.array(prior, dtype=np.float64)
    rows = ode._key_rows(key)
    for m, r in zip(ode._marker_values, rows):
        arr[ode._inds[m]] = ode.values(m)[r]
    return arr


def _other_name(ode):
    return "h" if len({f.name for f in ode.fun.values()}) > 1 else "Ca_i"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_states_to_functions(layout):
    from beat import grid as g

    solver = _stepped(layout)
    ode = solver.ode
    V = ode.v_ode.function_space
    n = ode.markers.x.array.size
    keys = ["V", _other_name(ode), 3, {m: ("V" if j == 0 else 1) for j, m in enumerate(ode._marker_values)}]
    prior = np.random.default_rng(8).standard_normal((len(keys), n))
    out = [g.Function(V) for _ in keys]
    for f, p in zip(out, prior):
        f.x.array[:] = p
    got = ode.states_to_functions(keys, out)  # right behind the step: the potential row is not complete yet
    assert got is out
    got = [np.array(f.x.array) for f in out]
    marked = np.zeros(n, dtype=bool)
    for m in ode._marker_values:
        marked |= ode._inds[m]
    assert 0 < (~marked).sum() < n
    for k, key in enumerate(keys):
        want = _assembly(ode, key, prior[k])
        assert got[k].tobytes() == want.tobytes(), key
        assert np.isfinite(want).all() and (want[marked] != prior[k][marked]).all()
    if layout == "two_models":  # "V" is a different row in each model
        assert len(set(ode._key_rows("V"))) == 2
    # outside = -1.0; new functions; the one-key form
    new = ode.states_to_functions(keys[:2], outside=-1.0)
    for k, f in enumerate(new):
        assert np.array(f.x.array).tobytes() == _assembly(ode, keys[k], np.full(n, -1.0)).tobytes()
    f = g.Function(V)
    f.x.array[:] = prior[2]
    assert ode.state_to_function(3, f) is f and np.array(f.x.array).tobytes() == _assembly(ode, 3, prior[2]).tobytes()
    assert np.array(ode.state_to_function("V", f, outside=7.0).x.array).tobytes() == _assembly(ode, "V", np.full(n, 7.0)).tobytes()
    # more than 8 keys go in chunks
    if layout == "grid":
        many = ode.states_to_functions(list(range(11)), outside=0.5)
        for r, f in enumerate(many):
            assert np.array(f.x.array).tobytes() == _assembly(ode, r, np.full(n, 0.5)).tobytes()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_states_to_dolfin(layout):
    solver = _stepped(layout)
    ode = solver.ode
    n = ode.markers.x.array.size
    if layout == "two_models":  # (the reference's loop takes the first marker's number of states: the second model has fewer)
        with pytest.raises(IndexError):
            ode.states_to_dolfin()
        return
    functions = ode.states_to_dolfin()
    assert len(functions) == 19
    for r, f in enumerate(functions):
        assert np.array(f.x.array).tobytes() == _assembly(ode, r, np.zeros(n)).tobytes()
    prior = np.random.default_rng(9).standard_normal(n)
    for f in functions:
        f.x.array[:] = prior
    ode.assign_all_states(functions)  # nodes without a marker keep what the functions held
    for r, f in enumerate(functions):
        assert np.array(f.x.array).tobytes() == _assembly(ode, r, prior).tobytes()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_function_to_state(layout):
    """Right after a split step: what is written comes back through values(marker), nothing else changes, and the next step equals
    the step of a solver given the same states through set_values."""
    from beat import grid as g

    a, b = _build(layout), _build(layout)
    _steps(a, 0, 2)
    _steps(b, 0, 2)
    ode = a.ode
    V = ode.v_ode.function_space
    n = ode.markers.x.array.size
    _steps(a, 2, 1)
    _steps(b, 2, 1)
    before = {m: b.ode.values(m).copy() for m in ode._marker_values}
    rng = np.random.default_rng(10)
    written = {}
    for key, lo, hi in (("V", -80.0, -60.0), ("m", 0.0, 0.2)):
        src = g.Function(V)
        vals = rng.uniform(lo, hi, n)
        src.x.array[:] = vals
        ode.function_to_state(key, src)
        written[key] = vals
    for m, rv, rm in zip(ode._marker_values, ode._key_rows("V"), ode._key_rows("m")):
        want = before[m].copy()
        want[rv] = written["V"][ode._inds[m]]
        want[rm] = written["m"][ode._inds[m]]
        assert ode.values(m).tobytes() == want.tobytes()
        b.ode.set_values(m, want)
    # the potential function shows the written values on the marked nodes, the old ones elsewhere
    ode.to_dolfin()
    b.ode.to_dolfin()
    assert np.array(ode.v_ode.x.array).tobytes() == np.array(b.ode.v_ode.x.array).tobytes()
    _steps(a, 3, 1)
    _steps(b, 3, 1)
    for m in ode._marker_values:
        assert ode.values(m).tobytes() == b.ode.values(m).tobytes() and np.isfinite(ode.values(m)).all()
    assert np.array(a.pde.state.x.array).tobytes() == np.array(b.pde.state.x.array).tobytes()
    # the potential function itself as the source (it aliases the row after a step)
    ode.function_to_state("V", a.pde.state)
    for m in ode._marker_values:
        assert ode.values(m).tobytes() == b.ode.values(m).tobytes()
    # a key per marker: the potential of the first marker, row 1 of the others.  In the compact layout the potential's home is
    # a field of the grid and such a key is refused; elsewhere it is written and comes back
    key = {m: ("V" if j == 0 else 1) for j, m in enumerate(ode._marker_values)}
    src = g.Function(V)
    vals = rng.uniform(-70.0, -65.0, n)
    src.x.array[:] = vals
    if layout in ("compact", "masked"):
        with pytest.raises(NotImplementedError, match="compact"):
            ode.function_to_state(key, src)
    else:
        kept = {m: ode.values(m).copy() for m in ode._marker_values}
        ode.function_to_state(key, src)
        for m, r in zip(ode._marker_values, ode._key_rows(key)):
            kept[m][r] = vals[ode._inds[m]]
            assert ode.values(m).tobytes() == kept[m].tobytes()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_field_writer(layout, tmp_path):
    import beat

    solver = _stepped(layout)
    ode = solver.ode
    mesh = ode.v_ode.function_space.mesh
    n = ode.markers.x.array.size
    shape = tuple(reversed(mesh.shape_global))
    other = _other_name(ode)
    with beat.FieldWriter(tmp_path / "full", {"v": (ode, "V"), "s": (ode, other)}, stride=1, dtype="float64", format="npy",
                          outside=-3.0) as w64, \
         beat.FieldWriter(tmp_path / "half", {"v": (ode, "V"), "s": (ode, other), "k": (ode, 2)}, stride=2, dtype="float32",
                          format="npy") as w32:
        w64.write(0.0)  # right behind the step
        w32.write(0.0)
        _steps(solver, NSTEPS, 1)
        w64.write(1.0)
    active = mesh.node_active() if mesh.active is not None else np.ones(n, dtype=bool)
    for name, key in (("v", "V"), ("s", other)):
        want = _assembly(ode, key, np.full(n, -3.0))
        want[~active] = -3.0
        got = np.load(tmp_path / "full" / f"{name}_1.npy")
        assert got.dtype == np.float64 and got.tobytes() == want.reshape(shape).tobytes()
        assert np.load(tmp_path / "full" / f"{name}_0.npy").tobytes() != got.tobytes()
    assert (tmp_path / "half" / "k_0.npy").is_file()
    # fp32 at stride 2, NaN outside: against a writer-free assembly of the same moment
    with beat.FieldWriter(tmp_path / "half2", {"v": (ode, "V"), "s": (ode, other)}, stride=2, dtype="float32", format="npy") as w:
        w.write(2.0)
    for name, key in (("v", "V"), ("s", other)):
        want = _assembly(ode, key, np.full(n, np.nan))
        want[~active] = np.nan
        want = np.float32(want.reshape(shape)[::2, ::2, ::2])
        got = np.load(tmp_path / "half2" / f"{name}_0.npy")
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    # a tissue node without a cell model holds NaN: it counts as non-finite
    t, stats = w.frames[0]
    no_model = active.copy()
    for m in ode._marker_values:
        no_model &= ~ode._inds[m]
    assert stats["v"][2] == no_model.sum() > 0


def test_errors(tmp_path):
    import beat
    from beat import grid as g

    solver = _stepped("two_models")
    ode = solver.ode
    V = ode.v_ode.function_space
    with pytest.raises(ValueError, match="marker 1.*small_cell.*Ca_i"):  # a name one model lacks
        ode.states_to_functions(["Ca_i"])
    with pytest.raises(IndexError, match="marker 1"):  # an int beyond a model's states
        ode.states_to_functions([7])
    with pytest.raises(IndexError):
        ode.function_to_state(7, g.Function(V))
    with pytest.raises(ValueError):
        ode.states_to_functions([{0: "V"}])  # a dict names every marker
    with pytest.raises(ValueError):
        ode.states_to_functions(["V", "m"], [g.Function(V)])
    with pytest.raises(ValueError, match="Ca_i"):
        beat.FieldWriter(tmp_path / "w", {"c": (ode, "Ca_i")}, format="npy")
    with pytest.raises(ValueError):
        beat.FieldWriter(tmp_path / "w", {"c": (ode, 7)}, format="npy")
    with pytest.raises(ValueError, match="1..8"):  # 9 keys to a writer
        beat.FieldWriter(tmp_path / "w", {f"f{k}": (ode, "V") for k in range(9)}, format="npy")
    host = _build("per_marker", host_callable=True).ode
    assert not host.on_device
    with pytest.raises(NotImplementedError, match="host callable"):
        host.states_to_functions(["V"])
    with pytest.raises(NotImplementedError, match="host callable"):
        host.function_to_state("V", g.Function(V))
    with pytest.raises(NotImplementedError, match="host callable"):
        beat.FieldWriter(tmp_path / "w", {"v": (host, 0)}, format="npy")
    assert not (tmp_path / "w").exists()


def test_demo_runs_at_a_reduced_size(tmp_path):
    import subprocess
    import sys

    run = subprocess.run([sys.executable, str(ROOT / "demos" / "multi_state_output.py"), "--lx", "4", "--ly", "2", "--lz", "1.5", "--dx", "0.25",
                          "--T", "2", "--out", str(tmp_path / "frames")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "restarted" in run.stdout and (tmp_path / "frames" / "Ca_i_1.npy").is_file()
