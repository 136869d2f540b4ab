"""beat.FieldWriter on a split solver: frames written behind ``solve(..., recorder=[w])`` against a second, identical solver whose
potential the test reads on the host at the same steps (what ``beat.io.write_function`` does), on a slab large enough for the
deferred update of the potential and on a voxel mesh with a hole; state rows, event maps, the writer's thread and the demo."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from _vti import read_pvd, read_vti

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DT, NSTEPS, EVERY = 0.01, 30, 5


def _fhn_solver(mesh):
    """demos/fitzhughnagumo.py on ``mesh``: stimulus in the low corner for 0.5 ms, forward-Euler ionic step, Godunov splitting."""
    import beat
    from beat import grid as g

    time = g.Constant(mesh, 0.0)
    parameters = np.array([0.26, 0.1, 1.0, 0.13, 0.013, 125.0, -85.0, 40.0, 0.0, 1.0, 0.0])
    stim = g.conditional(g.And(g.ge(time, 0.0), g.le(time, 0.5)), 600.0, 0.0)
    dim = mesh.topology.dim
    cells = g.locate_entities(mesh, dim, lambda x: (x[0] <= 0.5) & (x[1] <= 0.5))
    tags = g.meshtags(mesh, dim, cells, np.full(len(cells), 1, dtype=np.int32))
    dx = g.Measure("dx", domain=mesh, subdomain_data=tags)
    pde = beat.MonodomainModel(time=time, mesh=mesh, M=0.001, I_s=beat.Stimulus(expr=stim, dZ=dx, marker=1), dx=dx)
    ode = beat.odesolver.DolfinODESolver(
        v_ode=g.Function(g.functionspace(mesh, ("P", 1))), v_pde=pde.state, fun=beat.models.fhn.forward_euler_readme,
        init_states=np.array([0.0, -85.0]), parameters=parameters, num_states=2, v_index=1)
    return beat.MonodomainSplittingSolver(pde=pde, ode=ode)


def _slab():
    from beat import grid as g

    return g.create_box(g.COMM_WORLD, [(0.0, 0.0, 0.0), (2.0, 1.0, 0.6)], (40, 20, 12))  # 41 x 21 x 13 nodes: no one-launch solve


def _holed():
    from beat import grid as g

    mask = np.ones((6, 12, 20), dtype=bool)  # (cz, cy, cx)
    mask[:, 4:9, 8:14] = False  # a hole through the slab: the nodes strictly inside it touch no tissue
    return g.create_voxel_mesh(g.COMM_WORLD, mask, 0.05)


MESHES = {"slab": _slab, "voxels_with_a_hole": _holed}


def _steps():
    """The steps MonodomainSplittingSolver.solve((0, NSTEPS * DT), DT) makes (it adds dt up; k * dt differs in the last bit)."""
    steps, t0, t1 = [], 0.0, DT
    while t1 < NSTEPS * DT + 1e-12:
        steps.append((t0, t1))
        t0 = t1
        t1 = t0 + DT
    assert len(steps) == NSTEPS
    return steps


def _host_frames(solver):
    """The second solver: step, and at every EVERY-th step read the potential on the host."""
    frames = []
    for k, iv in enumerate(_steps()):
        solver.step(iv)
        if (k + 1) % EVERY == 0:
            frames.append(np.array(solver.pde.state.x.array))
    return frames


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("kind", list(MESHES))
@pytest.mark.parametrize("format", ["npy", "vti"])
def test_frames_equal_the_potential_read_on_the_host(tmp_path, kind, format):
    """stride 1 / fp64: every frame is the potential of the second solver bit for bit (NaN outside the tissue), the statistics are
    NumPy's over the tissue nodes, the final potentials and states of the two runs are equal, and a writer alone in ``recorder``
    does not reach for the probe recorder's fields (_can_batch)."""
    import beat

    a, b = _fhn_solver(MESHES[kind]()), _fhn_solver(MESHES[kind]())
    mesh = a.pde.state.function_space.mesh
    active = mesh.node_active()
    assert (kind == "slab") == bool(active.all()) and (kind == "slab") == (not a.pde._ops.small_active() and not a.pde._ops.per_node)
    path = tmp_path / "run"
    w = beat.FieldWriter(path, {"v": a.pde.state}, stride=1, dtype="float64", format=format, time=a.pde.time, every=EVERY)
    assert not a._can_batch(w)
    a.solve((0.0, NSTEPS * DT), DT, recorder=[w])
    w.close()
    w.close()
    want = _host_frames(b)
    nx, ny, nz = mesh.shape_global
    assert len(w.frames) == len(want) == NSTEPS // EVERY and w.shape == (nz, ny, nx)
    if format == "npy":
        index = json.loads((path / "index.json").read_text())
        times = index["times"]
        got = [np.load(path / f["v"]) for f in index["files"]]
        assert index["stride"] == [1, 1, 1] and index["origin"] == list(mesh.lower) and index["spacing"] == list(mesh.h)
    else:
        entries = read_pvd(tmp_path / "run.pvd")
        times = [t for t, _ in entries]
        files = [read_vti(tmp_path / name) for _, name in entries]
        got = [f.arrays["v"] for f in files]
        assert files[0].extent == [0, nx - 1, 0, ny - 1, 0, nz - 1] and files[0].spacing == list(mesh.h)
    # t = float(pde.time) after the step: the PDE's theta = 0.5 into the step
    assert np.allclose(times, [t0 + 0.5 * (t1 - t0) for t0, t1 in _steps()[EVERY - 1::EVERY]], rtol=0, atol=1e-12)
    assert [t for t, _ in w.frames] == times
    for k, (frame, host) in enumerate(zip(got, want)):
        assert _same_bits(np.asarray(frame, dtype=np.float64).ravel(), np.where(active, host, np.nan)), k
        mn, mx, bad = w.frames[k][1]["v"]
        assert (mn, mx, bad) == (host[active].min(), host[active].max(), 0), k
    assert want[-1][active].max() > want[-1][active].min()  # (the stimulus has moved the potential)
    assert _same_bits(np.array(a.pde.state.x.array), np.array(b.pde.state.x.array))
    assert _same_bits(np.ascontiguousarray(a.ode.values), np.ascontiguousarray(b.ode.values))


def test_state_rows_event_map_stride_and_box(tmp_path):
    """A state row given as (ode, name) and as (ode, index) equals ``ode.values[k]``; an event map is a field like any other;
    stride, box and fp32 give the NumPy slice of the same arrays, with origin and spacing to match."""
    import beat

    a = _fhn_solver(_slab())
    mesh = a.pde.state.function_space.mesh
    nx, ny, nz = mesh.shape_global
    rec = beat.EventRecorder(a.pde.state, -84.0, maps=("activation",))  # (1 mV above rest: the stimulated corner crosses it at once)
    s_name = a.ode.fun.state_names[0]
    assert a.ode.v_index == 1 and a.ode.fun.state_names[1] != s_name
    box = [(1, 40), (0, 21), (2, 11)]
    with beat.FieldWriter(tmp_path / "sub" / "run", {"v": (a.ode, 1), "s": (a.ode, s_name), "act": rec.activation}, stride=(3, 2, 4),
                          dtype="float32", box=box, time=lambda: 7.5, every=NSTEPS) as w:
        a.solve((0.0, NSTEPS * DT), DT, recorder=[rec, w])
    assert len(w.frames) == 1 and w.frames[0][0] == 7.5
    (t, name), = read_pvd(tmp_path / "sub" / "run.pvd")
    got = read_vti(tmp_path / "sub" / name)
    values = a.ode.values
    act = np.asarray(rec.activation.x.array)
    assert np.isfinite(act).any() and np.isnan(act).any()
    sl = (slice(2, 11, 4), slice(0, 21, 2), slice(1, 40, 3))
    for key, full in (("v", values[1]), ("s", values[0]), ("act", act)):
        want = full.reshape(nz, ny, nx)[sl].astype(np.float32)
        assert np.array_equal(got.arrays[key].view(np.uint32), want.view(np.uint32)), key
    assert list(got.arrays) == ["v", "s", "act"] and got.scalars == "v"
    assert got.extent == [0, 12, 0, 10, 0, 2]
    assert np.allclose(got.origin, [1 * mesh.h[0], 0.0, 2 * mesh.h[2]], rtol=0, atol=1e-15)
    assert np.allclose(got.spacing, [3 * mesh.h[0], 2 * mesh.h[1], 4 * mesh.h[2]], rtol=0, atol=1e-15)
    # the statistics cover the whole box; NaN (not yet activated) is counted and ignored
    inbox = act.reshape(nz, ny, nx)[2:11, 0:21, 1:40]
    assert w.frames[0][1]["act"] == (np.nanmin(inbox), np.nanmax(inbox), int(np.isnan(inbox).sum()))
    vbox = values[1].reshape(nz, ny, nx)[2:11, 0:21, 1:40]
    assert w.frames[0][1]["v"] == (vbox.min(), vbox.max(), 0)


def test_what_is_not_a_field_is_refused(tmp_path):
    import beat
    from beat import grid as g

    mesh = g.create_unit_square(g.COMM_WORLD, 8, 8, g.CellType.triangle)
    other = g.create_unit_square(g.COMM_WORLD, 8, 8, g.CellType.triangle)
    p1 = g.Function(g.functionspace(mesh, ("P", 1)))
    for bad in (g.Function(g.functionspace(mesh, ("P", 2))), g.Function(g.functionspace(mesh, ("DG", 1))),
                g.Function(g.functionspace(mesh, ("DG", 0))), g.Function(g.VectorFunctionSpace(mesh, 2))):
        with pytest.raises(NotImplementedError):
            beat.FieldWriter(tmp_path / "x", {"f": bad})
    with pytest.raises(ValueError):
        beat.FieldWriter(tmp_path / "x", {"a": p1, "b": g.Function(g.functionspace(other, ("P", 1)))})
    a = _fhn_solver(mesh)
    for bad in ((a.ode, "no_such_state"), (a.ode, 2), (a.ode, -1)):
        with pytest.raises(ValueError):
            beat.FieldWriter(tmp_path / "x", {"f": bad})
    for kw in (dict(stride=0), dict(stride=(1, 1, 1)), dict(box=[(0, 10), (0, 9)]), dict(box=[(0, 9)])):
        with pytest.raises(ValueError):
            beat.FieldWriter(tmp_path / "x", {"f": p1}, **kw)
    assert not list(tmp_path.iterdir())
    with beat.FieldWriter(tmp_path / "x", {"f": p1}) as w:  # 2-D, and a run without frames
        assert w.shape == (9, 9)
    with pytest.raises(ValueError):
        w.write(0.0)  # closed


def test_an_exception_in_the_writer_thread_comes_back(tmp_path):
    """The directory of the files cannot be made (a regular file is in the way): the thread's exception is raised by close() -- or by
    a write() that finds it first -- once the frame has been taken out of its slot; a second close() is quiet."""
    import beat
    from beat import grid as g

    (tmp_path / "in_the_way").write_text("a file")
    mesh = g.create_unit_square(g.COMM_WORLD, 8, 8, g.CellType.triangle)
    f = g.Function(g.functionspace(mesh, ("P", 1)))
    f.interpolate(lambda x: x[0] + 2.0 * x[1])
    w = beat.FieldWriter(tmp_path / "in_the_way" / "sub" / "run", {"f": f}, depth=2)
    w.write(0.0)
    with pytest.raises(OSError):
        w.close()
    w.close()
    assert w.frames == []
    w = beat.FieldWriter(tmp_path / "in_the_way" / "sub" / "run", {"f": f}, depth=1)
    w.write(0.0)
    with pytest.raises(OSError):
        w.write(1.0)  # (one slot: this write has waited for the first frame to leave it, and knows what became of it)
    with pytest.raises(OSError):
        w.close()
    w.close()
    assert w.frames == []


def test_back_pressure_keeps_every_frame(tmp_path):
    """More frames than slots, enqueued back to back: write() waits for the oldest slot, nothing is lost or reordered."""
    import beat
    from beat import grid as g

    mesh = g.create_unit_square(g.COMM_WORLD, 16, 16, g.CellType.triangle)
    f = g.Function(g.functionspace(mesh, ("P", 1)))
    with beat.FieldWriter(tmp_path / "frames", {"f": f}, dtype="float64", format="npy", depth=2) as w:
        for k in range(7):
            f.interpolate(lambda x, k=k: x[0] + k)
            w.write(float(k))
    index = json.loads((tmp_path / "frames" / "index.json").read_text())
    assert index["times"] == [float(k) for k in range(7)]
    x = np.linspace(0.0, 1.0, 17)
    for k in range(7):
        assert np.array_equal(np.load(tmp_path / "frames" / f"f_{k}.npy"), np.broadcast_to(x + k, (17, 17)))
        assert w.frames[k] == (float(k), {"f": (float(k), 1.0 + k, 0)})


def test_demo_runs_with_few_steps(tmp_path):
    run = subprocess.run([sys.executable, str(ROOT / "demos" / "slab_output.py"), "--lx", "6", "--ly", "3", "--lz", "1", "--dx", "0.25",
                          "--T", "3", "--out", str(tmp_path / "demo" / "slab")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    entries = read_pvd(tmp_path / "demo" / "slab.pvd")
    assert np.allclose([t for t, _ in entries], [1.0, 2.0, 3.0], rtol=0, atol=1e-12) and run.stdout.count("v in [") == 3
    frame = read_vti(tmp_path / "demo" / entries[-1][1])
    assert set(frame.arrays) == {"v", "activation"} and frame.arrays["v"].dtype == np.float32
    assert frame.arrays["v"].max() > 0.0 and np.isfinite(frame.arrays["activation"]).any()
