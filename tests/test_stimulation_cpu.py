"""CPU: host-side stimulus logic that needs no device -- generate_random_activation on DG0 data (mirror of the
reference's tests/test_stimulation.py:305-385) and the unit conversions of define_stimulus."""

import numpy as np
import pytest


def test_generate_random_activation():
    import beat
    from beat import grid as g

    domain = g.create_unit_cube(g.COMM_WORLD, 4, 4, 4)
    t = g.Constant(domain, 0.0)
    points = np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0]])
    delays = np.array([1.0, 3.0])
    stim_amplitude = 5.0
    stim_expr = beat.stimulation.generate_random_activation(mesh=domain, time=t, points=points, delays=delays,
                                                            stim_start=0.0, stim_duration=1.0,
                                                            stim_amplitude=stim_amplitude, tol=0.2)
    V = g.functionspace(domain, ("DG", 0))
    expr = g.Expression(stim_expr, beat.utils.interpolation_points(V))
    stim_func = g.Function(V)
    ids = domain.all_cells()
    mid = g.cell_midpoints(domain, ids).T
    for tv, expected_max in [(0.5, 0.0), (1.5, stim_amplitude), (2.5, 0.0), (3.5, stim_amplitude), (4.5, 0.0)]:
        t.value = tv
        stim_func.interpolate(expr)
        assert np.max(stim_func.x.array) == pytest.approx(expected_max)
        assert np.min(stim_func.x.array) == pytest.approx(0.0)
        # the cell-local fast path equals the plain evaluation of the expression at every centroid
        np.testing.assert_array_equal(stim_func.x.array, stim_expr.evaluate(mid))
    # first point: the cells whose centroid lies in the cube of half-width 0.2 around (0.5, 0.5, 0.5)
    t.value = 1.5
    stim_func.interpolate(expr)
    inside = (np.abs(mid - 0.5) <= 0.2).all(axis=0)
    np.testing.assert_array_equal(stim_func.x.array != 0.0, inside)


def test_generate_random_activation_assertion():
    import beat
    from beat import grid as g

    domain = g.create_unit_cube(g.COMM_WORLD, 1, 1, 1)
    t = g.Constant(domain, 0.0)
    with pytest.raises(AssertionError, match="Points and delays must have the same length"):
        beat.stimulation.generate_random_activation(mesh=domain, time=t, points=np.zeros((2, 3)), delays=np.zeros(3))


def test_generate_random_activation_recursion():
    """tests/test_stimulation.py:389-425 of the reference: 1500 stimulation points at the default recursion limit --
    building the expression, printing it and evaluating it must not recurse per point."""
    import sys

    import beat
    from beat import grid as g

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(1000)
    try:
        mesh = g.create_unit_cube(g.COMM_WORLD, 2, 2, 2)
        time = g.Constant(mesh, 0.0)
        rng = np.random.default_rng(0)
        num_points = 1500
        expr = beat.stimulation.generate_random_activation(mesh=mesh, time=time, points=rng.random((num_points, 3)),
                                                            delays=rng.random(num_points), stim_start=0.0, stim_duration=2.0,
                                                            stim_amplitude=1.0, tol=1e-12)
        assert isinstance(str(expr), str)
        f = g.Function(g.functionspace(mesh, ("DG", 0)))
        time.value = 1.0
        f.interpolate(expr)
        assert np.isfinite(f.x.array).all()
    finally:
        sys.setrecursionlimit(old)


def test_generate_random_activation_respects_voxel_mask():
    import beat
    from beat import grid as g

    mask = np.ones((4, 4, 4), dtype=bool)
    mask[:, :, :2] = False
    mesh = g.create_voxel_mesh(g.COMM_WORLD, mask, 0.25)
    t = g.Constant(mesh, 0.5)
    e = beat.stimulation.generate_random_activation(mesh, t, np.array([[0.5, 0.5, 0.5]]), np.array([0.0]),
                                                    stim_duration=1.0, stim_amplitude=2.0, tol=0.3)
    f = g.Function(g.functionspace(mesh, ("DG", 0)))
    f.interpolate(e)
    nz = np.flatnonzero(f.x.array)
    assert len(nz) > 0 and mesh.active[nz].all()
    assert (g.cell_midpoints(mesh, nz)[:, 0] > 0.5).all()


def test_12_leads_ecg():
    """tests/test_ecg.py:52-80 of the reference."""
    import beat

    x = np.ones(10)
    la, ra, ll = 1.2, 4.5, 3.6
    vs = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    Vw = np.mean([la, ra, ll])
    ecg = beat.ecg.Leads12(LA=la * x, RA=ra * x, LL=ll * x, **{f"V{i}": v * x for i, v in enumerate(vs, start=1)})
    for i, vi in enumerate(vs, start=1):
        assert np.allclose(getattr(ecg, f"V{i}_"), vi - Vw)
    assert np.allclose(ecg.I, la - ra) and np.allclose(ecg.II, ll - ra) and np.allclose(ecg.III, ll - la)
    assert np.allclose(ecg.aVR, 1.5 * (ra - Vw)) and np.allclose(ecg.aVL, 1.5 * (la - Vw)) and np.allclose(ecg.aVF, 1.5 * (ll - Vw))
    with pytest.raises(AttributeError):
        beat.ecg.Leads12(LA=x, RA=x, LL=x).V1_


def test_qt_interval():
    """tests/test_ecg.py:83-113 of the reference."""
    import beat

    qrs_peak_time, t_peak_offset_ms, t_width_ms = 200, 200, 60
    t, y = beat.ecg.example(sampling_rate_hz=1000, duration_s=1, noise_amplitude=0.0, wander_amplitude=0.0,
                            heart_rate_bpm=60, q_offset_ms=40, s_offset_ms=40, t_peak_offset_ms=t_peak_offset_ms,
                            r_width_ms=20, q_width_ms=20, s_width_ms=30, t_width_ms=t_width_ms, qrs_peak_time=qrs_peak_time)
    qt = beat.ecg.qt_interval(t=t, ecg_signal=y)
    assert np.isclose(qt.start_index, qrs_peak_time, atol=2)
    assert np.isclose(qt.end_index, qrs_peak_time + t_peak_offset_ms + 2 * t_width_ms / 3, atol=5)
    assert np.isclose(qt.qt_interval, qt.end_index - qt.start_index)


def test_import_shims_expose_the_reference_module_paths():
    """compat/: the dolfinx / ufl / scifem / mpi4py import lines of the reference's hot-path demos resolve to the
    beat.grid objects."""
    import importlib
    import sys
    from pathlib import Path

    compat = str(Path(__file__).resolve().parents[1] / "fenicsx-beat_amd" / "compat")
    shadowed = {m: sys.modules.pop(m) for m in list(sys.modules) if m.split(".")[0] in ("dolfinx", "ufl", "scifem", "mpi4py")}
    sys.path.insert(0, compat)
    try:
        from beat import grid as g

        dolfinx, ufl, scifem = (importlib.import_module(m) for m in ("dolfinx", "ufl", "scifem"))
        MPI = importlib.import_module("mpi4py.MPI")
        mesh = dolfinx.mesh.create_unit_square(MPI.COMM_WORLD, 4, 4, dolfinx.mesh.CellType.triangle)
        assert isinstance(mesh, g.Mesh) and dolfinx.cpp.mesh.CellType is g.CellType
        time = dolfinx.fem.Constant(mesh, dolfinx.default_scalar_type(0.0))
        expr = ufl.conditional(ufl.And(ufl.ge(time, 0.0), ufl.le(time, 1.0)), 2.0, 0.0)
        assert float(expr.evaluate()) == 2.0
        cells = dolfinx.mesh.locate_entities(mesh, mesh.topology.dim, lambda x: x[0] <= 0.5)
        tags = dolfinx.mesh.meshtags(mesh, mesh.topology.dim, cells, np.full(len(cells), 1, dtype=np.int32))
        dx = ufl.Measure("dx", domain=mesh, subdomain_data=tags)
        assert len(dx(1).cells()) == len(cells) == 16
        assert scifem.evaluate_function is g.evaluate_function and dolfinx.io.VTXWriter is g.VTXWriter
        assert MPI.COMM_WORLD.allreduce(3.0, op=MPI.SUM) == 3.0
    finally:
        sys.path.remove(compat)
        for m in list(sys.modules):
            if m.split(".")[0] in ("dolfinx", "ufl", "scifem", "mpi4py"):
                del sys.modules[m]
        sys.modules.update(shadowed)


def test_performance_monitor_contract(tmp_path, caplog):
    """telemetry: the attributes and keys the reference's own tests rely on (tests/test_telemetry.py)."""
    import json
    import logging
    import time

    from beat.telemetry import NullMonitor, PerformanceMonitor

    null = NullMonitor()
    with null.track_time("anything"):
        pass
    null.record_ksp(None)
    null.advance_step(0.0, 0.1)

    mon = PerformanceMonitor(log_frequency=2, synchronize=False)
    for _ in range(2):
        with mon.track_time("dummy_work"):
            time.sleep(0.01)
    assert mon.timings["dummy_work"] >= 0.02

    class Ksp:
        def __init__(self, its):
            self.its = its

        def getIterationNumber(self):
            return self.its

        def getResidualNorm(self):
            return 1e-6

        def getConvergedReason(self):
            return 2

    mon.record_ksp(Ksp(5))
    mon.record_ksp(None)  # ignored
    mon.record_ksp(Ksp(7))
    assert (mon.ksp_last_iterations, mon.ksp_total_iterations, mon.ksp_max_iterations) == (7, 12, 7)
    assert mon.ksp_last_residual_norm == 1e-6 and mon.ksp_last_converged_reason == 2
    with caplog.at_level(logging.INFO, logger="beat.telemetry"):
        mon.advance_step(0.0, 0.1)
        assert len(caplog.records) == 0
        mon.advance_step(0.1, 0.2)
        assert len(caplog.records) == 1 and "PDE step timing step=2" in caplog.records[0].message
        assert "dummy_work=" in caplog.records[0].message
        mon.display_summary()
        assert len(caplog.records) == 2 and "PERFORMANCE SUMMARY" in caplog.records[1].message
    mon.timings["test_metric"] = 1.234
    out = tmp_path / "sub" / "summary.json"
    mon.save_summary(out)
    data = json.loads(out.read_text())
    assert data["total_steps"] == 2 and data["ksp"]["total_iterations"] == 12 and data["timings"]["test_metric"] == 1.234


@pytest.mark.parametrize("dim,subdomain_dim,integral_type", [(2, 1, "exterior_facet"), (2, 2, "cell"), (3, 2, "exterior_facet"), (3, 3, "cell")])
def test_get_dZ_and_effective_dim(dim, subdomain_dim, integral_type):
    """tests/test_stimulation.py:110-205 of the reference for the entity dimensions this package has
    (cells and exterior facets)."""
    import beat
    from beat import grid as g

    mesh = g.create_unit_square(g.COMM_WORLD, 2, 2, g.CellType.triangle) if dim == 2 else g.create_unit_cube(g.COMM_WORLD, 2, 2, 2)
    ents = g.locate_entities(mesh, subdomain_dim, lambda x: np.logical_and(x[0] <= 0.5, x[1] <= 0.5))
    tags = g.meshtags(mesh, subdomain_dim, ents, np.full(len(ents), 1, dtype=np.int32))
    assert len(ents) > 0
    dZ = beat.stimulation.get_dZ(mesh, tags)
    assert isinstance(dZ, g.Measure) and dZ.integral_type() == integral_type
    assert beat.stimulation.compute_effective_dim(mesh, tags) == subdomain_dim + (3 - dim)


def test_unit_helpers_of_define_stimulus():
    """tests/test_stimulation.py:208-250 of the reference: compute_stimulus_unit, convert_chi, convert_amplitude."""
    import beat

    ureg = beat.units.ureg
    for effective_dim, mesh_unit, expected in [(0, "cm", "uA"), (1, "cm", "uA"), (2, "cm", "uA/cm"), (3, "cm", "uA/cm**2"),
                                               (2, "mm", "uA/mm"), (3, "mm", "uA/mm**2")]:
        assert beat.stimulation.compute_stimulus_unit(effective_dim, mesh_unit) == ureg(expected)
    assert beat.stimulation.convert_chi(1.0, "cm") == 1.0 * ureg("cm**-1")
    assert beat.stimulation.convert_chi(2.0 * ureg("mm**-1"), "cm") == 2.0 * ureg("mm**-1")
    for effective_dim, unit in [(1, "uA / cm"), (2, "uA / cm**2"), (3, "uA / cm**3")]:
        assert beat.stimulation.convert_amplitude(effective_dim, 2.0) == 2.0 * ureg(unit)
    assert 1.0 * ureg("cm") == 10.0 * ureg("mm") and not (1.0 * ureg("cm") == 1.0 * ureg("ms"))
    assert "uF" in repr(1.0 * ureg("uF/cm**2"))


def test_telemetry_caller_tests_run_under_the_import_shims(tmp_path):
    """Drop-in check where it needs no device: tests/_telemetry_caller.py -- the telemetry contract as a script written for
    the reference package exercises it (``from mpi4py import MPI``, a mocked KSP, the root logger) -- collected in a
    subprocess whose path holds only ``beat`` and the import shims (fenicsx-beat_amd/compat), without this suite's conftest.
    The module is collected from a copy in ``tmp_path``, with ``--confcutdir`` there: pytest lists every directory from the
    confcutdir down to a file it collects, and an ordinary user may not be allowed to list the ones above a checkout."""
    import os
    import shutil
    import subprocess
    import sys
    from pathlib import Path

    tests = Path(__file__).resolve().parent
    pkg = tests.parent / "fenicsx-beat_amd"
    caller = shutil.copy(tests / "_telemetry_caller.py", tmp_path / "test_telemetry_caller.py")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=f"{pkg / 'compat'}{os.pathsep}{pkg}")
    run = subprocess.run([sys.executable, "-m", "pytest", str(caller), "-q", "-p", "no:cacheprovider", "--noconftest",
                          f"--rootdir={tmp_path}", f"--confcutdir={tmp_path}", "-c", os.devnull],
                         cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "6 passed" in run.stdout


def test_comm_allreduce_honours_the_reduction_op():
    """mpi4py's comm.allreduce(value, op=...) on the communicator stand-in: SUM / MAX / MIN / PROD map to the matching
    collective (one rank: the value itself), anything else raises instead of silently summing."""
    from beat import grid as g

    sys_path_shim = __import__("sys").path
    compat = str(__import__("pathlib").Path(g.__file__).resolve().parents[1] / "compat")
    if compat not in sys_path_shim:
        sys_path_shim.insert(0, compat)
    from mpi4py import MPI

    comm = MPI.COMM_WORLD
    for op in (None, MPI.SUM, MPI.MAX, MPI.MIN, MPI.PROD):
        assert comm.allreduce(3.5, op=op) == 3.5
    import pytest

    with pytest.raises(ValueError):
        comm.allreduce(1.0, op="xor")


def test_single_cell_pacing_of_a_host_callable(tmp_path):
    """beat.single_cell.get_steady_state with an ordinary Python step function (the reference's convention:
    fun(states=, t=, parameters=, dt=), src/beat/single_cell.py:86-156): nbeats repetitions of the times arange(0, BCL, dt),
    tracked states recorded before every save_freq-th step of a beat, result cached under a key of function, inputs and
    protocol -- against a literal double loop."""
    import beat

    calls = []

    def fun(states, t, parameters, dt):
        calls.append(t)
        a, b = parameters
        v, s = states
        return np.array([v + dt * (-a * s + (1.0 if t < 0.25 else 0.0)), s + dt * b * v])

    y0, P = np.array([1.0, 0.0]), np.array([2.0, 0.5])
    dt, BCL, nbeats, every = 0.1, 1, 3, 0.3
    y = beat.single_cell.get_steady_state(fun, y0, P, tmp_path / "cache", nbeats=nbeats, BCL=BCL, save_every_ms=every, dt=dt,
                                          track_indices=[1, 0])
    times = np.arange(0.0, BCL, dt)
    assert len(calls) == nbeats * len(times) and np.allclose(calls[: len(times)], times) and calls[len(times)] == 0.0
    ref, rows = y0.copy(), []
    for _ in range(nbeats):
        for j, t in enumerate(times):
            if j % 3 == 0:
                rows.append([ref[1], ref[0]])
            ref = np.array([ref[0] + dt * (-2.0 * ref[1] + (1.0 if t < 0.25 else 0.0)), ref[1] + dt * 0.5 * ref[0]])
    np.testing.assert_allclose(y, ref, rtol=1e-15)
    tracked = np.load(next((tmp_path / "cache").glob("tracked_values_*.npy")))
    assert tracked.shape == (nbeats * 4, 2)
    np.testing.assert_allclose(tracked, np.array(rows), rtol=1e-15)
    # second call: served from the cache (the function is not called again); other inputs: another key
    n = len(calls)
    y2 = beat.single_cell.get_steady_state(fun, y0, P, tmp_path / "cache", nbeats=nbeats, BCL=BCL, save_every_ms=every, dt=dt)
    assert len(calls) == n and np.array_equal(y2, y)
    k = beat.single_cell.compute_hash(fun, y0, P, nbeats, BCL, dt)
    assert k != beat.single_cell.compute_hash(fun, y0 + 1e-12, P, nbeats, BCL, dt)
    assert k != beat.single_cell.compute_hash(fun, y0, P, nbeats + 1, BCL, dt)
    assert k != beat.single_cell.compute_hash(lambda states, t, parameters, dt: states * 2.0, y0, P, nbeats, BCL, dt)
