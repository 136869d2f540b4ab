"""Collected by tests/test_stimulation_cpu.py in a fresh interpreter whose path holds only the package and the import
shims (fenicsx-beat_amd/compat): the telemetry contract as a script written for the reference package uses it --
``mpi4py``'s communicator handed to the monitor, a mocked PETSc KSP, the root logger at INFO, rank-0-only reports."""
import json
import logging
import time
from unittest.mock import MagicMock

from mpi4py import MPI

from beat.telemetry import NullMonitor, PerformanceMonitor


def test_null_monitor_takes_every_hook():
    mon = NullMonitor()
    with mon.track_time("ignored"):
        pass
    mon.record_ksp(None)
    mon.record_ksp(MagicMock())
    mon.advance_step(0.0, 0.5)


def test_regions_accumulate_under_one_name():
    mon = PerformanceMonitor(comm=MPI.COMM_WORLD)
    for k in range(3):
        with mon.track_time("work"):
            time.sleep(0.005)
        assert mon.timings["work"] >= 0.005 * (k + 1)
    assert list(mon.timings) == ["work"]


def test_ksp_statistics_from_a_mocked_ksp():
    mon = PerformanceMonitor(comm=MPI.COMM_WORLD)
    ksp = MagicMock()
    ksp.getResidualNorm.return_value = 2.5e-9
    ksp.getConvergedReason.return_value = 3
    for its, total, most in ((4, 4, 4), (9, 13, 9), (2, 15, 9)):
        ksp.getIterationNumber.return_value = its
        mon.record_ksp(ksp)
        assert (mon.ksp_last_iterations, mon.ksp_total_iterations, mon.ksp_max_iterations) == (its, total, most)
    assert mon.ksp_last_residual_norm == 2.5e-9 and mon.ksp_last_converged_reason == 3


def test_a_log_line_every_log_frequency_steps(caplog):
    caplog.set_level(logging.INFO)
    mon = PerformanceMonitor(log_frequency=3, comm=MPI.COMM_WORLD)
    with mon.track_time("ode"):
        pass
    for k in range(6):
        mon.advance_step(0.1 * k, 0.1 * (k + 1))
    assert [r.message.split(",")[0] for r in caplog.records] == ["PDE step timing step=3", "PDE step timing step=6"]
    assert all("ode=" in r.message for r in caplog.records)


def test_summary_file_on_rank_zero(tmp_path):
    comm = MPI.COMM_WORLD
    mon = PerformanceMonitor(comm=comm)
    mon.step_counter, mon.ksp_total_iterations = 7, 31
    mon.timings["solve"] = 0.75
    target = tmp_path / "perf.json"
    mon.save_summary(target)
    assert comm.rank == 0  # (the shim's communicator is one rank)
    data = json.loads(target.read_text())
    assert data["total_steps"] == 7 and data["ksp"]["total_iterations"] == 31 and data["timings"] == {"solve": 0.75}


def test_summary_table_is_one_record_slowest_first(caplog):
    caplog.set_level(logging.INFO)
    mon = PerformanceMonitor(comm=MPI.COMM_WORLD)
    mon.step_counter = 12
    mon.timings.update(quick=0.2, slow=3.0, middle=1.0)
    mon.display_summary()
    assert len(caplog.records) == 1
    text = caplog.records[0].message
    assert "PERFORMANCE SUMMARY" in text and "Total Steps:           12" in text
    assert text.find("slow") < text.find("middle") < text.find("quick")
