"""beat (MI355X) -- HIP-native operator-split monodomain solver with the fenicsx-beat API surface.

``beat.MonodomainModel``, ``beat.odesolver.DolfinODESolver`` and ``beat.MonodomainSplittingSolver``
keep the reference's constructor signatures, methods and step semantics; meshes are structured
boxes (``beat.grid`` provides the handful of dolfinx/ufl names the callers use) and all arithmetic
runs in ``libbeat_hip.so``.  There is no CPU fallback."""

from . import (  # noqa: F401
    base_model,
    butcher,
    conductivities,
    ecg,
    events,
    fibres,
    geometry,
    grid,
    io,
    irksome_model,
    models,
    monodomain_model,
    monodomain_solver,
    odesolver,
    output,
    single_cell,
    stimulation,
    telemetry,
    units,
    utils,
)
from .ecg import ECGRecovery, LeadRecorder
from .events import EventRecorder
from .irksome_model import IrksomeMonodomainModel
from .monodomain_model import MonodomainModel
from .monodomain_solver import MonodomainSplittingSolver
from .output import FieldWriter
from .stimulation import Stimulus
from .telemetry import BaseMonitor, NullMonitor, PerformanceMonitor

__version__ = "0.1.0"
__program_name__ = "fenicsx-beat-amd"

__all__ = [
    "monodomain_model", "irksome_model", "IrksomeMonodomainModel", "butcher", "odesolver", "base_model", "MonodomainModel", "monodomain_solver",
    "MonodomainSplittingSolver", "utils", "single_cell", "conductivities", "stimulation", "geometry", "grid", "models",
    "Stimulus", "io", "ecg", "ECGRecovery", "LeadRecorder", "events", "EventRecorder", "fibres", "output", "FieldWriter", "telemetry", "BaseMonitor", "NullMonitor", "PerformanceMonitor", "units",
]
