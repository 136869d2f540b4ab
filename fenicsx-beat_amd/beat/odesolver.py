"""ODE (reaction) solvers -- interface of src/beat/odesolver.py:24-354.

``fun`` follows the reference's convention, ``fun(states=, t=, parameters=, dt=) -> new states``.
When ``fun`` is one of the built-in device models (``beat.models``) the ``(S, N)`` state array
lives in HBM and a step is one kernel launch; any other callable is the caller's own NumPy code and
is run exactly as the reference runs it (host arrays, the transmembrane potential staged to and
from the device field)."""

from __future__ import annotations

import abc
import ctypes as C
import logging
import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Any, Callable, NamedTuple

import numpy as np

from . import _hip, grid
from ._param_route import ParameterRoutes
from .models._base import DeviceModel, DeviceParameters
from .telemetry import BaseMonitor, NullMonitor
from .utils import local_project

EPS = 1e-12
logger = logging.getLogger(__name__)


class ODEResults(NamedTuple):
    y: np.ndarray
    t: np.ndarray


def solve(fun, t_bound: float, states, V, V_index: int, dt: float, parameters, t0: float = 0.0, extra=None):
    """Free-running multi-point loop of odesolver.py:24-43 (``states`` is advanced in place)."""
    if extra is None:
        extra = {}
    i = 0
    t = t0
    while t + dt < t_bound:
        new = fun(states=states, t=t, parameters=parameters, dt=dt, **extra)
        if new is not None and new is not states:
            states[:] = new
        V[i, :] = states[V_index, :]
        i += 1
        t += dt


@dataclass
class ODESystemSolver:
    fun: Callable
    states: np.ndarray
    parameters: np.ndarray
    missing_variables: np.ndarray | None = None
    _kwargs: dict = field(default_factory=dict)
    monitor: BaseMonitor = field(default_factory=NullMonitor)

    def __post_init__(self):
        if self.missing_variables is not None:
            self._kwargs["missing_variables"] = self.missing_variables

    @property
    def num_points(self) -> int:
        return self.states.shape[1]

    @property
    def num_states(self) -> int:
        return self.states.shape[0]

    def step(self, t0: float, dt: float) -> None:
        with self.monitor.track_time("ode_total_step"):
            with self.monitor.track_time("ode_function_call"):
                updated_states = self.fun(states=self.states, t=t0, parameters=self.parameters, dt=dt, **self._kwargs)
            with self.monitor.track_time("ode_state_update"):
                self.states[:] = updated_states


def _initial_values(init_states, shape, on_device: bool):
    """(S, N) initial values as the reference builds them (odesolver.py:149-153): a full array is copied, a
    per-state vector is broadcast to every point.  On the device the broadcast is done row by row in HBM
    (no (S, N) host array), signalled by returning the 1-D vector."""
    if np.shape(init_states) == shape:
        return np.copy(init_states)
    vec = np.asarray(init_states, dtype=np.float64)
    if on_device and vec.shape == (shape[0],):
        return vec
    values = np.zeros(shape)
    values.T[:] = init_states
    return values


class _CallableMonitor:
    """What ``ode.monitor`` of the Dolfin solvers is.  The dataclass field of that name holds the TELEMETRY monitor (the reference's
    interface: ``DolfinODESolver(..., monitor=...)``, ``ode.monitor.track_time(...)``) and stays that: every attribute read or set
    here is that object's (``telemetry``).  Called -- ``ode.monitor(names, t, out=None)`` -- it is the solver's
    ``monitor_values``: the model's monitored values on the device."""

    def __init__(self, telemetry, call):
        object.__setattr__(self, "telemetry", telemetry)
        object.__setattr__(self, "_call", call)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "telemetry"), name)

    def __setattr__(self, name, value):
        setattr(self.telemetry, name, value)

    def __call__(self, names, t, out=None):
        return self._call(names, t, out=out)


def _route_ops(ctx):
    """What ``ParameterRoutes`` does on the device or in the library (beat/_param_route.py)."""
    def class_table_doubles(model_id):
        stride = C.c_int()
        _hip.check(ctx.lib.beat_ode_class_table_doubles(model_id, C.byref(stride)))
        return stride.value

    def class_table_fill(model_id, sets, table):
        _hip.check(ctx.lib.beat_ode_class_table_fill(ctx.handle, model_id, sets.ctypes.data_as(C.c_void_p), sets.shape[1], sets.shape[0],
                                                     C.c_void_p(table.data_ptr())))

    return SimpleNamespace(torch=ctx.torch, from_numpy=ctx.from_numpy, zeros=ctx.zeros, class_table_doubles=class_table_doubles,
                           class_table_fill=class_table_fill, jit_available=lambda: ctx.lib.beat_ode_jit_stats(None) == 1)


class _DeviceODE:
    """(S, N) state array in HBM advanced by a built-in model kernel.  For a model with M missing variables
    (``beat.models.from_ode(..., missing=...)``) the array has S + M rows: the kernel reads rows S .. S + M - 1 as its inputs and
    never writes them; ``set_initial`` / ``set_states`` / ``state_values`` mean the S state rows."""

    def __init__(self, ctx, model: DeviceModel, num_states, n, plane, parameters, monitor):
        from ._device import StateArray

        if num_states != model.num_states:
            raise ValueError(f"{model.name} has {model.num_states} states, num_states={num_states}")
        if hasattr(model, "register"):  # a model generated from an .ode file (beat.models.from_ode): its source goes to the library
            model.register()
        self.ctx = ctx
        self.model = model
        self.n = n
        self.num_states, self.num_inputs = int(num_states), int(model.num_missing_variables)
        self.states = StateArray(ctx, self.num_states + self.num_inputs, n, plane)
        self.parameters = parameters
        self.monitor = monitor
        self.node_map = None   # (int32 node of the PDE grid per entry, the field holding the potential): compact layout
        self.routes = ParameterRoutes(model.name, model.num_parameters, model.model_id, n, _route_ops(ctx))

    # How the parameters reach the kernel is decided and cached by ``routes`` alone; these answer from its current route.
    classes = property(lambda self: self.routes.current.classes)  # (marker bytes on the device, class table, number of classes) | None
    _sparse = property(lambda self: self.routes.current.rows)  # (uniform vector, indices of the varying rows, their (K, N) rows) | None
    explicit_classes = property(lambda self: self.routes.explicit, lambda self, on: setattr(self.routes, "explicit", bool(on)))

    def set_classes(self, markers_dev, param_sets) -> None:
        """The explicit route (ParameterRoutes.set_classes): a byte per node names one of ``param_sets``; the parameters no longer decide."""
        self.routes.set_classes(markers_dev, param_sets)

    def set_initial(self, values) -> None:
        if values.ndim == 1:
            for k, val in enumerate(values):
                self.states.row_field(k).fill(float(val))
        else:
            self.set_states(values)

    def set_states(self, values) -> None:
        """The S state rows from an (S, N) host array."""
        if self.num_inputs == 0:
            return self.states.set(values)
        values = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        assert values.shape == (self.num_states, self.n), (values.shape, (self.num_states, self.n))
        self.states.rows[: self.num_states].copy_(self.ctx.torch.from_numpy(values))

    def state_values(self) -> np.ndarray:
        """The S state rows as an (S, N) host array."""
        return self.states.numpy() if self.num_inputs == 0 else self.states.rows[: self.num_states].cpu().numpy()

    def input_field(self, j: int):
        """Input row j (row S + j of the array) as a field."""
        if not 0 <= int(j) < self.num_inputs:
            raise IndexError(f"{self.model.name} has {self.num_inputs} missing variables, asked for {j}")
        return self.states.row_field(self.num_states + int(j))

    def monitor_rows(self, names, t, out_ptr, out_ld) -> None:
        """The monitor kernel of a generated model on the resident states, with the parameters as they are now and by the route the
        next step would take them (uniform vector, classes; per-node rows are read whole -- a generated model has no sparse-row
        instance).  The caller has brought the potential row up to date.  Does not wait."""
        route = self.routes.resolve(self.parameters)
        if route.kind == "none":
            raise ValueError(f"{self.model.name}: monitored values need the parameters")
        self.model.monitor_on_device(self.ctx, names, self.states.ptr, self.n, self.states.ld, t, out_ptr, out_ld, **route.monitor_kwargs())

    def step(self, t0, dt, v_index=0, v_copy=None, pending_ops=None, v_row=None):
        """``pending_ops``: diffusion operators whose last solve deferred its update of ``v_row`` (row v_index of
        these states): the kernel adds it while loading the potential (beat_ode_step_pending)."""
        route = self.routes.resolve(self.parameters)
        model_v = self.model.state_index(self.model.v_name) if self.model.v_name else -1
        if route.kind == "classes" and route.fallback is not None and v_copy is not None and self.model.v_name and int(v_index) != model_v:
            # the class kernel mirrors the model's own potential row only: per-node parameters that were routed to classes
            # go back to the per-node kernel, which mirrors any row (what the reference's v_index means, odesolver.py:135-146)
            route = route.fallback
        # (operator, ring, field stride, count) of what the launch applies, as the pending-update entry points take them; count -1:
        # the launch is enqueued BEHIND a solve that is still open (beat_ode_step_pending)
        pend_args = (None, None, 0, 0) if pending_ops is None else pending_ops.deferred.claim(
            v_row, int(v_index) == model_v, None if self.node_map is None else self.node_map[1], route.kind == "classes")
        lib, states = self.ctx.lib, (self.ctx.handle, self.model.model_id, self.states.ptr, self.n, self.states.ld)
        when = (float(t0), float(dt), int(v_index), None if v_copy is None else v_copy.ptr)
        with self.monitor.track_time("ode_total_step"):
            with self.monitor.track_time("ode_function_call"):  # the one place that maps a route's kind to its entry point
                if route.kind == "classes":
                    if int(v_index) != model_v and pend_args[0] is not None:
                        raise ValueError("a pending update needs the model's own potential row")
                    nmap, vfield = (None, None) if self.node_map is None else (C.c_void_p(self.node_map[0].data_ptr()), self.node_map[1].ptr)
                    _hip.check(lib.beat_ode_step_classes(*states, *route.args(), *when, nmap, vfield, *pend_args))
                elif route.kind == "rows":
                    _hip.check(lib.beat_ode_step_rows(*states, *route.args(), *when, *pend_args))
                elif pend_args[0] is not None:
                    _hip.check(lib.beat_ode_step_pending(*states, *route.args(), *when, *pend_args))
                else:
                    _hip.check(lib.beat_ode_step(*states, *route.args(), *when))
            if pend_args[3] < 0:  # the call has finished the solve it was enqueued behind: take its record
                pending_ops.deferred.finished_behind()
            with self.monitor.track_time("ode_state_update"):
                pass  # updated in place by the kernel


ROWS_NONTEMPORAL = False  # beat_rows_to_fields reads the rows with plain loads (profiles/multi_state_fields.md has both)


class _RowsPlan:
    """A ``beat_rows_plan`` (include/beat_hip.h) over the state arrays of a ``DolfinMultiODESolver``: where every node's states
    live (``layout``: beat._rows_layout), each class's array (``bases``: device addresses, ``lds``).  Moves up to 8 rows per launch
    between the arrays and fields of the grid, on the context's stream, without waiting."""

    def __init__(self, ctx, layout, bases, lds, cls_dev=None):
        k = len(bases)
        self.ctx, self.n, self.num_classes, self.bases, self.lds = ctx, int(layout.cls.size), k, tuple(bases), tuple(lds)
        self._cls = ctx.from_numpy(layout.cls) if cls_dev is None else cls_dev  # (borrowed by the plan: kept alive here)
        self._pos = None if layout.pos is None else ctx.from_numpy(layout.pos)
        self.handle = C.c_void_p()
        _hip.check(ctx.lib.beat_rows_plan_create(
            ctx.handle, self.n, self._cls.data_ptr(), None if self._pos is None else self._pos.data_ptr(), k, (C.c_void_p * k)(*bases),
            (C.c_int64 * k)(*lds), (C.c_int64 * k)(*layout.class_n), (C.c_int * k)(*layout.class_rows), C.byref(self.handle)))

    def _args(self, rows, fields):
        for fld in fields:
            if fld.n != self.n:
                raise ValueError(f"expected a field of {self.n} values, got {fld.n}")
        flat = [int(r) for rows_f in rows for r in rows_f]
        return len(fields), (C.c_int * len(flat))(*flat), (C.c_void_p * len(fields))(*[f.ptr.value for f in fields])

    def expand(self, rows, fields, fill=None, nontemporal=None) -> None:
        """fields[f][i] = row rows[f][c] of node i's class c at the node's column; a node without a class keeps its value (``fill``
        None) or gets ``fill``.  More than 8 fields go in chunks."""
        nt = ROWS_NONTEMPORAL if nontemporal is None else nontemporal
        mode = (_hip.ROWS_KEEP if fill is None else _hip.ROWS_FILL) | (_hip.ROWS_NT_LOADS if nt else 0)
        for a in range(0, len(fields), _hip.ROWS_MAX_FIELDS):
            nf, flat, ptrs = self._args(rows[a : a + _hip.ROWS_MAX_FIELDS], fields[a : a + _hip.ROWS_MAX_FIELDS])
            _hip.check(self.ctx.lib.beat_rows_to_fields(self.handle, nf, flat, ptrs, mode, 0.0 if fill is None else float(fill), 0))

    def collapse(self, rows, fields) -> None:
        """The other way: the nodes with a class write fields[f][i] into their class's row."""
        for a in range(0, len(fields), _hip.ROWS_MAX_FIELDS):
            nf, flat, ptrs = self._args(rows[a : a + _hip.ROWS_MAX_FIELDS], fields[a : a + _hip.ROWS_MAX_FIELDS])
            _hip.check(self.ctx.lib.beat_fields_to_rows(self.handle, nf, flat, ptrs, 0))

    def __del__(self):  # pragma: no cover
        try:
            self.ctx.lib.beat_rows_plan_destroy(self.handle)
        except Exception:
            pass


class BaseDolfinODESolver(abc.ABC):
    v_ode: grid.Function
    v_pde: grid.Function
    _metadata: dict[str, Any] | None = None
    _pending_ops = None  # diffusion operators that may hold a deferred update of the V row (fused step)
    _aliases: tuple = ()  # functions that alias the V row (see grid.Function)

    def _sync_v(self):
        """Bring the V row up to date if the last fused diffusion solve left its final update to the next ionic
        kernel (deferred-x PCG): everything that reads or overwrites the row outside that kernel calls this."""
        if self._pending_ops is not None:
            self._pending_ops.flush_pending()

    def _release_aliases(self):
        """The V row is about to change outside the fused step: give every function that merely
        aliases it its own copy of the current values first."""
        self._sync_v()
        for f in self._aliases:
            if f._alias is self._v_row:
                f.materialize()
        self._aliases = ()

    def _alias_v(self, ops, *functions) -> None:
        """``functions`` (the potential's: pde.state, pde.v_, v_ode) become aliases of the V row, which ``ops`` completes."""
        self._pending_ops = ops
        for f in functions:
            f.alias_to(self._v_row, sync=ops.deferred)
        self._aliases = functions

    def _initialize_metadata(self):
        if self.v_ode.ufl_element().family_name == "Quadrature":
            self._metadata = {"quadrature_degree": self.v_ode.ufl_element().degree()}
        else:
            self._metadata = None

    @abc.abstractmethod
    def to_dolfin(self) -> None: ...

    @abc.abstractmethod
    def from_dolfin(self) -> None: ...

    def ode_to_pde(self) -> None:
        local_project(self.v_ode, self.v_pde.function_space, self.v_pde)

    def pde_to_ode(self) -> None:
        local_project(self.v_pde, self.v_ode.function_space, self.v_ode)

    @abc.abstractmethod
    def step(self, t0: float, dt: float) -> None: ...

    @property
    @abc.abstractmethod
    def full_values(self): ...


@dataclass
class DolfinODESolver(BaseDolfinODESolver):
    v_ode: grid.Function
    v_pde: grid.Function
    init_states: np.ndarray
    parameters: np.ndarray
    fun: Callable
    num_states: int
    v_index: int = 0
    missing_variables: np.ndarray | None = None
    num_missing_variables: int = 0
    monitor: BaseMonitor = field(default_factory=NullMonitor)

    def __post_init__(self):
        self.on_device = isinstance(self.fun, DeviceModel)
        values = _initial_values(self.init_states, self.shape, self.on_device)
        if self.on_device:
            m = int(self.fun.num_missing_variables)
            if m == 0 and self.missing_variables is not None:
                raise ValueError(f"{self.fun.name} has no missing variables: missing_variables would be ignored (a model made by "
                                 "beat.models.from_ode(..., missing=...) takes them)")
            if m and m != int(self.num_missing_variables):
                raise ValueError(f"{self.fun.name} has {m} missing variables, num_missing_variables={self.num_missing_variables}")
            mesh = self.v_ode.function_space.mesh
            plane = mesh.plane if self.v_ode.function_space.is_p1 else 0  # only P1 rows are stencil operands
            self._dev = _DeviceODE(self.v_ode._ctx, self.fun, self.num_states, self.num_points, plane,
                                   self.parameters, self.monitor)
            self._dev.set_initial(values)
            self._v_row = self._dev.states.row_field(self.v_index)
            self._ode = self._dev
            self._missing_sent = None      # the (M, N) values that were uploaded: what the live array is compared with
            self._missing_functions = {}   # row -> (the function that IS the row, its version when handed out)
            self._missing_resident = set()  # rows written on the device: the NumPy array no longer decides them
            if m:
                if self.missing_variables is None:
                    self.missing_variables = self.fun.init_missing_values()
                self._refresh_missing()
        else:
            self._values = values
            self._ode = ODESystemSolver(fun=self.fun, states=self._values, parameters=self.parameters,
                                        missing_variables=self.missing_variables, monitor=self.monitor)
        self._initialize_metadata()
        self.monitor = _CallableMonitor(self.monitor, self.monitor_values)

    # ---- reference interface --------------------------------------------------------------------
    def to_dolfin(self) -> None:
        """values[v_index] -> v_ode  (odesolver.py:164-166)"""
        if self.on_device:
            if self.v_ode._alias is self._v_row:
                return
            self._sync_v()
            self.v_ode.writable_field().copy_from(self._v_row)
            self.v_ode._touch()
        else:
            self.v_ode.x.array[:] = self._values[self.v_index, :]

    def from_dolfin(self) -> None:
        """v_ode -> values[v_index]  (odesolver.py:168-170)"""
        if self.on_device:
            if self.v_ode._alias is self._v_row:
                return
            self._release_aliases()
            self._v_row.copy_from(self.v_ode.field)
        else:
            self._values[self.v_index, :] = np.asarray(self.v_ode.x.array)

    @property
    def values(self):
        if self.on_device:
            self._sync_v()
            return self._dev.state_values()
        return self._values

    # ---- missing variables of a split cell model, on the device -----------------------------------
    def _refresh_missing(self) -> None:
        """The input rows as ``missing_variables`` has them NOW: the live (M,) or (M, N) array is compared with the copy that was
        uploaded and the rows edited in place since are uploaded again (the reference hands ``fun`` the live array on every step;
        the rule ``ParameterRoutes.resolve`` applies to a live (P, N) parameter array).  A row that has been written on the
        device -- through ``missing_function`` or ``set_missing`` -- is resident: the array is no longer consulted for it."""
        m = self._dev.num_inputs if self.on_device else 0
        if m == 0:
            return
        for j, (f, version) in self._missing_functions.items():
            if f._version != version:
                self._missing_resident.add(j)
        if len(self._missing_resident) == m:
            return
        live = np.asarray(self.missing_variables, dtype=np.float64)
        if live.shape not in ((m,), (m, self.num_points)):
            raise ValueError(f"missing_variables must have shape ({m},) or {self.shape_missing_values}, got {live.shape}")
        live = live.reshape(m, -1)
        sent = self._missing_sent
        for j in range(m):
            if j in self._missing_resident or (sent is not None and sent[j].shape == live[j].shape and np.array_equal(sent[j], live[j])):
                continue
            self._dev.input_field(j).set(live[j])  # ((1,) is broadcast to the row)
            if j in self._missing_functions:  # (the upload is not a write THROUGH the function: the row stays the array's)
                f = self._missing_functions[j][0]
                f._touch()
                self._missing_functions[j] = (f, f._version)
        self._missing_sent = live.copy()

    def _missing_row(self, name) -> int:
        if not (self.on_device and self._dev.num_inputs):
            raise ValueError(f"{getattr(self.fun, 'name', self.fun)} has no missing variables on the device")
        return self.fun.missing_index(name) if isinstance(name, str) else int(name)

    def missing_function(self, name) -> grid.Function:
        """A function on ``v_ode``'s space whose field IS the kernel's input row of the missing variable ``name``: whatever writes
        it -- ``other.monitor([...], t, out=[f])``, ``other.state_to_function(k, f)``, ``f.x.array[:] = ...`` -- writes what the
        next step reads, with no pass over the host.  Once the row has been written through it, the ``missing_variables`` array
        is no longer consulted for that row."""
        j = self._missing_row(name)
        if j not in self._missing_functions:
            f = grid.Function(self.v_ode.function_space, name=self.fun.missing_names[j], field=self._dev.input_field(j))
            self._missing_functions[j] = (f, f._version)
        return self._missing_functions[j][0]

    def set_missing(self, name, value) -> None:
        """The missing variable ``name`` at every node from a float, an (N,) array or a ``grid.Function`` (a device copy).  The
        row is resident from here on: the ``missing_variables`` array is no longer consulted for it."""
        j = self._missing_row(name)
        row = self._dev.input_field(j)
        if isinstance(value, grid.Function):
            if value.num_values != row.n:  # (the copy is row.n values long)
                raise ValueError(f"expected a function of {row.n} values, got {value.num_values}")
            row.copy_from(value.field)
        elif np.ndim(value) == 0:
            row.fill(float(value))
        else:
            value = np.asarray(value, dtype=np.float64)
            if value.shape != (self.num_points,):
                raise ValueError(f"expected {self.num_points} values, got shape {value.shape}")
            row.set(value)
        self._missing_resident.add(j)
        if j in self._missing_functions:
            self._missing_functions[j][0]._touch()

    def state_to_function(self, index_or_name, out: grid.Function) -> grid.Function:
        """State row ``index_or_name`` copied on the device into ``out`` (for instance another solver's ``missing_function``).
        With ``missing_function`` and ``set_missing`` this couples two device solvers without a device-to-host copy."""
        if not self.on_device:
            raise NotImplementedError("state_to_function copies a row of the device's state array: fun is a host callable")
        k = self.fun.state_index(index_or_name) if isinstance(index_or_name, str) else int(index_or_name)
        if not 0 <= k < self.num_states:
            raise IndexError(f"state {k} of {self.num_states}")
        if out.num_values != self._dev.n:  # (the copy is as long as ``out``)
            raise ValueError(f"expected a function of {self._dev.n} values, got {out.num_values}")
        if k == self.v_index:
            self._sync_v()
        out.writable_field().copy_from(self._dev.states.row_field(k))
        out._touch()
        return out

    @property
    def num_parameters(self) -> int:
        return len(self.parameters)

    @property
    def shape(self) -> tuple[int, int]:
        return (self.num_states, self.num_points)

    @property
    def shape_missing_values(self) -> tuple[int, int]:
        return (self.num_missing_variables, self.num_points)

    @property
    def num_points(self) -> int:
        return self.v_ode.x.array.size

    def step(self, t0: float, dt: float):
        if self.on_device:
            self._release_aliases()
            self._dev.parameters = self.parameters
            self._refresh_missing()
            self._dev.step(t0, dt)
        else:
            self._ode.step(t0=t0, dt=dt)

    def monitor_values(self, names, t: float, out: list[grid.Function] | None = None) -> list[grid.Function]:
        """``ode.monitor(names, t, out=None)`` (see _CallableMonitor: ``monitor`` is also the telemetry field).  The model's monitored values ``names`` (a gotranx module's ``monitor_values``: currents, fluxes, rates, ``d<state>_dt``
        -- ``fun.monitor_names``) at every node, at time ``t``, as functions on ``v_ode``'s space: evaluated on the device from
        the resident states and the parameters as they are now; no state leaves the device.  ``out``: functions to write into
        instead of new ones.  Returns without waiting for the kernel.  For models made by ``beat.models.from_ode``."""
        if not self.on_device or not hasattr(self.fun, "monitor_on_device"):
            raise NotImplementedError("monitor() evaluates the named intermediates of a model made by beat.models.from_ode: a hand-written "
                                      "kernel or a host callable keeps none; use from_ode on the model's .ode file")
        V = self.v_ode.function_space
        if V.mesh.comm.size > 1:
            raise NotImplementedError("monitor() is not available on a decomposed mesh")
        from ._device import StateArray

        names = [names] if isinstance(names, str) else list(names)
        if out is not None and len(out) != len(names):
            raise ValueError(f"{len(names)} names, {len(out)} functions")
        # the potential row must be complete: a step leaves its solve open and its last update to the next ionic launch
        # (what to_dolfin / values do before they read the row: finish the solve, apply the update)
        self._sync_v()
        self._dev.parameters = self.parameters
        self._refresh_missing()  # (a model with missing variables: the monitor kernel reads them as rows, like the step)
        mesh = V.mesh
        rows = StateArray(self.v_ode._ctx, len(names), self.num_points, mesh.plane if V.is_p1 else 0)
        self._dev.monitor_rows(names, t, rows.ptr, rows.ld)
        if out is None:  # each new function owns its row of the kernel's output
            out = [grid.Function(V, name=nm, field=rows.row_field(j)) for j, nm in enumerate(names)]
        else:
            for j, f in enumerate(out):
                f.writable_field().copy_from(rows.row_field(j))
        for f in out:
            f._touch()
        return out

    @property
    def full_values(self):
        return self.values

    def set_values(self, values) -> None:
        """Overwrite the whole (S, N) state array (e.g. with a pre-paced steady state)."""
        values = np.asarray(values, dtype=np.float64)
        if self.on_device:
            self._release_aliases()
            self._dev.set_states(np.broadcast_to(values.reshape(self.num_states, -1), self.shape))
        else:
            self._values[:] = values.reshape(self.num_states, -1)

    def assign_all_states(self, functions: list[grid.Function]) -> None:
        vals = self.values
        assert len(functions) == vals.shape[0], "Number of functions must match number of states"
        for index, f in enumerate(functions):
            f.x.array[:] = vals[index, :]

    def states_to_dolfin(self, names: list[str] | None = None) -> list[grid.Function]:
        V = self.v_ode.function_space
        num_states = self.num_states
        if names is not None:
            msg = f"Number of names must match number of states, got {len(names)} names, but number of states is {num_states}"
            assert len(names) == num_states, msg
        else:
            names = [f"state_{i}" for i in range(num_states)]
        functions = [grid.Function(V, name=name) for name in names]
        self.assign_all_states(functions)
        return functions


@dataclass
class DolfinMultiODESolver(BaseDolfinODESolver):
    """One cell model / parameter set per marker value (odesolver.py:228-354)."""

    v_ode: grid.Function
    v_pde: grid.Function
    markers: grid.Function
    init_states: dict
    parameters: dict
    fun: dict
    num_states: dict
    v_index: dict
    monitor: BaseMonitor = field(default_factory=NullMonitor)

    def __post_init__(self):
        if self.v_ode.x.array.size != self.markers.x.array.size:
            raise RuntimeError("Marker and voltage need to be in the same function space")
        self._marker_values = tuple(self.init_states.keys())
        marker_arr = np.asarray(self.markers.x.array)
        self._num_points, self._inds, self._idx_dev, self._odes, self._values = {}, {}, {}, {}, {}
        ctx = self.v_ode._ctx
        self._ctx = ctx
        self.on_device = all(isinstance(f, DeviceModel) for f in self.fun.values())
        if self.on_device:
            for f in self.fun.values():
                if f.num_missing_variables:
                    raise NotImplementedError(f"{f.name} has missing variables: DolfinMultiODESolver takes none (nor does the reference's); "
                                              "use one DolfinODESolver per half")
            for f in self.fun.values():  # models generated from .ode files get their ids now (markers sharing one are compared below)
                if hasattr(f, "register"):
                    f.register()
        self._initialize_full_values()
        telemetry = self.monitor  # (the per-marker solvers below take the telemetry monitor itself)
        self.monitor = _CallableMonitor(telemetry, self.monitor_values)
        self._marked = self.on_device and self._one_launch_possible()
        if self._marked:
            self._setup_one_launch(marker_arr)
            self._initialize_metadata()
            return
        for marker in self._marker_values:
            where = marker_arr == marker
            n_m = int(where.sum())
            self._num_points[marker] = n_m
            self._inds[marker] = where
            values = _initial_values(self.init_states[marker], self.shape(marker), self.on_device)
            if self.on_device:
                dev = _DeviceODE(ctx, self.fun[marker], self.num_states[marker], n_m, 0, self.parameters[marker],
                                 telemetry)
                dev.set_initial(values)
                self._odes[marker] = dev
                self._idx_dev[marker] = ctx.from_numpy(np.nonzero(where)[0].astype(np.int64))
            else:
                self._values[marker] = values
                self._odes[marker] = ODESystemSolver(fun=self.fun[marker], states=values,
                                                     parameters=self.parameters[marker], monitor=telemetry)
        self._initialize_metadata()

    # ---- one launch for all markers (the markers share one device model: cell types, parameter regions) ----------------
    def _one_launch_possible(self) -> bool:
        """All markers run the same built-in model with uniform (1-D) parameter sets on the PDE's P1 space: then the
        nodes live in ONE (S, N) state array with a byte per node naming the node's parameter set, and a step is one
        kernel launch (beat_ode_step_classes) instead of one per marker plus a scatter and a gather of the potential
        (BEAT_MULTI_ONE_LAUNCH=0 keeps the per-marker arrays: the reference's literal data layout)."""
        if os.environ.get("BEAT_MULTI_ONE_LAUNCH", "1") == "0":
            return False
        ms = self._marker_values
        funs = [self.fun[m] for m in ms]
        return (
            1 <= len(ms) <= _hip.MAX_CLASSES
            and all(f.model_id == funs[0].model_id for f in funs)
            and len({int(self.num_states[m]) for m in ms}) == 1
            and len({int(self.v_index[m]) for m in ms}) == 1
            and all(not isinstance(self.parameters[m], DeviceParameters) and np.ndim(self.parameters[m]) == 1 for m in ms)
            and self.v_ode.function_space.is_p1
        )

    def _setup_one_launch(self, marker_arr) -> None:
        ctx, ms = self._ctx, self._marker_values
        model, S, vi = self.fun[ms[0]], int(self.num_states[ms[0]]), int(self.v_index[ms[0]])
        n = marker_arr.size
        mesh = self.v_ode.function_space.mesh
        cls_full = np.full(n, 255, dtype=np.uint8)
        for k, marker in enumerate(ms):
            where = marker_arr == marker
            self._inds[marker] = where
            self._num_points[marker] = int(where.sum())
            cls_full[where] = k
        self._marked_any = cls_full != 255
        self._all_marked = bool(self._marked_any.all())
        self._idx_all = None if self._all_marked else ctx.from_numpy(np.nonzero(self._marked_any)[0].astype(np.int64))
        # Layout.  The ionic kernels are bound by fp64 issue: a lane without a cell costs what a busy one does.  When the
        # nodes that carry a model are a fraction of the grid (the wall of a voxelised geometry inside its box: 26 %) the
        # state array holds only those -- plus any other node of the tissue, which still diffuses -- and a node map
        # tells the kernel where each one's potential lives in the PDE's field; otherwise the array spans the grid and
        # its potential row IS that field.  BEAT_MULTI_COMPACT = 0 | 1 forces one or the other.
        tissue = mesh.node_active() if mesh.active is not None else np.ones(n, dtype=bool)
        held = self._marked_any | tissue
        # wavefronts (64 consecutive nodes) that would meet more than one class: each costs one pass per class
        seg = np.full(((n + 63) // 64) * 64, 255, dtype=np.uint8)
        seg[:n] = cls_full
        seg = seg.reshape(-1, 64)
        present = np.zeros(len(seg), dtype=np.int64)
        for k in range(len(ms)):
            present += (seg == k).any(axis=1)
        mixed = float((present > 1).sum()) / max(1, int((present > 0).sum()))
        want = os.environ.get("BEAT_MULTI_COMPACT")
        compact = (held.mean() < 0.9 or mixed > 0.05) if want is None else (want == "1")
        self._vi = vi
        if compact:
            # one run of whole 256-node tiles per class (then the tissue nodes without a model), nodes ascending inside a run
            tile = 256
            runs = [(k, np.nonzero(self._inds[m])[0]) for k, m in enumerate(ms)]
            rest = np.nonzero(held & ~self._marked_any)[0]
            if rest.size:
                runs.append((255, rest))
            node_parts, cls_parts, pos, real_pos, off = [], [], {}, [], 0
            for k, nodes in runs:
                pad = (-nodes.size) % tile
                node_parts += [nodes, np.zeros(pad, dtype=np.int64)]
                cls_parts += [np.full(nodes.size, k, dtype=np.uint8), np.full(pad, 254, dtype=np.uint8)]
                if k != 255:
                    pos[ms[k]] = off + np.arange(nodes.size)
                real_pos.append(off + np.arange(nodes.size))
                off += nodes.size + pad
            node_idx = np.concatenate(node_parts)
            cls = np.concatenate(cls_parts)
            real_pos = np.concatenate(real_pos)
            if node_idx.size == 0 or node_idx.max() >= 2**31:
                raise ValueError("the node map holds 32-bit indices")
            n_c = int(node_idx.size)
            self._dev = _DeviceODE(ctx, model, S, n_c, 0, None, self.monitor.telemetry)
            self._v_row = ctx.field(n, mesh.plane)  # the potential's home: a field of the PDE grid
            self._v_row.copy_from(self.v_ode.field)  # nodes outside every marker keep the potential they have
            self._real_pos = ctx.from_numpy(real_pos.astype(np.int64))       # entries of the array that are nodes ...
            self._real_nodes = ctx.from_numpy(node_idx[real_pos].astype(np.int64))  # ... and the nodes they are
            self._node_idx = self._real_nodes
            self._dev.node_map = (ctx.from_numpy(node_idx.astype(np.int32)), self._v_row)
        else:
            self._dev = _DeviceODE(ctx, model, S, n, mesh.plane, None, self.monitor.telemetry)
            self._v_row = self._dev.states.row_field(vi)
            self._v_row.copy_from(self.v_ode.field)
            self._node_idx = None
            cls = cls_full
            pos = {m: np.nonzero(self._inds[m])[0] for m in ms}
        rows = self._dev.states.rows  # (S, n) view of the device array: filled there (tens of GB at full size, not a host array)
        self._idx_dev = {}
        for marker in ms:
            idx = ctx.from_numpy(pos[marker].astype(np.int64))
            self._idx_dev[marker] = idx
            init = np.asarray(self.init_states[marker], dtype=np.float64)
            if init.ndim == 1:  # (S,) broadcast to the marker's nodes (odesolver.py:149-153)
                for r in range(S):
                    rows[r].index_fill_(0, idx, float(init[r]))
            else:
                if init.shape != self.shape(marker):
                    raise ValueError(f"init_states[{marker}] has shape {init.shape}, expected {self.shape(marker)}")
                rows.index_copy_(1, idx, ctx.from_numpy(np.ascontiguousarray(init)))
        if compact:  # the marked nodes' initial potential goes to its home (the others keep what v_ode held)
            for marker in ms:
                nodes = ctx.from_numpy(np.nonzero(self._inds[marker])[0].astype(np.int64))
                self._v_row.data.index_copy_(0, nodes, rows[vi].index_select(0, self._idx_dev[marker]))
        self._cls_dev = ctx.from_numpy(cls)
        self._dev.set_classes(self._cls_dev, [self.parameters[m] for m in ms])
        self._odes = {}

    def _refresh_compact_v(self) -> None:
        """Compact layout: the potential row of the state array mirrors the field only as of the last ionic launch."""
        if self._marked and self._node_idx is not None:
            self._sync_v()
            self._dev.states.rows[self._vi].index_copy_(0, self._real_pos, self._v_row.data.index_select(0, self._real_nodes))

    def _fused_prepare(self) -> int:
        """Called by the fused split step before the ionic launch: refresh the class table if a parameter set was
        edited; returns the potential's row."""
        self._dev.set_classes(self._cls_dev, [self.parameters[m] for m in self._marker_values])
        return self._vi

    def _masked_copy(self, dst, src) -> None:
        """dst[i] = src[i] on the nodes that carry a marker (all of them: a plain copy)."""
        if self._all_marked:
            dst.copy_from(src)
            return
        lib, n_m = self._ctx.lib, int(self._idx_all.numel())
        tmp = self._ctx.zeros(n_m)
        _hip.check(lib.beat_gather(self._ctx.handle, C.c_void_p(tmp.data_ptr()), src.ptr, C.c_void_p(self._idx_all.data_ptr()), n_m))
        _hip.check(lib.beat_scatter(self._ctx.handle, dst.ptr, C.c_void_p(tmp.data_ptr()), C.c_void_p(self._idx_all.data_ptr()), n_m))

    def _initialize_full_values(self):
        ns = tuple(self.num_states.values())
        self._all_states_equal_size = bool((np.array(ns) == ns[0]).all())
        if self._all_states_equal_size:
            self._full_values = np.zeros((ns[0], self.markers.x.array.size))

    def _each_v_row(self, scatter: bool, field) -> None:
        """Per-marker arrays: every marker's potential row is scattered to ``field`` (``scatter``) or gathered from it."""
        move = self._ctx.lib.beat_scatter if scatter else self._ctx.lib.beat_gather  # (both: destination, source, indices, count)
        for marker in self._marker_values:
            row = self._odes[marker].states.row_field(self.v_index[marker])
            dst, src = (field, row) if scatter else (row, field)
            _hip.check(move(self._ctx.handle, dst.ptr, src.ptr, C.c_void_p(self._idx_dev[marker].data_ptr()), row.n))

    def to_dolfin(self) -> None:
        if self._marked:
            if self.v_ode._alias is self._v_row:
                return
            self._sync_v()
            self._masked_copy(self.v_ode.writable_field(overwrite_all=False), self._v_row)
            self.v_ode._touch()
        elif self.on_device:
            self._each_v_row(True, self.v_ode.writable_field(overwrite_all=False))
            self.v_ode._touch()
        else:
            arr = np.asarray(self.v_ode.x.array).copy()
            for marker in self._marker_values:
                arr[self._inds[marker]] = self._values[marker][self.v_index[marker], :]
            self.v_ode.x.array[:] = arr

    def scatter_v(self, dst) -> None:
        """Potentials of every marker's states -> field ``dst`` (fused split step)."""
        if self._marked:
            self._sync_v()
            return self._masked_copy(dst, self._v_row)
        self._each_v_row(True, dst)

    def gather_v(self, src) -> None:
        """Field ``src`` -> the potential rows of every marker's states (fused split step)."""
        if self._marked:
            self._release_aliases()
            return self._masked_copy(self._v_row, src)
        self._each_v_row(False, src)

    def from_dolfin(self) -> None:
        if self._marked:
            if self.v_ode._alias is self._v_row:
                return
            self._release_aliases()
            self._masked_copy(self._v_row, self.v_ode.field)
        elif self.on_device:
            self._each_v_row(False, self.v_ode.field)
        else:
            arr = np.asarray(self.v_ode.x.array)
            for marker in self._marker_values:
                self._values[marker][self.v_index[marker], :] = arr[self._inds[marker]]

    def values(self, marker: int):
        if self._marked:  # the marker's columns of the one state array, (S, N_marker) as the reference keeps them
            self._sync_v()
            self._refresh_compact_v()
            return self._dev.states.rows.index_select(1, self._idx_dev[marker]).cpu().numpy()
        return self._odes[marker].states.numpy() if self.on_device else self._values[marker]

    def set_values(self, marker: int, values) -> None:
        """Overwrite the (S, N_marker) states of one marker (e.g. with a pre-paced steady state)."""
        values = np.broadcast_to(np.asarray(values, dtype=np.float64).reshape(self.num_states[marker], -1), self.shape(marker))
        if self._marked:
            self._release_aliases()
            self._dev.states.rows.index_copy_(1, self._idx_dev[marker], self._ctx.from_numpy(np.ascontiguousarray(values)))
            if self._node_idx is not None:  # the potential's home is the field
                nodes = self._ctx.from_numpy(np.nonzero(self._inds[marker])[0].astype(np.int64))
                self._v_row.data.index_copy_(0, nodes, self._ctx.from_numpy(np.ascontiguousarray(values[self._vi])))
        elif self.on_device:
            self._odes[marker].states.set(np.ascontiguousarray(values))
        else:
            self._values[marker][:] = values

    def num_parameters(self, marker: int) -> int:
        return len(self.parameters[marker])

    def shape(self, marker: int) -> tuple[int, int]:
        return (self.num_states[marker], self._num_points[marker])

    def num_points(self, marker: int) -> int:
        return self._num_points[marker]

    def step(self, t0: float, dt: float):
        if self._marked:
            with self.monitor.track_time("total_ode_step"):
                self._release_aliases()
                self._dev.step(t0, dt, v_index=self._fused_prepare())
            return
        with self.monitor.track_time("total_ode_step"):
            for marker, ode in self._odes.items():
                with self.monitor.track_time(f"marker_{marker}_ode_step"):
                    if self.on_device:
                        ode.parameters = self.parameters[marker]
                        ode.step(t0, dt)
                    else:
                        ode.step(t0=t0, dt=dt)

    def monitor_values(self, names, t: float, out=None):
        raise NotImplementedError("monitor() is not available for DolfinMultiODESolver: use DolfinODESolver with one beat.models.from_ode model")

    # ---- state rows as functions of the grid, on the device -----------------------------------------------------------------
    def _rows_plan(self) -> _RowsPlan:
        """The rows plan over the state arrays as they lie now: built on first use, again if an array has moved."""
        from . import _rows_layout

        ms = self._marker_values
        if self._marked:
            states = self._dev.states
            bases, lds = (states.ptr.value,) * len(ms), (states.ld,) * len(ms)
        else:
            bases, lds = tuple(self._odes[m].states.ptr.value for m in ms), tuple(self._odes[m].states.ld for m in ms)
        plan = getattr(self, "_rows", None)
        if plan is not None and (plan.bases, plan.lds) == (bases, lds):
            return plan
        n = self.markers.x.array.size
        rows = [int(self.num_states[m]) for m in ms]
        if not self._marked:  # one array per marker
            layout, cls_dev = _rows_layout.marker_layout(n, [np.nonzero(self._inds[m])[0] for m in ms], rows), None
        elif self._node_idx is None:  # one array over the grid: its class bytes are the plan's
            cls_full = np.full(n, _rows_layout.NO_MODEL, dtype=np.uint8)
            for k, m in enumerate(ms):
                cls_full[self._inds[m]] = k
            layout, cls_dev = _rows_layout.grid_layout(cls_full, len(ms), rows), self._cls_dev
        else:  # one compact array: the node map and class bytes the ionic kernel reads
            layout, cls_dev = _rows_layout.compact_layout(n, self._dev.node_map[0].cpu().numpy(), self._cls_dev.cpu().numpy(), len(ms),
                                                          rows), None
        self._rows = _RowsPlan(self._ctx, layout, bases, lds, cls_dev)
        return self._rows

    def _key_rows(self, key) -> list[int]:
        """The row of every marker's states that ``key`` names: an int (the same row for every marker), a state name (each model's
        own row of it) or a dict marker -> int | name."""
        if isinstance(key, dict):
            if set(key) != set(self._marker_values):
                raise ValueError(f"a key per marker {self._marker_values} expected, got {tuple(key)}")
            per_marker = key
        else:
            per_marker = {m: key for m in self._marker_values}
        rows = []
        for m in self._marker_values:
            k, fun = per_marker[m], self.fun[m]
            if isinstance(k, str):
                if k not in fun.state_names:
                    raise ValueError(f"marker {m}: {fun.name} has no state {k!r} (it has {', '.join(fun.state_names)})")
                k = fun.state_index(k)
            k = int(k)
            if not 0 <= k < int(self.num_states[m]):
                raise IndexError(f"marker {m}: state {k} of {self.num_states[m]}")
            rows.append(k)
        return rows

    def _rows_device_only(self, what: str) -> None:
        if not self.on_device:
            raise NotImplementedError(f"{what} moves rows of the device's state arrays: fun is a host callable")
        if self.v_ode.function_space.mesh.comm.size > 1:
            raise NotImplementedError(f"{what} is not available on a decomposed mesh")

    def _is_v(self, rows) -> list[bool]:
        return [r == int(self.v_index[m]) for r, m in zip(rows, self._marker_values)]

    def _expand_rows(self, rows, fields, fill=None) -> None:
        """``fields[f]`` (device fields of the grid) from the rows ``rows[f]`` (one per marker) in as few launches as 8 fields each
        allow; a node without a marker keeps its value or gets ``fill``.  A potential row is completed first.  Does not wait."""
        if any(any(self._is_v(r)) for r in rows):
            self._sync_v()  # finish the open solve, apply what it deferred
            self._refresh_compact_v()  # (compact layout: the row mirrors the potential's home field as of the last ionic launch)
        self._rows_plan().expand(rows, fields, fill)

    def states_to_functions(self, keys, out: list[grid.Function] | None = None, outside: float | None = None) -> list[grid.Function]:
        """Row ``key`` of whatever model each node runs, as a function on ``v_ode``'s space, for every ``key`` in ``keys``: an int
        (the same row for every marker), a state name (``"V"`` may be a different row in each model) or a dict marker -> int |
        name.  One launch per 8 keys, on the device; returns without waiting.  ``out``: functions to write into instead of new
        ones.  A node outside every marker keeps what ``out`` holds (``outside=None``; a new function holds 0) or is set to
        ``outside``.  Equals ``values(marker)[row]`` on every marker's nodes."""
        self._rows_device_only("states_to_functions()")
        keys = list(keys)
        rows = [self._key_rows(k) for k in keys]
        if out is None:
            V = self.v_ode.function_space
            out = [grid.Function(V, name=k if isinstance(k, str) else f"state_{k}" if isinstance(k, int) else "state") for k in keys]
        elif len(out) != len(keys):
            raise ValueError(f"{len(keys)} keys, {len(out)} functions")
        n = self.markers.x.array.size
        for f in out:
            if f.num_values != n:
                raise ValueError(f"expected a function of {n} values, got {f.num_values}")
        if not keys:
            return out
        self._expand_rows(rows, [f.writable_field(overwrite_all=outside is not None) for f in out], outside)
        for f in out:
            f._touch()
        return out

    def state_to_function(self, key, out: grid.Function, outside: float | None = None) -> grid.Function:
        """``states_to_functions([key], [out], outside)[0]`` (the name ``DolfinODESolver`` has for it)."""
        return self.states_to_functions([key], [out], outside)[0]

    def function_to_state(self, key, src: grid.Function) -> None:
        """``src`` -> row ``key`` (see ``states_to_functions``) on the nodes that carry a marker, on the device: a restart from saved
        frames, a calcium field or a block region put into one state.  A potential row is written as ``from_dolfin`` writes it
        from ``v_ode``; in the compact layout a key that names the potential for some markers only is refused.  Returns without
        waiting."""
        self._rows_device_only("function_to_state()")
        rows = self._key_rows(key)
        if src.num_values != self.markers.x.array.size:
            raise ValueError(f"expected a function of {self.markers.x.array.size} values, got {src.num_values}")
        is_v = self._is_v(rows)
        compact = self._marked and self._node_idx is not None  # the potential's home is a field of the grid, not the row
        if compact and any(is_v) and not all(is_v):
            raise NotImplementedError("function_to_state() in the compact layout: a key that names the potential for some markers only")
        self._release_aliases()  # (a function that aliases the potential row -- src itself, maybe -- gets its own copy first)
        fld = src.field
        self._rows_plan().collapse([rows], [fld])
        if compact and all(is_v):
            self._masked_copy(self._v_row, fld)

    def assign_all_states(self, functions: list[grid.Function]) -> None:
        num_states = self.num_states[self._marker_values[0]]
        assert len(functions) == num_states, "Number of functions must match number of states"
        if self.on_device and self.v_ode.function_space.mesh.comm.size == 1:
            # one pass over the grid per 8 states (odesolver.py:312-339 pulls every marker's whole array through the host per state)
            self.states_to_functions(list(range(num_states)), functions)
            return
        for index, f in enumerate(functions):
            arr = np.asarray(f.x.array).copy()
            for marker in self._marker_values:
                arr[self._inds[marker]] = self.values(marker)[index, :]
            f.x.array[:] = arr

    def states_to_dolfin(self, names: list[str] | None = None) -> list[grid.Function]:
        V = self.v_ode.function_space
        num_states = self.num_states[self._marker_values[0]]
        if names is not None:
            assert len(names) == num_states, "Number of names must match number of states"
        else:
            names = [f"state_{i}" for i in range(num_states)]
        functions = [grid.Function(V, name=name) for name in names]
        self.assign_all_states(functions)
        return functions

    @property
    def full_values(self):
        if not self._all_states_equal_size:
            msg = ("Cannot get full values size states are not of equal size. "
                   f"Have {self.num_states=}, use .values(marker) instead")
            raise RuntimeError(msg)
        for marker in self._marker_values:
            self._full_values[:, self._inds[marker]] = self.values(marker)
        return self._full_values
