"""How a solver's cell-model parameters reach the ionic kernel.  A ``Route`` is one resolved decision,
``ParameterRoutes`` (one per ``_DeviceODE``) the only code that takes and caches one.  What touches the device or the library is
handed in as ``ops``: ``torch``, ``from_numpy(host array) -> tensor``, ``zeros(n) -> tensor``, ``class_table_doubles(model_id) -> int``,
``class_table_fill(model_id, (classes, P) host array, table)`` and ``jit_available() -> bool``, so the policy runs on the CPU with
CPU tensors and a recording stub (tests/test_param_route_cpu.py)."""

from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _hip
from .models._base import DeviceParameters, host_and_device_parameters, parameter_args


class Route(NamedTuple):
    """``kind`` and the data that kind needs (the objects themselves: a route keeps alive what the kernel will read)."""

    kind: str                      # "none" | "uniform" | "classes" | "rows" | "per_node"
    vector: np.ndarray | None = None  # "uniform": the host (P,) vector
    classes: tuple | None = None   # "classes": (marker bytes on the device, class table, number of classes)
    rows: tuple | None = None      # "rows": (uniform host vector, int32 indices of the varying rows, their (K, N) device rows)
    per_node: tuple | None = None  # "per_node": ((P, N) device tensor, P, ld)
    fallback: "Route | None" = None  # "classes" / "rows" derived from per-node parameters: the per-node route of the same array

    def args(self):
        """The parameter arguments of the kind's entry point.  beat_ode_step_classes: (class table, number of classes, marker bytes);
        beat_ode_step_rows: (uniform vector, P, row indices, K, rows, ld); beat_ode_step / _pending: (vector, P, per-node rows, ld)."""
        if self.kind == "classes":
            markers, table, count = self.classes
            return C.c_void_p(table.data_ptr()), count, C.c_void_p(markers.data_ptr())
        if self.kind == "rows":
            uni, idx, rows = self.rows
            return (uni.ctypes.data_as(C.c_void_p), len(uni), idx.ctypes.data_as(C.c_void_p), len(idx), C.c_void_p(rows.data_ptr()),
                    rows.shape[1])
        tensor, num, ld = self.per_node or (None, 0 if self.vector is None else len(self.vector), 0)
        return parameter_args(self.vector, tensor, ld, num)

    def monitor_kwargs(self) -> dict:
        """The parameter keywords of ``monitor_on_device`` (varying rows are read whole: a generated model has no sparse-row instance)."""
        per_node = (self.fallback if self.kind == "rows" else self).per_node
        return dict(host_params=self.vector, per_node=None if per_node is None else (per_node[0], per_node[2]), classes=self.classes)


class ParameterRoutes:
    def __init__(self, name: str, num_parameters: int, model_id: int, n: int, ops):
        self.name, self.num_parameters, self.model_id, self.n, self.ops = name, int(num_parameters), int(model_id), int(n), ops
        self.current = Route("none")  # the route last resolved or set
        self.explicit = False   # the owner set the classes itself (set_classes): the parameters are not consulted
        self._host = None       # copy of the live NumPy array ``current`` was derived from (its upload lives in the route)
        self._handle = self._version = None  # the DeviceParameters handle ``current`` was derived from (the object: an id() comes back), its version then
        self._sets = None       # (classes, P) host copy of what the class table holds

    def set_classes(self, markers, sets) -> Route:
        """One launch for several uniform parameter sets (beat_ode_step_classes): ``markers`` = a byte per node on the device naming
        its set (255: none, the node is not advanced), ``sets`` = the sets in class order.  Calling it again with the same number of
        sets only refreshes the table, and only if a set changed (the reference hands ``fun`` the live parameter arrays every step,
        odesolver.py:70-76).  From here on ``resolve`` answers with these classes whatever the parameters."""
        self.current = self._class_route(markers, sets, None)
        self.explicit, self._host, self._handle = True, None, None
        return self.current

    def _class_route(self, markers, sets, fallback) -> Route:
        P = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64) for p in sets]))
        if P.ndim != 2 or P.shape[1] != self.num_parameters or not 1 <= P.shape[0] <= _hip.MAX_CLASSES:
            raise ValueError(f"{self.name}: {P.shape[0]} parameter sets of {P.shape[1:]} values "
                             f"(expected 1..{_hip.MAX_CLASSES} sets of {self.num_parameters})")
        if self.current.kind == "classes" and self.current.classes[2] == P.shape[0]:
            table = self.current.classes[1]
        else:
            table = self.ops.zeros(self.ops.class_table_doubles(self.model_id) * P.shape[0])
            self._sets = None
        if self._sets is None or not np.array_equal(self._sets, P):
            self.ops.class_table_fill(self.model_id, P, table)
            self._sets = P.copy()
        return Route("classes", classes=(markers, table, P.shape[0]), fallback=fallback)

    def _classify(self, t):
        """Per-node parameters (P, N) that are piecewise constant -- demos/pace_train.py:133-167 zeroes two conductances in half of
        the cable -- are a handful of uniform parameter sets: the distinct columns become classes, a byte per node names its class,
        and the step runs the class kernel (uniform parameters in scalar registers, no per-node rows to load: 424 B/node for TP06,
        896 for ToR-ORd) instead of the per-node one.  Returns (marker bytes on the device, (classes, P) host array) or None when
        the columns are not few (a smooth gradient: per-node kernel).  BEAT_PARAM_CLASSES=0 turns the analysis off."""
        if os.environ.get("BEAT_PARAM_CLASSES", "1") == "0":
            return None
        torch = self.ops.torch
        varying = (t != t[:, :1]).any(dim=1)
        n = t.shape[1]
        if not bool(varying.any()):
            return torch.zeros(n, dtype=torch.uint8, device=t.device), t[:, :1].T.cpu().numpy()
        cols = t[varying]
        stride = max(1, n // 65536)  # a sample first: a smooth field shows at once
        if torch.unique(cols[:, ::stride], dim=1).shape[1] > _hip.MAX_CLASSES:
            return None
        uniq, inv = torch.unique(cols, dim=1, return_inverse=True)
        if uniq.shape[1] > _hip.MAX_CLASSES:
            return None
        first = torch.full((uniq.shape[1],), n, dtype=torch.int64, device=t.device)
        first.scatter_reduce_(0, inv, torch.arange(n, device=t.device), reduce="amin")
        return inv.to(torch.uint8), t[:, first].T.contiguous().cpu().numpy()

    def _derive(self, tensor) -> Route:
        """The route of per-node parameters held in ``tensor``: classes if they allow it, else -- when at most sixteen ROWS vary
        over the nodes (smooth gradients in a few conductances; four without run-time compilation) -- those rows alone next to
        the uniform vector (beat_ode_step_rows reads 8 B per varying row and node instead of 8 P), else all P rows."""
        per_node = Route("per_node", per_node=(tensor, self.num_parameters, self.n))
        found = self._classify(tensor)
        if found is not None:  # (the fallback: for the caller the class kernel does not serve, a mirror of another row than V)
            return self._class_route(found[0], list(found[1]), per_node)
        # (a model registered as source has no compiled sparse-row instance: all its rows are read)
        if os.environ.get("BEAT_PARAM_SPARSE", "1") != "0" and tensor.shape[1] == self.n and self.model_id < _hip.CUSTOM_MODEL_BASE:
            varying = (tensor != tensor[:, :1]).any(dim=1)
            idx = varying.nonzero().flatten().cpu().numpy().astype(np.int32)
            # (up to 16 varying rows on a kernel instance compiled for their indices, 4 where that cannot be had)
            jit = os.environ.get("BEAT_JIT", "1") != "0" and self.ops.jit_available()
            if 1 <= len(idx) <= (_hip.MAX_SPARSE_ROWS if jit else _hip.MAX_SPARSE_ROWS_RT):
                rows = tensor[varying].contiguous()  # (K, N): the only parameter data a step reads from memory
                uniform = np.ascontiguousarray(tensor[:, 0].cpu().numpy(), dtype=np.float64)
                return Route("rows", rows=(uniform, np.ascontiguousarray(idx), rows), fallback=per_node)
        return per_node

    def resolve(self, p) -> Route:
        """The route of the parameters ``p`` as they are now: None, a (P,) vector, a live (P, N) NumPy array or a DeviceParameters
        handle.  A vector or an unchanged handle costs no device work; neither cache outlives a route that was not derived from it
        (a classified array, then a vector, then the same array classifies again)."""
        if self.explicit:
            return self.current
        checked = (self.ops, p, self.num_parameters, self.n)  # (host_and_device_parameters refuses any other shape, and uploads)
        if isinstance(p, DeviceParameters):  # resident handle: nothing to check or move per step
            if self._handle is not p or self._version != p.version:  # new values: look at them once
                self._host = None  # (the route now follows THIS handle: the NumPy array's cache is stale)
                self.current = self._derive(host_and_device_parameters(*checked)[1])
                self._handle, self._version = p, p.version
        elif p is None or np.ndim(p) == 1:
            hp = host_and_device_parameters(*checked)[0]
            self._host = self._handle = None
            self.current = Route("none") if hp is None else Route("uniform", vector=hp)
        else:
            # per-node NumPy parameters: the reference hands the live array to ``fun`` every step (odesolver.py:70-76), so any in-place
            # edit must reach the kernel.  Exact comparison with the copy that was uploaded (one host pass per step; a handle avoids it).
            p = np.asarray(p, dtype=np.float64)
            if self._host is None or self._host.shape != p.shape or not np.array_equal(self._host, p):
                self.current = self._derive(host_and_device_parameters(*checked)[1])
                self._host, self._handle = p.copy(), None
        return self.current
