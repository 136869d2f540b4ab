"""Field snapshots for ParaView or NumPy, taken on the device and written BEHIND the time loop.

Every tissue demo of the reference has the same ``save(t)`` in its loop, once per millisecond of simulated time
(demos/niederer_benchmark.py:226-277, demos/slab.py:284-299, demos/lv_endocardial.py:311-326, demos/biv_endocardial.py:299-314,
demos/ukb_atlas.py:386-418, demos/fitzhughnagumo.py:252-301): ``vtx.write(t)``, ``io4dolfinx.write_function(..., solver.pde.state,
time=t, name="v")`` and ``print(v.max(), v.min())``.  Through ``beat.io.write_function`` that is a flush of the potential's
deferred update, a synchronous copy of the whole fp64 field and a disk write on the thread that drives the GPU.  ``FieldWriter``
takes the frame in one launch (beat_snap_*: cropped to a box, down-sampled, converted to fp32 if asked; the same pass yields min, max
and the number of non-finite values), copies it to pinned host memory on a stream of its own while the loop goes on, and a host
thread writes it: VTK ImageData (``.vti`` per frame and a ``.pvd`` time index, which ParaView opens as it is) or ``.npy``.

The functions that write files (``write_vti``, ``write_pvd``, ``FrameFiles``) take NumPy arrays and need no GPU and no VTK library."""

from __future__ import annotations

import ctypes as C
import json
import math
import os
import queue
import threading
from pathlib import Path

import numpy as np

from . import _hip

FORMATS = ("vti", "npy")
_DTYPES = {"float64": 0, "float32": 1}
_VTK_TYPES = {"float32": "Float32", "float64": "Float64"}


# ---- files: NumPy in, no device -----------------------------------------------------------------------------------------------
def _replace_text(path: Path, text: str) -> None:
    """``path`` holds ``text`` or what it held before, never a part of either (a temporary file beside it, then os.replace)."""
    tmp = path.with_name(path.name + ".tmp")
    tmp.write_text(text)
    os.replace(tmp, path)


def _pad3(values, fill):
    values = [float(v) for v in values]
    return values + [fill] * (3 - len(values))


def write_vti(path, arrays: dict, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)) -> None:
    """One VTK ImageData file with the point data ``arrays`` (name -> array of shape (nz, ny, nx), (ny, nx) or (nx,), all alike, float32
    or float64; x runs fastest), raw appended: per array a UInt64 byte count and the bytes, ``offset`` counted from the byte after
    the ``_``.  ``origin`` and ``spacing`` per used axis (x first); unused axes have extent ``0 0``."""
    if not arrays:
        raise ValueError("write_vti needs at least one array")
    arrays = {str(k): np.ascontiguousarray(a) for k, a in arrays.items()}
    first = next(iter(arrays.values()))
    if not 1 <= first.ndim <= 3:
        raise ValueError(f"arrays of 1 to 3 dimensions expected, got shape {first.shape}")
    for name, a in arrays.items():
        if a.shape != first.shape:
            raise ValueError(f"array {name!r} has shape {a.shape}, the first one {first.shape}")
        if a.dtype.name not in _VTK_TYPES:
            raise ValueError(f"array {name!r} is {a.dtype}: float32 or float64 expected")
    nx, ny, nz = list(reversed(first.shape)) + [1] * (3 - first.ndim)
    extent = f"0 {nx - 1} 0 {ny - 1} 0 {nz - 1}"
    fmt = lambda v: " ".join(repr(x) for x in v)  # noqa: E731
    lines = ['<?xml version="1.0"?>',
             '<VTKFile type="ImageData" version="1.0" byte_order="LittleEndian" header_type="UInt64">',
             f'  <ImageData WholeExtent="{extent}" Origin="{fmt(_pad3(origin, 0.0))}" Spacing="{fmt(_pad3(spacing, 1.0))}">',
             f'    <Piece Extent="{extent}">',
             f'      <PointData Scalars="{next(iter(arrays))}">']
    offset = 0
    for name, a in arrays.items():
        lines.append(f'        <DataArray type="{_VTK_TYPES[a.dtype.name]}" Name="{name}" format="appended" offset="{offset}"/>')
        offset += 8 + a.nbytes
    lines += ["      </PointData>", "    </Piece>", "  </ImageData>", '  <AppendedData encoding="raw">', "   _"]
    with open(path, "wb") as fh:
        fh.write("\n".join(lines).encode("ascii"))
        for a in arrays.values():
            fh.write(np.uint64(a.nbytes).astype("<u8").tobytes())
            fh.write(a.astype(a.dtype.newbyteorder("<"), copy=False).data)
        fh.write(b"\n  </AppendedData>\n</VTKFile>\n")


def write_pvd(path, entries) -> None:
    """The time index ParaView opens: ``entries`` = [(time, file name relative to the .pvd), ...].  Replaced as a whole."""
    lines = ['<?xml version="1.0"?>', '<VTKFile type="Collection" version="0.1" byte_order="LittleEndian">', "  <Collection>"]
    lines += [f'    <DataSet timestep="{float(t)!r}" group="" part="0" file="{name}"/>' for t, name in entries]
    lines += ["  </Collection>", "</VTKFile>", ""]
    _replace_text(Path(path), "\n".join(lines))


def _json_number(x):
    x = float(x)
    return x if math.isfinite(x) else None  # (JSON has no NaN)


class FrameFiles:
    """The files of one run.  ``format="vti"``: ``<path>_<k:06d>.vti`` per frame with all fields, and ``<path>.pvd``;
    ``format="npy"``: the directory ``path`` with ``<name>_<k>.npy`` of shape (nz, ny, nx) per field and frame, and ``index.json``
    (times, statistics, origin, spacing, stride, box).  The index is rewritten after every frame through a temporary file, so a run
    that dies leaves a valid index of what it wrote.  Directories are made when the first frame arrives."""

    def __init__(self, path, names, format="vti", origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), stride=(1, 1, 1), box=None):
        if format not in FORMATS:
            raise ValueError(f"format must be one of {FORMATS}, got {format!r}")
        self.path = Path(path)
        self.names = tuple(str(n) for n in names)
        self.format = format
        self.origin, self.spacing = [float(v) for v in origin], [float(v) for v in spacing]
        self.stride = [int(s) for s in stride]
        self.box = None if box is None else [[int(a), int(b)] for a, b in box]
        self.times, self.stats, self.files = [], [], []
        self.closed = False

    @property
    def index_path(self) -> Path:
        return self.path.with_name(self.path.name + ".pvd") if self.format == "vti" else self.path / "index.json"

    def add(self, t, arrays: dict, stats: dict | None = None) -> None:
        """Frame number len(self.times): ``arrays`` name -> array, ``stats`` name -> (min, max, nonfinite)."""
        if self.closed:
            raise ValueError("these frame files are closed")
        if tuple(arrays) != self.names:
            raise ValueError(f"fields {tuple(arrays)} given, {self.names} expected")
        k = len(self.times)
        if self.format == "vti":
            self.path.parent.mkdir(parents=True, exist_ok=True)
            name = f"{self.path.name}_{k:06d}.vti"
            write_vti(self.path.parent / name, arrays, self.origin, self.spacing)
            self.files.append(name)
        else:
            self.path.mkdir(parents=True, exist_ok=True)
            for field, a in arrays.items():
                np.save(self.path / f"{field}_{k}.npy", np.asarray(a))
            self.files.append({field: f"{field}_{k}.npy" for field in arrays})
        self.times.append(float(t))
        self.stats.append({n: [_json_number(v) for v in (stats or {}).get(n, (float("nan"), float("nan"), -1))] for n in self.names})
        self._write_index()

    def _write_index(self) -> None:
        if self.format == "vti":
            write_pvd(self.index_path, list(zip(self.times, self.files)))
        else:
            _replace_text(self.index_path, json.dumps({
                "fields": list(self.names), "times": self.times, "stats": self.stats, "files": self.files, "origin": self.origin,
                "spacing": self.spacing, "stride": self.stride, "box": self.box}))

    def close(self) -> None:
        """The final index (a run without frames leaves an empty one, if its directory exists).  Idempotent."""
        if self.closed:
            return
        self.closed = True
        if self.times or self.index_path.parent.is_dir():
            self._write_index()


# ---- the lattice: what the arguments mean ----------------------------------------------------------------------------------------
def lattice(shape, stride=1, box=None):
    """(lo, hi, stride, samples) per axis of a grid of ``shape`` nodes (x first, 1 to 3 axes): ``stride`` an int or one per axis,
    ``box`` None (the whole grid) or a (lo, hi) range of node indices per axis, as the slice lo:hi:stride takes them."""
    shape = [int(n) for n in shape]
    dim = len(shape)
    strides = [stride] * dim if np.ndim(stride) == 0 else list(stride)
    if len(strides) != dim:
        raise ValueError(f"stride has {len(strides)} entries for {dim} axes")
    if any(int(s) != s or int(s) < 1 for s in strides):
        raise ValueError(f"a stride is a positive integer, got {stride!r}")
    box = [(0, n) for n in shape] if box is None else [tuple(r) for r in box]
    if len(box) != dim or any(len(r) != 2 for r in box):
        raise ValueError(f"box is one (lo, hi) range of node indices per axis ({dim} here), got {box!r}")
    for a, ((lo, hi), n) in enumerate(zip(box, shape)):
        if int(lo) != lo or int(hi) != hi or not 0 <= lo < hi <= n:
            raise ValueError(f"box range {(lo, hi)} of axis {a}: 0 <= lo < hi <= {n} expected")
    lo, hi, strides = [int(r[0]) for r in box], [int(r[1]) for r in box], [int(s) for s in strides]
    return lo, hi, strides, [len(range(a, b, s)) for a, b, s in zip(lo, hi, strides)]


# ---- the writer -----------------------------------------------------------------------------------------------------------------
class FieldWriter:
    """``FieldWriter(path, fields, stride=1, dtype="float32", box=None, outside=nan, format="vti", depth=2, stats=True, time=None,
    every=1)``

    ``fields``: name -> a scalar P1 ``grid.Function`` (the potential ``pde.state``, an event map ``rec.activation``, ...) or
    ``(DolfinODESolver, state name or index)`` for a row of a device model's state array that spans the grid, read in place, or
    ``(DolfinMultiODESolver, key)`` -- ``key`` an int, a state name or a dict marker -> int | name, as ``states_to_functions`` takes
    it: the row of whatever model a node runs, expanded per frame into a staging field the writer owns (all such sources of a solver
    in one launch, ahead of the frame's).  A node without a cell model gets ``outside`` there -- a TISSUE node without a model too,
    which then counts as non-finite in the statistics when ``outside`` is NaN.  All on one undivided mesh; at most 8.  ``stride`` (an int or one per axis) and ``box`` (a (lo, hi) range of node indices per axis)
    choose the nodes ``lo:hi:stride``; on a voxel mesh a sample outside the tissue gets ``outside``.  ``dtype``: ``"float32"`` (rounded
    to nearest even, as ``numpy.float32``) or ``"float64"``.  ``format``: see ``FrameFiles``.  Origin = mesh.lower + lo h, spacing = h
    stride.

    ``write(t)`` enqueues a frame of the fields as they are now and returns without waiting for the device: one launch on the
    compute stream, the copy on the writer's own stream, the file from the writer's thread.  A function is read through its
    ``field``, which applies a pending deferred update of the potential first: that finishes the solve ``step()`` left open -- one
    host wait per FRAME, not per step (so is ``_sync_v()`` for the potential row of an ODE solver).  ``write`` blocks only when all
    ``depth`` slots are in flight, until the oldest has been written.  As a recorder (``solver.solve(..., recorder=[rec, w])``)
    ``record()`` is called every step and writes every ``every``-th one at t = float(``time``) -- ``pde.time`` holds t0 + theta dt of
    the last step, the time the PDE took its stimulus at; a callable is called; without ``time`` t counts the steps.

    ``frames``: [(t, {name: (min, max, nonfinite)}), ...] of the frames written so far -- over ALL tissue nodes of the box, sampled
    or not (``stats=False``: (nan, nan, -1), and the pass reads the sampled rows only); NaN is counted and ignored by min and max.
    An exception in the writer's thread is raised by the next ``write()`` or ``close()``.  ``close()`` drains and leaves the final
    index; it is idempotent, and the writer is a context manager."""

    def __init__(self, path, fields, stride=1, dtype="float32", box=None, outside=float("nan"), format="vti", depth=2, stats=True,
                 time=None, every=1, nontemporal=False):
        from . import grid
        from .odesolver import BaseDolfinODESolver, DolfinODESolver

        self._snap = None
        self._closed = True  # (until everything is made: __del__ of a writer whose constructor raised has nothing to close)
        if format not in FORMATS:
            raise ValueError(f"format must be one of {FORMATS}, got {format!r}")
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be 'float32' or 'float64', got {dtype!r}")
        if int(depth) != depth or not 1 <= depth <= _hip.SNAP_MAX_DEPTH:
            raise ValueError(f"depth must be 1..{_hip.SNAP_MAX_DEPTH}, got {depth!r}")
        if int(every) != every or every < 1:
            raise ValueError(f"every must be a positive integer, got {every!r}")
        if not isinstance(fields, dict) or not 1 <= len(fields) <= _hip.SNAP_MAX_FIELDS:
            raise ValueError(f"fields must be a dict of 1..{_hip.SNAP_MAX_FIELDS} entries, name -> function or (ode solver, state)")
        mesh = None
        sources = []
        for name, src in fields.items():
            if not isinstance(name, str) or not name or any(c in name for c in '"<>&/\\'):
                raise ValueError(f"a field name is a non-empty string without quotes, angle brackets, & or slashes, got {name!r}")
            if isinstance(src, (grid.VectorFunction, grid.CellFunction)):
                raise NotImplementedError(f"field {name!r}: vector and cell functions are not written, only scalar P1 functions")
            if isinstance(src, grid.Function):
                if not src.function_space.is_p1:
                    raise NotImplementedError(f"field {name!r}: a {src.function_space.family} {src.function_space.degree} function "
                                              "does not live on the grid's nodes; only scalar P1 functions are written")
                m, entry = src.function_space.mesh, ("function", src)
            elif isinstance(src, tuple) and len(src) == 2 and isinstance(src[0], BaseDolfinODESolver):
                ode, key = src
                if not ode.on_device:
                    raise NotImplementedError(f"field {name!r}: the ODE solver runs a host callable; its states are not on the device")
                if not ode.v_ode.function_space.is_p1:
                    raise NotImplementedError(f"field {name!r}: the ODE solver's space is not P1, its rows do not span the grid's nodes")
                m = ode.v_ode.function_space.mesh
                if isinstance(ode, DolfinODESolver):  # a row of the one state array, read in place
                    if isinstance(key, str):
                        if key not in ode.fun.state_names:
                            raise ValueError(f"field {name!r}: {ode.fun.name} has no state {key!r} (it has {', '.join(ode.fun.state_names)})")
                        key = ode.fun.state_index(key)
                    k = int(key)
                    if not 0 <= k < ode.num_states:
                        raise ValueError(f"field {name!r}: state {key!r} of {ode.num_states}")
                    entry = ("row", ode, k, ode._dev.states.row_field(k))
                else:  # a multi-model solver: the rows are expanded per frame into a staging field, made below behind the checks
                    try:
                        rows = ode._key_rows(key)
                    except (ValueError, IndexError) as exc:
                        raise ValueError(f"field {name!r}: {exc}") from None
                    ode._rows_device_only("FieldWriter")
                    entry = ("multi", ode, rows)
            else:
                raise ValueError(f"field {name!r}: a scalar P1 grid.Function or (DolfinODESolver, state) expected, got {type(src).__name__}")
            if mesh is not None and m is not mesh:
                raise ValueError(f"field {name!r} lives on another mesh than the fields before it")
            mesh = m
            sources.append(entry)
        if mesh.comm.size > 1:
            raise NotImplementedError("FieldWriter on a decomposed mesh: a piece per rank and a .pvti over them are not built")
        lo, hi, strides, ns = lattice(mesh.shape_global[: mesh.dim], stride, box)
        self.names = tuple(fields)
        self.mesh = mesh
        self.shape = tuple(reversed(ns))  # of a frame: (nz, ny, nx) down to (nx,)
        self.dtype = np.dtype(dtype)
        self.every = int(every)
        self._time = time
        self._sources = sources
        self._calls = 0
        self._nframes = 0
        self.frames = []
        self._files = FrameFiles(path, self.names, format, origin=[l + a * h for l, a, h in zip(mesh.lower, lo, mesh.h)],
                                 spacing=[h * s for h, s in zip(mesh.h, strides)], stride=strides, box=list(zip(lo, hi)))
        ctx = (sources[0][1] if sources[0][0] == "function" else sources[0][1].v_ode)._ctx
        self._ctx = ctx
        # one staging field of the grid per source of a multi-model solver
        self._sources = sources = [src + (ctx.field(mesh.num_nodes, mesh.plane),) if src[0] == "multi" else src for src in sources]
        self._outside = float(outside)
        self._mask = None
        if mesh.active is not None:  # a voxel mesh: uploaded once
            self._mask = ctx.from_numpy(mesh.node_active().astype(np.uint8))
        pad = lambda v, fill: (C.c_int64 * 3)(*(list(v) + [fill] * (3 - len(v))))  # noqa: E731
        self._n = mesh.num_nodes
        handle = C.c_void_p()
        flags = (_hip.SNAP_STATS if stats else 0) | (_hip.SNAP_NT_LOADS if nontemporal else 0)
        _hip.check(ctx.lib.beat_snap_create(ctx.handle, pad(mesh.shape_global[: mesh.dim], 1), pad(lo, 0), pad(hi, 1), pad(strides, 1),
                                            _DTYPES[dtype], len(sources), int(depth), None if self._mask is None else self._mask.data_ptr(),
                                            float(outside), flags, C.byref(handle)))
        self._snap = handle
        info = (C.c_int64 * 6)()
        _hip.check(ctx.lib.beat_snap_info(handle, info))
        assert [info[0], info[1], info[2]] == ns + [1] * (3 - len(ns)), (list(info), ns)
        self._field_bytes = int(info[3])
        self._free = threading.Semaphore(int(depth))
        self._queue = queue.Queue()
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._run, name="beat-field-writer", daemon=True)
        self._thread.start()

    # ---- the loop's side ---------------------------------------------------------------------------------------------------------
    def _pointers(self):
        ptrs = (C.c_void_p * len(self._sources))()
        # rows of multi-model solvers: every solver's are expanded into their staging fields in ONE launch, ahead of the pack launch
        # on the same stream -- so the staging fields are free again for the next frame at once
        multi = {}
        for src in self._sources:
            if src[0] == "multi":
                multi.setdefault(id(src[1]), (src[1], [], []))
                multi[id(src[1])][1].append(src[2])
                multi[id(src[1])][2].append(src[3])
        for ode, rows, staging in multi.values():
            ode._expand_rows(rows, staging, self._outside)
        for j, src in enumerate(self._sources):
            if src[0] == "function":
                fld = src[1].field  # (applies what is pending on the potential)
            elif src[0] == "multi":
                fld = src[3]
            else:
                _, ode, k, fld = src
                if k == ode.v_index:
                    ode._sync_v()
            if fld.n != self._n:
                raise ValueError(f"field {self.names[j]!r} has {fld.n} values, the mesh {self._n} nodes")
            ptrs[j] = fld.ptr.value
        return ptrs

    def write(self, t) -> None:
        """Enqueue a frame of the fields as they are now; see the class."""
        if self._closed:
            raise ValueError("this FieldWriter is closed")
        ptrs = self._pointers()
        self._free.acquire()  # all slots in flight: until the oldest frame is on disk
        if self._error is not None:  # (looked at behind the wait: what the oldest frame met is known by now)
            self._free.release()
            raise self._error
        slot = C.c_int(-1)
        rc = self._ctx.lib.beat_snap_enqueue(self._snap, ptrs, C.byref(slot))
        if rc != 0:
            self._free.release()
            _hip.check(rc)
        self._queue.put((slot.value, float(t)))
        self._nframes += 1

    def record(self) -> None:
        """A step has been made (``MonodomainSplittingSolver.solve(..., recorder=...)``): every ``every``-th call writes a frame."""
        self._calls += 1
        if self._calls % self.every == 0:
            time = self._time
            self.write(float(self._calls) if time is None else float(time()) if callable(time) else float(time))

    # ---- the thread's side ---------------------------------------------------------------------------------------------------------
    def _run(self) -> None:
        lib, nf = self._ctx.lib, len(self.names)
        while True:
            item = self._queue.get()
            if item is None:
                return
            slot, t = item
            try:
                host, stats = C.c_void_p(), (C.c_double * (3 * nf))()
                _hip.check(lib.beat_snap_wait(self._snap, slot, C.byref(host), stats))
                if self._error is None:  # (after a failure the frames are only taken out of their slots)
                    raw = np.ctypeslib.as_array((C.c_ubyte * (nf * self._field_bytes)).from_address(host.value))
                    frames = raw.view(self.dtype).reshape((nf,) + self.shape)
                    per_field = {n: (stats[3 * j], stats[3 * j + 1], int(stats[3 * j + 2])) for j, n in enumerate(self.names)}
                    self._files.add(t, {n: frames[j] for j, n in enumerate(self.names)}, per_field)
                    self.frames.append((t, per_field))
            except BaseException as exc:  # noqa: BLE001 -- handed to the thread that drives the loop
                if self._error is None:
                    self._error = exc
            finally:
                lib.beat_snap_release(self._snap, slot)
                self._free.release()

    def close(self) -> None:
        """Wait for the frames on their way, write the final index, free the device side.  Raises what the writer's thread met."""
        if self._closed:
            return
        self._closed = True
        self._queue.put(None)
        self._thread.join()
        try:
            if self._error is None:
                self._files.close()
        finally:
            snap, self._snap = self._snap, None
            _hip.check(self._ctx.lib.beat_snap_destroy(snap))
        if self._error is not None:
            raise self._error

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except BaseException:
            if exc_type is None:  # (an exception on its way out of the block is the one to see)
                raise
        return False

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except BaseException:
            pass
