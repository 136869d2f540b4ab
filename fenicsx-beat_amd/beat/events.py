"""Per-node event maps recorded ON THE DEVICE: activation time, last activation, repolarisation time, APD, maximal upstroke
velocity and maximal potential of a function that a time loop advances.

Every tissue demo of the reference builds its activation map on the host, from the whole potential after each step
(demos/irksome_model_gotranx.py:251-254: ``crossed = (v_arr >= activation_threshold) & (tact_arr < 0.0); tact_arr[crossed] = t``;
demos/niederer_benchmark.py:285-287: the same rule with ``> 0.0`` at probe points).  Here that would be a flush of the deferred
update, a device-to-host copy of the field and a synchronisation per step; ``EventRecorder.observe`` is one launch
(beat_field_events), and where the potential's last update is still pending on the diffusion operator it IS that update
(beat_pde_x_flush_events: one pass over the potential instead of two).  That second route is not free of the host: the solve
that ``step()`` leaves open has to be finished first, which waits for it and reads its KSP record, once per step, and the next
ionic launch is no longer queued behind the open solve."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _hip
from ._deferred import DeferredUpdate
from .grid import Function

# public name -> field of beat_event_maps
MAPS = {"activation": "act_first", "last_activation": "act_last", "repolarisation": "repol", "apd": "apd",
        "dvdt_max": "dvdt_max", "v_max": "v_max"}
_TIME_MAPS = ("act_first", "act_last", "repol", "apd")
_COMPARE = {">=": 0, ">": 1}
_MODES = {"step": 0, "linear": 1}


class EventRecorder:
    """``EventRecorder(f, threshold, repolarisation_threshold=None, maps=("activation",), mode="step", compare=">=")``

    ``maps``: any of ``activation`` (time of the first upstroke through ``threshold``; a node found above it when first observed
    is activated at that step, the reference's rule), ``last_activation`` (of the latest one), ``repolarisation`` (time of the
    latest fall below ``repolarisation_threshold`` of an activated node), ``apd`` (that time minus the activation it belongs to),
    ``dvdt_max`` (largest (v_new - v_old) / dt seen) and ``v_max``.  Each is a ``grid.Function`` on ``f``'s space
    (``rec.activation.x.array``).  Times are NaN where nothing has happened -- the nodes outside the tissue of a voxel mesh among
    them; the two maxima are -inf until the first observation, which gives every node a value (0 for both outside the tissue,
    where the potential stays 0).  ``mode``: ``"step"`` gives an event the end of its step (the reference), ``"linear"`` the time at
    which the line through the two values crosses the threshold.  ``compare``: ``">="`` or ``">"``, the reference's two spellings
    of "above".

    ``observe(t0, t1)`` after each step enqueues the pass (``MonodomainSplittingSolver.solve(..., recorder=rec)`` calls it).  On a
    function of its own it does not wait; on the potential of a split step it first finishes the solve that ``step()`` left open
    (one host wait per step).  The potential a step ago is kept only when a map or the mode needs it (all but ``activation`` in step mode and
    ``v_max``), and is taken from ``f`` when the recorder is made or ``reset()``."""

    def __init__(self, f: Function, threshold, repolarisation_threshold=None, maps=("activation",), mode="step", compare=">="):
        if isinstance(maps, str):
            maps = (maps,)
        maps = tuple(maps)
        unknown = [m for m in maps if m not in MAPS]
        if unknown or len(set(maps)) != len(maps):
            raise ValueError(f"maps must be distinct names out of {sorted(MAPS)}, got {maps!r}")
        if mode not in _MODES:
            raise ValueError(f"mode must be 'step' or 'linear', got {mode!r}")
        if compare not in _COMPARE:
            raise ValueError(f"compare must be '>=' or '>', got {compare!r}")
        down = "repolarisation" in maps or "apd" in maps
        if down and repolarisation_threshold is None:
            raise ValueError("the maps 'repolarisation' and 'apd' need repolarisation_threshold")
        if f.function_space.mesh.comm.size > 1:
            raise NotImplementedError("EventRecorder on a decomposed mesh: the maps would need no communication, but nothing tests them yet")
        self._f = f
        self._ctx = f._ctx
        self.maps = maps
        self.threshold = float(threshold)
        self.repolarisation_threshold = None if repolarisation_threshold is None else float(repolarisation_threshold)
        self.mode, self.compare = mode, compare
        self._n = f.num_values
        self._functions = {name: Function(f.function_space, name) for name in maps}
        fields = {MAPS[name]: fn._own for name, fn in self._functions.items()}
        if down and "act_last" not in fields:  # a repolarisation belongs to an activation: kept though not asked for
            fields["act_last"] = self._new_field()
        needs_prev = (mode == "linear" and any(k in fields for k in _TIME_MAPS)) or any(k in fields for k in ("act_last", "dvdt_max"))
        if needs_prev:
            fields["v_prev"] = self._new_field()
        self._fields = fields
        self._args = _hip.EventMaps(
            thr_up=self.threshold, thr_down=0.0 if self.repolarisation_threshold is None else self.repolarisation_threshold,
            mode=_MODES[mode], strict=_COMPARE[compare], **{k: fld.ptr.value for k, fld in fields.items()})
        self.fused_passes = 0  # observations that were the deferred update of the potential as well
        self.reset()

    def _new_field(self):
        like = self._f._own
        return self._ctx.field(like.n, like.plane)

    def __getattr__(self, name):
        fns = self.__dict__.get("_functions", {})
        if name in fns:
            return fns[name]
        if name in MAPS:
            raise AttributeError(f"the map {name!r} was not selected (maps={self.__dict__.get('maps')!r})")
        raise AttributeError(name)

    def reset(self) -> None:
        """Forget everything: times NaN, maxima -inf, the potential a step ago = ``f`` as it is now."""
        for key, fld in self._fields.items():
            if key == "v_prev":
                fld.copy_from(self._f.field)
            else:
                fld.fill(float("nan") if key in _TIME_MAPS else -np.inf)
        for fn in self._functions.values():
            fn._touch()

    def observe(self, t0, t1) -> None:
        """The step (t0, t1) has just been made: update the maps from ``f``.  One launch.  Where ``f`` is the potential whose solve is still
        open, that solve is finished first: the host waits for it and reads its record (``DeferredUpdate.flush_events``)."""
        f = self._f
        args = C.byref(self._args)
        # f aliases the potential row whose update the diffusion operator still owes (the fused split step): this pass applies it
        owner = f._alias_sync if f._alias is not None else None
        if isinstance(owner, DeferredUpdate) and owner.flush_events(f._alias, args, float(t0), float(t1)):
            self.fused_passes += 1
        else:
            _hip.check(self._ctx.lib.beat_field_events(self._ctx.handle, f.field.ptr, self._n, args, float(t0), float(t1)))
        for fn in self._functions.values():
            fn._touch()
