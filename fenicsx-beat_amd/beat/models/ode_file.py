"""A device cell model from a user's gotran ``.ode`` file: ``beat.models.from_ode(path)``.

The reference takes ANY ``fun(states, t, parameters, dt)`` -- normally the function gotranx generates from an ``.ode`` file
(demos/niederer_benchmark.py:82-99: ``gotranx.load_ode`` + ``gotranx.cli.gotran2py.get_code(..., scheme=[generalized_rush_larsen])``)
-- and evaluates it with NumPy on the host (src/beat/odesolver.py:67-79).  The models this package ships (FHN, TP06, ToR-ORd) are
hand-written kernels; a model it does not ship used to run as a Python callable on host arrays, with the whole state array making
a round trip per step.  ``from_ode`` closes that: the file is parsed (``ast``: the format is Python syntax), every assignment is
turned into a SymPy expression, the right-hand sides f_i and the TOTAL self-derivatives J_ii = d f_i / d y_i (intermediates
resolved: the variant the reference's Niederer table pins) are put through common-subexpression elimination and printed
as one C++ ``Model`` struct for ``csrc/beat_ode_kernel.h``; the library compiles it at first use (``beat_ode_model_register``,
run-time ``hipcc --genco``, cached like the sparse-row instances) and every entry point that takes a model id takes this one:
the fused split step, the pending update, the library's step loop, per-node parameter rows, parameter classes and cell types in
one launch (``DolfinMultiODESolver``), the in-kernel time loop (``run`` / ``single_cell.get_steady_state``).  Schemes: ``generalized_rush_larsen`` (gotranx's GRL1:
y_i += f_i / J_ii (exp(J_ii dt) - 1) where |J_ii| > 1e-8, forward Euler elsewhere), ``forward_euler`` and
``generalized_rush_larsen_2`` (``grl2``: below).  ``exp`` in the
kernel is the library's table-driven evaluation (what the shipped models use: <= 1 ulp, 13 instead of ~50 VALU instructions; the
argument is kept inside double range); ``fast_exp=False`` prints libm's.

GRL2 is the second-order generalised Rush-Larsen step (Sundnes, Artebrant, Skavhaug, Tveito, IEEE Trans. Biomed. Eng. 2009): it
linearises about the midpoint and integrates from y_n.  With phi(a, h) = (exp(a h) - 1) / a where |a| > 1e-8 and h elsewhere
(GRL1's switch),

    stage 1   a_i = J_ii(y_n, t),          b_i = f_i(y_n, t),                               yh_i = y_n,i + phi(a_i, dt/2) b_i
    stage 2   A_i = J_ii(yh, t + dt/2),    B_i = f_i(yh, t + dt/2) + A_i (y_n,i - yh_i),    y_n+1,i = y_n,i + phi(A_i, dt) B_i

and a state whose self-derivative is identically zero takes the explicit midpoint rule (yh_i = y_i + dt/2 f_i(y_n, t),
y_n+1,i = y_i + dt f_i(yh, t + dt/2)).  ``time`` in the file's expressions is t in stage 1 and t + dt/2 in stage 2; a linear scalar
equation y' = a y + c is integrated exactly.  Both stages are printed into the one ``Model::step`` -- one launch, the states loaded
once, nothing stored in between -- so every route of a generated model takes it as it is.  It costs one more evaluation of (f, J)
per step; with ``MonodomainSplittingSolver(theta=0.5)`` and the PDE step's theta = 0.5 it makes the whole split step second order
in time, where GRL1 and forward Euler leave it first order whatever the PDE side does.  The models this package ships as
hand-written kernels (``tp06``, ``torord``, FHN) stay GRL1 / forward Euler.

The same expressions, lambdified for NumPy, are the handle's HOST evaluation (``numpy_step``): what the tests compare the kernel
with, and what runs where no GPU / compiler is to be had.  Parameters: a (P,) vector or per node (P, N); what a generated model
does not get is the instance compiled for a FEW varying rows (beat_ode_step_rows: a (P, N) array of a generated model is read
whole, or runs as classes when its columns are few).  SymPy is needed (it is what gotranx itself builds on).

Every assignment of the file -- currents, fluxes, rates, the ``d<state>_dt`` -- stays available by name, as in a gotranx module:
``monitor_names`` / ``monitor_index(name)`` / ``monitor_values(t, states, parameters, names)``.  For a selection of names a second
struct is printed (``_monitor_cxx``: same printer, common subexpressions over the selection alone) and evaluated by a read-only
kernel over the state array (``ode_monitor_kernel``, ``beat_ode_monitor``); ``numpy_monitor`` is its host twin.

Missing variables.  A cell model is routinely cut in two -- an electrophysiology half and a mechanics half -- and each half then
uses a few names the other half owns; the reference hands their values to ``fun`` as ``missing_variables`` on every step
(src/beat/odesolver.py:51-57).  ``from_ode(path, missing=("ca", "lmbda"))`` (or ``missing="auto"``) declares them: each is a real
symbol that is CONSTANT over a step -- the self-derivatives J_kk do not see it -- and may stand in any expression, the
monitored ones included.  For the kernel the model has NS = S + M rows: rows S .. S + M - 1 of the state array are INPUTS, loaded
where an expression uses them (8 B per used input row, node and step) and never stored, so every entry point of a generated
model serves it unchanged, and the in-kernel time loop holds them fixed over the run.  Under GRL2 both stages see the step-start
value of a missing variable: the step is then FIRST order in that variable, second order in the model's own states.
``missing_names`` / ``num_missing_variables`` / ``missing_index(name)`` / ``init_missing_values(**values)`` are the names a
gotranx-generated module of a split ODE is believed to offer; gotranx was not at hand when this was written, so that is a
recollection, not a checked parity.  ``num_states``, ``state_names``, ``state_index`` and ``init_state_values`` cover the file's
states alone.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from ._base import DeviceModel, host_and_device_parameters, parameter_args
from ._ode_parse import parse_ode

_SCHEMES = ("generalized_rush_larsen", "forward_euler", "generalized_rush_larsen_2")
# gotranx's own names for the first two schemes (gotranx.schemes: what its code generator is asked for), and GRL2's short one
_SCHEME_ALIASES = {"forward_generalized_rush_larsen": "generalized_rush_larsen", "forward_explicit_euler": "forward_euler",
                   "explicit_euler": "forward_euler", "grl2": "generalized_rush_larsen_2"}


def _on_gpu() -> bool:
    """Is there a GPU to run a kernel on?  (Without one -- or without torch -- the handle evaluates with NumPy.)"""
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


class OdeFileModel(DeviceModel):
    """A :class:`DeviceModel` generated from an ``.ode`` file (see the module docstring)."""

    def __init__(self, path, scheme="generalized_rush_larsen", v_name=None, name=None, fast_exp=True, missing=None, missing_ranges=None):
        from . import _ode_cxx  # (SymPy is needed from here on, not by `import beat`)
        from ._ode_numpy import NumpyTwin
        from ._ode_symbolic import OdeSystem

        scheme = _SCHEME_ALIASES.get(scheme, scheme)
        if scheme not in _SCHEMES:
            raise ValueError(f"scheme must be one of {_SCHEMES}, got {scheme!r}")
        self.path, self.scheme, self.fast_exp = Path(path), scheme, bool(fast_exp)
        source = parse_ode(self.path, missing)
        self.missing_names = source.missing_names
        self.missing_ranges = {nm: (0.0, 1.0) for nm in self.missing_names}
        for nm, (lo, hi) in (missing_ranges or {}).items():
            if nm not in self.missing_ranges:
                raise ValueError(f"{self.path}: missing_ranges names {nm!r}, which is not a missing variable of this model")
            self.missing_ranges[nm] = (float(lo), float(hi))
        if v_name is None:
            v_name = next((s for s in source.states if s.lower() in ("v", "vm", "v_m")), None)
        if v_name is not None and v_name not in source.states:
            raise KeyError(f"{v_name!r} is not a state of {self.path.name}")
        self._stem = "".join(c if c.isalnum() else "_" for c in (name or self.path.stem))
        super().__init__(f"{self._stem}_{scheme}", -1, source.states, source.parameters, v_name)
        self._system = OdeSystem.from_source(source, scheme)
        self._grl = self._system.grl  # which J_kk are not identically zero: the states that take the exponential update
        self._twin = NumpyTwin(self._system, scheme)
        # every assignment of the file, in dependency order: what monitor_values / numpy_monitor can be asked for
        self.monitor_names = tuple(self._system.assigned)
        self._monitors = {}       # names of one launch -> the library's monitor id (beat_ode_monitor_register), once self-checked
        self._registered = None   # the library's id, once the compiled kernel has passed _self_check
        self._library_id = None   # the id beat_ode_model_register gave (the source is handed over once per process)
        self.cxx_name, self.source = _ode_cxx.step_struct(self._system, scheme, self._stem, self.state_index(v_name) if v_name else None,
                                                          _ode_cxx.CxxOptions.from_environment(self.fast_exp))
        self.key = f"{self.cxx_name}"

    @property
    def num_missing_variables(self) -> int:
        return len(self.missing_names)

    @property
    def num_rows(self) -> int:
        """Rows of the state array the kernel works on: the states, then one input row per missing variable."""
        return self.num_states + self.num_missing_variables

    def missing_index(self, name: str) -> int:
        if name not in self.missing_names:
            raise KeyError(f"Unknown missing variable {name}")
        return self.missing_names.index(name)

    def init_missing_values(self, **values) -> np.ndarray:
        """An (M,) vector of the missing variables in the order of ``missing_names``: 0.0 but for the ones given by name."""
        for k in values:
            if k not in self.missing_names:
                raise KeyError(f"Unknown missing variable {k}")
        return np.array([values.get(k, 0.0) for k in self.missing_names], dtype=np.float64)

    def _rows(self, states, missing_variables):
        """(S + M, N) rows for the kernel -- ``states`` (S,) or (S, N) above ``missing_variables`` (M,) or (M, N) -- and whether
        ``states`` was (S,).  TypeError where the model has missing variables and gets none, or has none and gets some."""
        m = self.num_missing_variables
        if m == 0 and missing_variables is not None:
            raise TypeError(f"{self.name} has no missing variables: missing_variables must not be given")
        if m and missing_variables is None:
            raise TypeError(f"{self.name} has the missing variables {self.missing_names}: missing_variables=... is required")
        y = np.asarray(states, dtype=np.float64)
        y2 = y.reshape(y.shape[0], -1)
        if m == 0:
            return y2, y.ndim == 1
        if y2.shape[0] != self.num_states:
            raise ValueError(f"{self.name} has {self.num_states} states, got {y2.shape[0]}")
        c = np.asarray(missing_variables, dtype=np.float64)
        if c.shape not in ((m,), (m, y2.shape[1])):
            raise ValueError(f"missing_variables must have shape ({m},) or ({m}, {y2.shape[1]}), got {c.shape}")
        return np.concatenate([y2, np.broadcast_to(c.reshape(m, -1), (m, y2.shape[1]))], axis=0), y.ndim == 1

    def _monitor_cxx(self, names):
        """``_ode_cxx.monitor_struct`` for ``names`` (at most _hip.MAX_MONITORS), with the BEAT_ODE_* switches as they are now."""
        from . import _ode_cxx

        return _ode_cxx.monitor_struct(self._system, names, self._stem, _ode_cxx.CxxOptions.from_environment(self.fast_exp))

    def monitor_sources(self, names=None):
        """[(struct name, source, names)] -- one per launch: ``names`` (None: all) in runs of at most _hip.MAX_MONITORS."""
        from .. import _hip

        names = self._monitor_selection(names)
        return [self._monitor_cxx(names[k:k + _hip.MAX_MONITORS]) + (tuple(names[k:k + _hip.MAX_MONITORS]),)
                for k in range(0, len(names), _hip.MAX_MONITORS)]

    def numpy_step(self, states, t, parameters, dt, missing_variables=None):
        """One step on the HOST with NumPy: the same expressions as the kernel's (the reference's way of evaluating ``fun``).
        ``missing_variables``: (M,) or (M, N), for a model made with ``missing=`` (TypeError where such a model gets none, or
        another model gets some); held at these values through both stages of GRL2.  Returns the S states."""
        return self._twin.step(*self._rows(states, missing_variables), t, parameters, dt)

    def monitor_index(self, name: str) -> int:
        if name not in self.monitor_names:
            raise KeyError(f"Unknown monitor {name}")
        return self.monitor_names.index(name)

    def _monitor_selection(self, names):
        """``names`` (None: all) as a list, each one checked."""
        if names is None:
            return list(self.monitor_names)
        if isinstance(names, str):
            names = [names]
        names = list(names)
        for nm in names:
            self.monitor_index(nm)
        return names

    def numpy_monitor(self, states, t, parameters, names=None, missing_variables=None):
        """The values of the file's assignments ``names`` (None: all of ``monitor_names``) on the HOST with NumPy: (M,) for (S,)
        states, (M, N) for (S, N); parameters (P,) or (P, N); ``missing_variables`` as for ``numpy_step``.  What the monitor kernel is held to."""
        return self._twin.monitor(self._monitor_selection(names), *self._rows(states, missing_variables), t, parameters)

    # ------------------------------------------------------------------------------------------------ device
    def register(self) -> int:
        """The library's id for this model (beat_ode_model_register: the source is handed over once per process; the kernel is
        compiled when a step first needs it).  Raises BeatHipError where the library cannot compile at run time."""
        from .. import _hip

        if self._registered is None:
            if self._library_id is None:
                mid = C.c_int(-1)
                _hip.check(_hip.load().beat_ode_model_register(self.cxx_name.encode(), self.source.encode(), self.num_rows,
                                                       max(self.num_parameters, 1), self.state_index(self.v_name) if self.v_name else 0,
                                                       C.byref(mid)))
                self._library_id = int(mid.value)
            # the id is handed out only once the compiled kernel has passed its check: a caller that catches the check's error and
            # asks again gets the check again, not the id of a kernel known to be wrong
            self.model_id = self._library_id  # (the check itself steps the model through DeviceModel.__call__)
            try:
                self._self_check()
            except BaseException:
                self.model_id = -1
                raise
            self._registered = self._library_id
        return self._registered

    def _sample_states(self, n: int, seed: int = 0) -> np.ndarray:
        """States to try a kernel on: the initial values, the potential spread over [-100, 60] mV, values in [0, 1] (gates) spread
        over [0, 1], everything else within +-30 % of its initial value.  A model with missing variables gets (S + M, n): each
        input row spread over its ``missing_ranges`` entry ((0, 1) unless ``from_ode`` was told otherwise)."""
        rng = np.random.default_rng(seed)
        y = np.repeat(self.init_state_values()[:, None], n, axis=1)
        for k, name in enumerate(self.state_names):
            y0 = y[k, 0]
            if name == self.v_name:
                y[k] = rng.uniform(-100.0, 60.0, n)
            elif 0.0 <= y0 <= 1.0:
                y[k] = rng.uniform(0.0, 1.0, n)
            else:
                y[k] = y0 * rng.uniform(0.7, 1.3, n)
        y[:, 0] = self.init_state_values()
        if self.missing_names:
            y = np.concatenate([y, np.stack([rng.uniform(*self.missing_ranges[nm], n) for nm in self.missing_names])], axis=0)
        return y

    def _split_rows(self, rows):
        """(the S state rows, the M input rows or None) of an (S + M, N) array."""
        return rows[: self.num_states], (rows[self.num_states:] if self.missing_names else None)

    def _numpy_step_rows(self, rows, t, parameters, dt):
        """``numpy_step`` on the kernel's (S + M, N) rows: the states advanced, the input rows as they were."""
        y, c = self._split_rows(rows)
        out = self.numpy_step(y, t, parameters, dt, missing_variables=c)
        return out if c is None else np.concatenate([out, c], axis=0)

    def step_rows(self, rows, t, parameters, dt):
        """One kernel step of the (S + M, N) rows as the state array holds them -- the states above the input rows -- staged
        through the device: all rows back, the input rows untouched.  (``__call__`` takes and returns the S states.)"""
        self.register()
        return DeviceModel.__call__(self, states=rows, t=t, parameters=parameters, dt=dt)

    @staticmethod
    def step_error(dev, ref, y):
        """|dev - ref| / max(|ref|, |y|) (relative to the state before or after the step, whichever is larger: y + dt f may
        cancel) over the finite reference values; inf where ``dev`` is not finite there."""
        ok = np.isfinite(ref)
        with np.errstate(all="ignore"):  # (inf - inf where both sides overflow: masked by `ok`)
            err = np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(y)), 1e-12)
        return np.where(ok, np.where(np.isfinite(dev), err, np.inf), 0.0)

    def _check_against_numpy(self, what, rows, device, host, error):
        """The frame of the two self checks: ``device(y, t, p, dt)`` against ``host(y, t, p, dt)`` on the 2048 states of
        ``_sample_states`` at two times, the instance refused (RuntimeError) where ``error(dev, ref, y)`` exceeds 1e-6 -- a sample
        far from the model's physiological range may sit where exp(J dt) - 1 cancels, and the two exp()s differ in the last bit
        (3e-8 seen); a miscompiled kernel is wrong by O(1) on thousands of values.  Returns the largest error seen, or None
        where BEAT_JIT_SELF_CHECK=0 skips the check."""
        import os

        if os.environ.get("BEAT_JIT_SELF_CHECK", "1") == "0":
            return None
        y = self._sample_states(2048)
        p = self.init_parameter_values()
        worst = 0.0
        for t, dt in ((0.0, 0.01), (0.37, 0.05)):
            dev = device(y, t, p, dt)
            with np.errstate(all="ignore"):
                ref = host(y, t, p, dt)
            err = error(dev, ref, y)
            if err.max() > 1e-6:
                k, i = np.unravel_index(int(np.argmax(err)), err.shape)
                raise RuntimeError(
                    f"{self.name}: the compiled {what} differs from the NumPy evaluation of the same expressions ({rows[k]}, sample {i}: "
                    f"{dev[k, i]!r} against {ref[k, i]!r}; {int((err > 1e-6).sum())} of {err.size} values) -- a miscompiled (heavily spilled) "
                    "kernel; other compiler flags (BEAT_JIT_EXTRA_FLAGS) may help, BEAT_JIT_SELF_CHECK=0 skips this check")
            worst = max(worst, float(err.max()))
        return worst

    def _self_check(self) -> None:
        """The model's PLAIN kernel instance (uniform parameters, no pending update) against the NumPy evaluation of the same
        expressions (``_check_against_numpy``, to 1e-6 of each value), once per process: a big generated kernel is heavily spilled,
        and such a kernel has been seen miscompiled (round 1; reproduced in round 5, tools/diag_spill.py) -- wrong values on part of
        the nodes, silently.  The other instances (per-node rows, pending update, classes) are held against this one by the library
        at their first launch (csrc/beat_ode_jit.hip: custom_cross_check).  BEAT_JIT_SELF_CHECK=0 skips both.  A GRL2 model is held
        to the same 1e-6 through both of its stages (``numpy_step`` is the two-stage twin): a last-bit difference of the two
        exp()s in stage 1 reaches the result only through stage 2's derivative with respect to the midpoint values, and the
        bound needs no widening for it (tests/data/small_cell.ode on an MI355X: 2.3e-8 under GRL2, 3.3e-8 under GRL1).  The input
        rows of a model with missing variables are part of both sides: the kernel must hand them back as they went in."""
        if getattr(self, "_verified", False):
            return
        worst = self._check_against_numpy(
            "kernel", [f"state {s}" for s in self.state_names] + [f"input row {m}" for m in self.missing_names],
            lambda y, t, p, dt: DeviceModel.__call__(self, states=y, t=t, parameters=p, dt=dt), self._numpy_step_rows, self.step_error)
        if worst is not None:
            self.self_check_error = worst
            self._verified = True

    # ---- monitored values --------------------------------------------------------------------------------
    def _monitor_launches(self, names):
        """[(the library's monitor id, number of rows)] for ``names``, one per launch of at most _hip.MAX_MONITORS rows
        (beat_ode_monitor_register: a selection's source is handed over once per process; its kernel is compiled when a launch
        first needs it).  The id is handed out once the selection's plain instance has passed ``_monitor_self_check``."""
        from .. import _hip

        self.register()
        out = []
        for k in range(0, len(names), _hip.MAX_MONITORS):
            run = tuple(names[k:k + _hip.MAX_MONITORS])
            if run not in self._monitors:
                name, source = self._monitor_cxx(list(run))
                mid = C.c_int(-1)
                _hip.check(_hip.load().beat_ode_monitor_register(self._registered, name.encode(), source.encode(), len(run), C.byref(mid)))
                self._monitor_self_check(int(mid.value), run)
                self._monitors[run] = int(mid.value)
            out.append((self._monitors[run], len(run)))
        return out

    def monitor_on_device(self, ctx, names, states_ptr, n, ld, t, out_ptr, out_ld, host_params=None, per_node=None, classes=None):
        """Enqueue the monitor kernel(s) for ``names`` on a RESIDENT state array (``states_ptr``: its row 0, rows ``ld`` apart):
        row j of the selection goes to ``out_ptr`` + 8 j ``out_ld`` bytes.  Parameters: ``host_params`` (a (P,) NumPy vector), or
        ``per_node`` = (the (P, n) device rows, tensor or pointer, their stride), or ``classes`` = (marker bytes, table, number of classes)
        as ``_DeviceODE.set_classes`` keeps them.  Does not wait."""
        row = 0
        for mid, m in self._monitor_launches(self._monitor_selection(names)):
            self._monitor_call(ctx, mid, states_ptr, n, ld, t, out_ptr.value + 8 * row * int(out_ld), out_ld, host_params, per_node, classes)
            row += m

    def _monitor_call(self, ctx, mid, states_ptr, n, ld, t, out_addr, out_ld, host_params, per_node, classes):
        """beat_ode_monitor for one registered selection (see monitor_on_device for the arguments)."""
        from .. import _hip

        hp = None if host_params is None else np.ascontiguousarray(host_params, dtype=np.float64)
        mk, table, ncls = (None, None, 0) if classes is None else (C.c_void_p(classes[0].data_ptr()), C.c_void_p(classes[1].data_ptr()), int(classes[2]))
        _hip.check(ctx.lib.beat_ode_monitor(ctx.handle, mid, states_ptr, int(n), int(ld), *parameter_args(hp, *(per_node or (None, 0)), max(self.num_parameters, 1)),
                                            table, ncls, mk, float(t), C.c_void_p(out_addr), int(out_ld)))

    def _monitor_staged(self, mid, m, y2, t, parameters):
        """One launch on host arrays staged through the device: (m, N)."""
        from .._device import Context, StateArray

        ctx = Context.default()
        S, n = y2.shape
        sa = StateArray(ctx, S, n)
        sa.set(y2)
        hp, ppn, pld = host_and_device_parameters(ctx, parameters, self.num_parameters, n)
        out = ctx.zeros(m * n)
        self._monitor_call(ctx, mid, sa.ptr, n, sa.ld, t, out.data_ptr(), n, hp, None if ppn is None else (ppn, pld), None)
        return out.cpu().numpy().reshape(m, n)

    @staticmethod
    def monitor_error(dev, ref):
        """|dev - ref| / max(|ref|, S_k), S_k the largest finite |ref| of row k (a sum of currents that cancel is measured against
        the row's scale), over the finite reference values; inf where ``dev`` is not finite there."""
        dev, ref = np.atleast_2d(dev), np.atleast_2d(ref)
        ok = np.isfinite(ref)
        with np.errstate(all="ignore"):
            scale = np.where(ok, np.abs(ref), 0.0).max(axis=1, keepdims=True)
            err = np.abs(dev - ref) / np.maximum(np.maximum(np.abs(ref), scale), 1e-300)
        return np.where(ok, np.where(np.isfinite(dev), err, np.inf), 0.0)

    def _monitor_self_check(self, mid: int, names) -> None:
        """A selection's PLAIN kernel instance (uniform parameters) against ``numpy_monitor`` (``_check_against_numpy``), to 1e-6 of
        each value (of its row's scale where the value is smaller), at its first use in a process: the reason is ``_self_check``'s.
        The per-node and class instances are held against this one by the library at their first launch (csrc/beat_ode_jit.hip:
        monitor_cross_check).  BEAT_JIT_SELF_CHECK=0 skips both; a failing instance raises."""
        self._check_against_numpy("monitor kernel", names, lambda y, t, p, dt: self._monitor_staged(mid, len(names), y, t, p),
                                  lambda y, t, p, dt: self.numpy_monitor(self._split_rows(y)[0], t, p, list(names), missing_variables=self._split_rows(y)[1]),
                                  lambda dev, ref, y: self.monitor_error(dev, ref))

    def monitor_values(self, t, states, parameters, names=None, missing_variables=None):
        """gotranx's ``monitor_values(t, states, parameters)``: the values of the file's assignments ``names`` (None: all, in the
        order of ``monitor_names``; ``monitor_index(name)`` gives a row) for (S,) or (S, N) states and (P,) or (P, N) parameters,
        as (M,) or (M, N).  With a GPU the arrays are staged through the device and the monitor kernel runs; without one this is
        ``numpy_monitor``, as ``__call__`` is ``numpy_step``.  ``missing_variables``: (M,) or (M, N) for a model made with
        ``missing=`` (the kernel reads them as rows behind the states)."""
        if not _on_gpu():
            return self.numpy_monitor(states, t, parameters, names, missing_variables=missing_variables)
        names = self._monitor_selection(names)
        y2, one_d = self._rows(states, missing_variables)
        y2 = np.ascontiguousarray(y2)
        if y2.shape[0] != self.num_rows:
            raise ValueError(f"{self.name} has {self.num_states} states, got {y2.shape[0] - self.num_missing_variables}")
        out = np.concatenate([self._monitor_staged(mid, m, y2, t, parameters) for mid, m in self._monitor_launches(names)], axis=0)
        return out[:, 0].copy() if one_d else out

    def __call__(self, states=None, t=0.0, parameters=None, dt=None, missing_variables=None, **kwargs):
        """The reference's ``fun(states=, t=, parameters=, dt=[, missing_variables=])``: the S states advanced by one step.  A model
        made with ``missing=`` needs ``missing_variables`` ((M,) or (M, N)); any other refuses them (TypeError either way)."""
        if dt is None:
            raise TypeError("dt is required")
        if not _on_gpu():
            return self.numpy_step(states, t, parameters, dt, missing_variables=missing_variables)
        rows, one_d = self._rows(states, missing_variables)
        if not self.missing_names:
            self.register()
            return super().__call__(states=states, t=t, parameters=parameters, dt=dt, **kwargs)
        out = self.step_rows(rows, t, parameters, dt)[: self.num_states]
        return out[:, 0].copy() if one_d else out

    def run(self, states, parameters, dt, nsteps, nbeats=1, t0=0.0, track_indices=None, save_freq=1, missing_variables=None):
        """nbeats x nsteps steps inside ONE launch (beat_ode_run: ``ode_run_kernel`` instantiated for this model at first use), as
        for the shipped models -- ``single_cell.get_steady_state`` with a generated model paces on the device.
        ``missing_variables``: (M,) or (M, N), held constant over the whole run (the kernel keeps the input rows in registers
        next to the states and never advances them)."""
        self.register()
        rows, one_d = self._rows(states, missing_variables)
        if not self.missing_names:
            return super().run(states, parameters, dt, nsteps, nbeats=nbeats, t0=t0, track_indices=track_indices, save_freq=save_freq)
        if track_indices is not None and any(not 0 <= int(i) < self.num_states for i in track_indices):
            raise ValueError(f"track_indices must name states of {self.name} (0 .. {self.num_states - 1})")
        out, track = super().run(rows, parameters, dt, nsteps, nbeats=nbeats, t0=t0, track_indices=track_indices, save_freq=save_freq)
        out = out[: self.num_states]
        if one_d:
            out, track = out[:, 0].copy(), (None if track is None else track[:, :, 0])
        return out, track


def from_ode(path, scheme: str = "generalized_rush_larsen", v_name: str | None = None, name: str | None = None,
             fast_exp: bool = True, missing=None, missing_ranges: dict | None = None) -> OdeFileModel:
    """A device cell model from a gotran ``.ode`` file: pass the result as ``fun`` to ``DolfinODESolver`` (and use its
    ``init_state_values`` / ``init_parameter_values`` / ``state_index`` / ``parameter_index`` as those of a gotranx module).
    ``scheme``: ``"generalized_rush_larsen"`` (GRL1), ``"forward_euler"``, or the second-order ``"generalized_rush_larsen_2"``
    (``"grl2"``; see the module docstring).

    ``missing``: the missing variables of a SPLIT cell model -- names the file uses and neither declares nor assigns, because the
    other half of the model owns them (see the module docstring).  ``None``: there are none, and an undefined name is an error;
    a sequence of names: these, in this order; ``"auto"``: every free name of the file, sorted.  ``missing_ranges``:
    ``{name: (lo, hi)}``, the range the kernel's self check draws a missing variable from, (0, 1) where not given."""
    return OdeFileModel(path, scheme=scheme, v_name=v_name, name=name, fast_exp=fast_exp, missing=missing, missing_ranges=missing_ranges)
