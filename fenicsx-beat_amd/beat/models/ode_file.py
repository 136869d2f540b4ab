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

import ast
import copy
import ctypes as C
import hashlib
from pathlib import Path

import numpy as np

from ._base import DeviceModel, host_and_device_parameters, parameter_args

_SCHEMES = ("generalized_rush_larsen", "forward_euler", "generalized_rush_larsen_2")
# gotranx's own names for the first two schemes (gotranx.schemes: what its code generator is asked for), and GRL2's short one
_SCHEME_ALIASES = {"forward_generalized_rush_larsen": "generalized_rush_larsen", "forward_explicit_euler": "forward_euler",
                   "explicit_euler": "forward_euler", "grl2": "generalized_rush_larsen_2"}
_RUSH_LARSEN = ("generalized_rush_larsen", "generalized_rush_larsen_2")  # the schemes that need the self-derivatives J_ii


def _walk(text: str, where: str):
    tree = ast.parse(text, filename=where)
    for node in tree.body:
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Name):
            yield "call", node.value.func.id, node.value
        elif isinstance(node, ast.Assign):
            if len(node.targets) != 1 or not isinstance(node.targets[0], ast.Name):
                raise ValueError(f"{where}:{node.lineno}: only plain assignments `name = expression` are understood")
            yield "assign", node.targets[0].id, node.value
        elif isinstance(node, ast.Expr):  # a docstring / bare constant
            continue
        else:
            raise ValueError(f"{where}:{node.lineno}: statement not understood in an .ode file")


_EXPR_NODES = (ast.BinOp, ast.UnaryOp, ast.Call, ast.Name, ast.Constant, ast.Load, ast.Add, ast.Sub, ast.Mult, ast.Div, ast.Pow,
               ast.USub, ast.UAdd, ast.Compare, ast.Lt, ast.LtE, ast.Gt, ast.GtE, ast.Eq, ast.NotEq, ast.BoolOp, ast.And, ast.Or, ast.Not,
               ast.Mod)
# What an expression of an .ode file may call (SymPy's function of the same name, but for the two renamed below and Conditional),
# and the constants it may name besides its states, parameters and intermediates (tests/data/language_cell.ode uses each of them)
_FUNCTIONS = ("exp", "log", "sqrt", "floor", "abs", "Abs", "pow", "sin", "cos", "tan", "tanh", "sinh", "cosh", "atan", "asin", "acos",
              "Conditional", "Lt", "Le", "Gt", "Ge", "Eq", "And", "Or", "Not")
_SYMPY_NAMES = {"abs": "Abs", "pow": "Pow"}
_CONSTANTS = ("time", "t", "pi")
_RELATIONS = ("Lt", "Le", "Gt", "Ge", "Eq", "And", "Or", "Not")


def _check_expression(node, where: str, known) -> None:
    """The right-hand side of an assignment is evaluated (with SymPy objects for the names) to build the expression tree: only
    arithmetic, comparisons and calls of the functions an .ode file may use pass -- no attribute access, subscripts, lambdas,
    comprehensions or keyword tricks: an .ode file is data, and this is not the place where it gets to run code."""
    for n in ast.walk(node):
        if not isinstance(n, _EXPR_NODES):
            raise ValueError(f"{where}:{getattr(n, 'lineno', '?')}: `{type(n).__name__}` is not understood in an expression of an .ode file")
        if isinstance(n, ast.Call):
            if not isinstance(n.func, ast.Name) or n.func.id not in known or n.keywords:
                raise ValueError(f"{where}:{n.lineno}: call of an unknown function in an .ode file"
                                 + (f": {n.func.id}" if isinstance(n.func, ast.Name) else ""))
        if isinstance(n, ast.Constant) and not isinstance(n.value, (int, float)):
            raise ValueError(f"{where}:{n.lineno}: only numbers are understood in an expression of an .ode file")


class _ComparisonsAsNumbers(ast.NodeTransformer):
    """gotran lets a comparison stand in arithmetic as 0 or 1 -- ``gammas*((zetas > 0)*zetas + (zetas < -1)*(-zetas - 1))`` in the
    Land model, ``Gt(Zetas, 0)*Zetas`` in the reference's own file: a comparison (infix or Lt / Le / Gt / Ge / Eq / And / Or / Not)
    that is an operand of an arithmetic operator becomes ``_indicator(comparison)``
    (Piecewise((1, c), (0, True))); as an argument of Conditional / And / Or / Not it stays a condition.

    Infix forms become the calls first, since Python's own meaning of them on SymPy objects is not gotran's: ``a == b`` and
    ``a != b`` on a Symbol are a structural test that gives a bool (``Eq`` / ``Not(Eq)`` here), a chained ``a < b <= c`` and
    ``and`` / ``or`` / ``not`` ask a relation for its truth value (``And`` of the pairs, ``And`` / ``Or`` / ``Not`` here).  The
    operands of ``and`` / ``or`` / ``not`` must be comparisons: anything else is refused with its line."""

    _OPS = {ast.Lt: "Lt", ast.LtE: "Le", ast.Gt: "Gt", ast.GtE: "Ge", ast.Eq: "Eq", ast.NotEq: "Eq"}

    def __init__(self, where: str):
        self.where = where

    @staticmethod
    def _call(name, args, like):
        return ast.copy_location(ast.Call(func=ast.Name(id=name, ctx=ast.Load()), args=args, keywords=[]), like)

    @staticmethod
    def _is_relation(node):
        return isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in _RELATIONS

    def _wrap(self, node):
        return self._call("_indicator", [node], node) if self._is_relation(node) else node

    def _relations(self, nodes, what, like):
        for n in nodes:
            if not self._is_relation(n):
                raise ValueError(f"{self.where}:{like.lineno}: the operands of `{what}` in an .ode file must be comparisons")
        return nodes

    def visit_Compare(self, node):
        self.generic_visit(node)
        pairs, left = [], node.left
        for op, right in zip(node.ops, node.comparators):
            rel = self._call(self._OPS[type(op)], [copy.deepcopy(left), copy.deepcopy(right)], node)
            pairs.append(self._call("Not", [rel], node) if isinstance(op, ast.NotEq) else rel)
            left = right
        return pairs[0] if len(pairs) == 1 else self._call("And", pairs, node)

    def visit_BoolOp(self, node):
        self.generic_visit(node)
        what = "and" if isinstance(node.op, ast.And) else "or"
        return self._call("And" if what == "and" else "Or", self._relations(node.values, what, node), node)

    def visit_BinOp(self, node):
        self.generic_visit(node)
        node.left, node.right = self._wrap(node.left), self._wrap(node.right)
        return node

    def visit_UnaryOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Not):
            return self._call("Not", self._relations([node.operand], "not", node), node)
        node.operand = self._wrap(node.operand)
        return node


def _number(node) -> float:
    if isinstance(node, ast.Call):  # ScalarParam(value, unit=..., ...)
        return float(ast.literal_eval(node.args[0]))
    return float(ast.literal_eval(node))


def _dependency_order(assignments):
    """gotran files may use an intermediate before the line that defines it: order by dependencies (stable)."""
    defined = {name for name, _ in assignments}
    deps = {name: ({n.id for n in ast.walk(node) if isinstance(n, ast.Name)} & defined) - {name} for name, node in assignments}
    out, done, pending = [], set(), list(assignments)
    while pending:
        rest = [(n, e) for n, e in pending if not deps[n] <= done]
        ready = [(n, e) for n, e in pending if deps[n] <= done]
        if not ready:
            raise ValueError(f"cyclic definitions: {[n for n, _ in rest]}")
        for n, e in ready:
            out.append((n, e))
            done.add(n)
        pending = rest
    return out


def _on_gpu() -> bool:
    """Is there a GPU to run a kernel on?  (Without one -- or without torch -- the handle evaluates with NumPy.)"""
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


class _Body:
    """The body of a generated function as it is being written (the step's, a monitor selection's): the printer, the file's
    states, parameters and time as y_k / p_k / t, the common subexpressions ``repl`` in those symbols, the ``lines`` so far and the
    symbols they use.

    ``second_of``: the body of a two-stage step's first stage.  This one then CONTINUES it -- same printer, same ``lines`` -- with
    the same expressions at the midpoint: the states as yh_k, the time as th, and every common subexpression that depends on a
    state or on the time under a name of its own (x_7 -> xh_7).  One that depends on parameters alone keeps its name and is not
    printed again where the first stage has it."""

    def __init__(self, model, repl, second_of=None):
        import sympy

        y, p = model._sym["y"], model._sym["p"]
        self.ns, self.np, self.nin = len(y), len(p), len(model._sym["m"])
        # a missing variable is input row S + j of the state array: y_{S+j} in either stage (held at its step-start value)
        inputs = {s: sympy.Symbol(f"y_{self.ns + j}") for j, s in enumerate(model._sym["m"])}
        if second_of is None:
            self.pr, self.uses_mod = model._printer()
            self.sub = {s: sympy.Symbol(f"y_{k}") for k, s in enumerate(y)}
            self.sub.update({s: sympy.Symbol(f"p_{k}") for k, s in enumerate(p)})
            self.sub[model._sym["t"]] = sympy.Symbol("t")
            self.sub.update(inputs)
            self.temp = {lhs: e.xreplace(self.sub) for lhs, e in repl}
            self.lines = []
        else:
            self.pr, self.uses_mod, self.lines = second_of.pr, second_of.uses_mod, second_of.lines
            moving = {s for s in y} | {model._sym["t"]}
            for lhs, e in repl:  # (in definition order: what a moving temporary is used in moves too)
                if e.free_symbols & moving:
                    moving.add(lhs)
            self.sub = {s: sympy.Symbol(f"yh_{k}") for k, s in enumerate(y)}
            self.sub.update({s: sympy.Symbol(f"p_{k}") for k, s in enumerate(p)})
            self.sub[model._sym["t"]] = sympy.Symbol("th")
            self.sub.update({lhs: sympy.Symbol(str(lhs).replace("x_", "xh_")) for lhs, _ in repl if lhs in moving})
            self.sub.update(inputs)
            self.temp = {lhs.xreplace(self.sub): e.xreplace(self.sub) for lhs, e in repl}
        self.emit, self.emitted = model._emitter(self.temp, self.pr, self.lines)
        if second_of is not None:
            self.emitted |= second_of.emitted  # (the parameter-only temporaries the first stage has defined)
        self.used = set()

    def expr(self, e):
        """``e`` in the body's symbols: the temporaries it needs are emitted, its symbols noted as used."""
        import sympy

        e = sympy.sympify(e).xreplace(self.sub)
        self.emit(e)
        self.used |= e.free_symbols
        return e

    def loads(self, every_state: bool):
        """The load lines of the states (all of them, or the used ones), of the used input rows (a model's missing variables:
        rows S .. S + M - 1, read and never stored) and of the used parameters, once the body is written."""
        import sympy

        for e in self.emitted:
            if e in self.temp:  # (a second stage's set also names the first stage's temporaries: that body accounts for them)
                self.used |= self.temp[e].free_symbols
        return ([f"    const double y_{k} = io.load({k});" for k in range(self.ns + self.nin)
                 if (every_state and k < self.ns) or sympy.Symbol(f"y_{k}") in self.used],
                [f"    const double p_{k} = p[{k}];" for k in range(self.np) if sympy.Symbol(f"p_{k}") in self.used])


class OdeFileModel(DeviceModel):
    """A :class:`DeviceModel` generated from an ``.ode`` file (see the module docstring)."""

    def __init__(self, path, scheme="generalized_rush_larsen", v_name=None, name=None, fast_exp=True, missing=None, missing_ranges=None):
        import sympy

        self.fast_exp = bool(fast_exp)

        scheme = _SCHEME_ALIASES.get(scheme, scheme)
        if scheme not in _SCHEMES:
            raise ValueError(f"scheme must be one of {_SCHEMES}, got {scheme!r}")
        self.path = Path(path)
        self.scheme = scheme
        text = self.path.read_text()
        states, params, assigns = {}, {}, []
        for kind, nm, node in _walk(text, str(self.path)):
            if kind == "call" and nm in ("states", "parameters"):
                target = states if nm == "states" else params
                for kw in node.keywords:
                    target[kw.arg] = _number(kw.value)
            elif kind == "assign":
                assigns.append((nm, node))
            # (expressions(...), component(...), comment(...): grouping only)
        if not states:
            raise ValueError(f"{self.path}: no states(...) found")
        assigns = _dependency_order(assigns)
        self.missing_names = self._missing_names(missing, states, params, assigns)
        self.missing_ranges = {nm: (0.0, 1.0) for nm in self.missing_names}
        for nm, (lo, hi) in (missing_ranges or {}).items():
            if nm not in self.missing_ranges:
                raise ValueError(f"{self.path}: missing_ranges names {nm!r}, which is not a missing variable of this model")
            self.missing_ranges[nm] = (float(lo), float(hi))
        if v_name is None:
            v_name = next((s for s in states if s.lower() in ("v", "vm", "v_m")), None)
        if v_name is not None and v_name not in states:
            raise KeyError(f"{v_name!r} is not a state of {self.path.name}")
        stem = "".join(c if c.isalnum() else "_" for c in (name or self.path.stem))
        super().__init__(f"{stem}_{scheme}", -1, states, params, v_name)
        # ---- symbolic right-hand sides and total self-derivatives
        ysym = {s: sympy.Symbol(s, real=True) for s in states}
        psym = {p: sympy.Symbol(p, real=True) for p in params}
        msym = {m: sympy.Symbol(m, real=True) for m in self.missing_names}  # constant over a step: J_kk never differentiates by one
        tsym, dtsym = sympy.Symbol("time", real=True), sympy.Symbol("dt", real=True)

        def piecewise(c, a, b):
            return sympy.Piecewise((a, c), (b, True))

        ns = {nm: getattr(sympy, _SYMPY_NAMES.get(nm, nm)) for nm in _FUNCTIONS if nm != "Conditional"}
        ns.update({"Conditional": piecewise, "time": tsym, "t": tsym, "pi": sympy.pi,
                   "_indicator": lambda c: sympy.Piecewise((sympy.Integer(1), c), (sympy.Integer(0), True))})
        ns.update(psym)
        ns.update(msym)
        ns.update(ysym)
        rhs, line, assigned = {}, {}, {}
        for nm, node in assigns:
            _check_expression(node, str(self.path), set(_FUNCTIONS))
            node = ast.fix_missing_locations(_ComparisonsAsNumbers(str(self.path)).visit(node))
            try:
                expr = sympy.sympify(eval(compile(ast.Expression(node), str(self.path), "eval"), {"__builtins__": {}}, ns))
            except Exception as exc:  # noqa: BLE001
                raise ValueError(f"{self.path}: cannot turn `{nm} = ...` into an expression: {exc}") from exc
            ns[nm] = assigned[nm] = expr
            if nm.startswith("d") and nm.endswith("_dt") and nm[1:-3] in states:
                rhs[nm[1:-3]], line[nm[1:-3]] = expr, node.lineno
        missing = [s for s in states if s not in rhs]
        if missing:
            raise ValueError(f"{self.path}: no d<state>_dt for {missing}")
        names = list(states)
        f = [rhs[s] for s in names]
        J = [self._self_derivative(rhs[s], ysym[s], f"{self.path}:{line[s]}: d{s}_dt") if scheme in _RUSH_LARSEN
             else sympy.Integer(0) for s in names]
        self._grl = [bool(j != 0) for j in J]
        repl, red = sympy.cse(f + J, symbols=sympy.numbered_symbols("x_"), optimizations="basic")
        self._sym = dict(y=[ysym[s] for s in names], p=[psym[p] for p in params], m=[msym[m] for m in self.missing_names], t=tsym, dt=dtsym, repl=repl,
                         f=red[: len(names)], J=red[len(names):])
        # every assignment of the file, in dependency order: what monitor_values / numpy_monitor can be asked for
        self.monitor_names = tuple(assigned)
        self._mon_expr = assigned
        self._mon_numpy_fn = None
        self._monitors = {}       # names of one launch -> the library's monitor id (beat_ode_monitor_register), once self-checked
        self._stem = stem
        self._numpy_fn = None
        self._registered = None   # the library's id, once the compiled kernel has passed _self_check
        self._library_id = None   # the id beat_ode_model_register gave (the source is handed over once per process)
        self.source = self._cxx(stem)
        self.key = f"{self.cxx_name}"

    def _missing_names(self, missing, states, params, assigns) -> tuple:
        """The names ``missing`` declares (None: none; "auto": every free name of the file, sorted), checked: a ValueError names the
        file and the name that is declared or assigned in the file, reserved, used by nothing, or given twice."""
        if missing is None:
            return ()
        assigned = {nm for nm, _ in assigns}
        reserved = set(_FUNCTIONS) | set(_CONSTANTS) | {"dt"}
        used = {n.id for _, node in assigns for n in ast.walk(node) if isinstance(n, ast.Name)}
        if isinstance(missing, str):
            if missing != "auto":
                missing = (missing,)
            else:
                return tuple(sorted(used - set(states) - set(params) - assigned - reserved))
        out = []
        for nm in missing:
            if not isinstance(nm, str) or not nm.isidentifier():
                raise ValueError(f"{self.path}: {nm!r} is not the name of a missing variable")
            if nm in out:
                raise ValueError(f"{self.path}: missing variable {nm!r} is given twice")
            for what, where in (("a state", states), ("a parameter", params), ("assigned", assigned), ("a reserved name", reserved)):
                if nm in where:
                    raise ValueError(f"{self.path}: {nm!r} cannot be a missing variable: it is {what} in the file")
            if nm not in used:
                raise ValueError(f"{self.path}: missing variable {nm!r} is used by no expression of the file")
            out.append(nm)
        return tuple(out)

    @property
    def num_missing_variables(self) -> int:
        return len(self.missing_names)

    @property
    def num_rows(self) -> int:
        """Rows of the state array the kernel works on: the states, then one input row per missing variable."""
        return self.num_states + self.num_missing_variables

    def missing_index(self, name: str) -> int:
        try:
            return self.missing_names.index(name)
        except ValueError:
            raise KeyError(f"Unknown missing variable {name}") from None

    def init_missing_values(self, **values) -> np.ndarray:
        """An (M,) vector of the missing variables in the order of ``missing_names``: 0.0 but for the ones given by name."""
        d = dict.fromkeys(self.missing_names, 0.0)
        for k, v in values.items():
            if k not in d:
                raise KeyError(f"Unknown missing variable {k}")
            d[k] = v
        return np.array([d[k] for k in self.missing_names], dtype=np.float64)

    def _rows(self, states, missing_variables):
        """(S + M, N) rows for the kernel -- ``states`` (S,) or (S, N) above ``missing_variables`` (M,) or (M, N) -- and whether
        ``states`` was (S,).  TypeError where the model has missing variables and gets none, or has none and gets some."""
        m = self.num_missing_variables
        if m == 0:
            if missing_variables is not None:
                raise TypeError(f"{self.name} has no missing variables: missing_variables must not be given")
            y = np.asarray(states, dtype=np.float64)
            return y.reshape(y.shape[0], -1), y.ndim == 1
        if missing_variables is None:
            raise TypeError(f"{self.name} has the missing variables {self.missing_names}: missing_variables=... is required")
        y = np.asarray(states, dtype=np.float64)
        y2 = y.reshape(y.shape[0], -1)
        if y2.shape[0] != self.num_states:
            raise ValueError(f"{self.name} has {self.num_states} states, got {y2.shape[0]}")
        c = np.asarray(missing_variables, dtype=np.float64)
        if c.shape not in ((m,), (m, y2.shape[1])):
            raise ValueError(f"missing_variables must have shape ({m},) or ({m}, {y2.shape[1]}), got {c.shape}")
        return np.concatenate([y2, np.broadcast_to(c.reshape(m, -1), (m, y2.shape[1]))], axis=0), y.ndim == 1

    @staticmethod
    def _self_derivative(expr, y, where: str):
        """d expr / d y, or a ValueError naming the equation: floor and % have no derivative the generator can print (SymPy
        leaves ``Derivative(floor(y), y)`` in the result or refuses outright), and none is made up for them here."""
        import sympy

        try:
            j = sympy.diff(expr, y)
        except Exception as exc:  # noqa: BLE001
            raise ValueError(f"{where}: cannot differentiate with respect to the state {y}: {exc}") from exc
        if j.has(sympy.Derivative, sympy.Subs):
            raise ValueError(f"{where}: the derivative with respect to the state {y} is not one the generator can print "
                             f"({next(iter(j.atoms(sympy.Derivative, sympy.Subs)))}): floor and % of a state have none")
        return j

    # ------------------------------------------------------------------------------------------------ C++
    def _printer(self):
        """The C++ printer of the generated code (the step's and the monitors') and the list it notes a use of ``%`` in."""
        import os

        from sympy.printing.c import C99CodePrinter

        class Printer(C99CodePrinter):
            def _print_Pow(self, expr):  # small integer powers as products (pow() on fp64 is a long software routine)
                b, e = expr.as_base_exp()
                if e.is_Integer and 2 <= int(e) <= 4:
                    pb = self.parenthesize(b, 1000)  # as an atom
                    return "(" + "*".join([pb] * int(e)) + ")"
                if e.is_Integer and -4 <= int(e) <= -1:
                    pb = self.parenthesize(b, 1000)
                    return "(1.0/(" + "*".join([pb] * (-int(e))) + "))"
                return super()._print_Pow(expr)

            def _print_Mod(self, expr):  # Python's %, as NumPy evaluates it (np.mod): the result takes the divisor's sign
                uses_mod.append(True)
                a, b = expr.args
                return f"beat_mod({self._print(a)}, {self._print(b)})"

            def _print_Piecewise(self, expr):
                # BRANCH-FREE: both arms evaluated, the result selected (v_cndmask).  As `c ? a : b` with the arms inline the
                # compiler builds divergent branches; a heavily spilled kernel (the reference's ToR-ORd files generate 250 - 300 spilled
                # SGPRs and 450 spilled VGPRs) then reloads registers it spilled under another lane mask -- wrong values on exactly the
                # nodes that take the other arm, in the states behind that arm, different from run to run (ROCm 7.2; seen in round 1
                # on the generated ToR-ORd kernel and reproduced in round 5: tools/diag_spill.py, profiles/r05_generated_spills.md).
                # A lane computes both arms of a divergent branch anyway.
                if os.environ.get("BEAT_ODE_BRANCHES") == "1":  # the form that was seen miscompiled (tests of the self checks)
                    return super()._print_Piecewise(expr)
                args = list(expr.args)
                out = self._print(args[-1][0])
                if args[-1][1] != True:  # noqa: E712 -- no default arm: what C's chained ?: would leave undefined
                    out = f"beat_sel({self._print(args[-1][1])}, {out}, 0.0)"
                for e, c in reversed(args[:-1]):
                    out = f"beat_sel({self._print(c)}, {self._print(e)}, {out})"
                return out

        # exp(): the library's table-driven evaluation (FastMath::exp of csrc/ionic_models.h, what the shipped models use: 13 VALU
        # instructions, <= 1 ulp, the 256-entry table in LDS) with the argument kept inside double range -- or libm's
        uses_mod = []
        return Printer({"contract": False, "user_functions": {"exp": "fexp" if self.fast_exp else "exp"}}), uses_mod

    @staticmethod
    def _emitter(temp, pr, lines):
        """``emit(expr)``: the common subexpressions ``expr`` needs and that are not out yet, appended to ``lines`` depth first --
        a temporary is defined next to its first use -- and the set of those emitted so far."""
        emitted = set()

        def emit(expr):
            stack = [(sym, False) for sym in sorted(expr.free_symbols, key=str, reverse=True) if sym in temp]
            while stack:
                sym, done = stack.pop()
                if sym in emitted:
                    continue
                if done:
                    emitted.add(sym)
                    lines.append(f"    const double {sym} = {pr.doprint(temp[sym])};")
                    continue
                stack.append((sym, True))
                for dep in sorted(temp[sym].free_symbols, key=str, reverse=True):
                    if dep in temp and dep not in emitted:
                        stack.append((dep, False))

        return emit, emitted

    def _cxx_helpers(self, uses_mod) -> str:
        """The lambdas the printed expressions call (fexp, beat_sel, beat_mod), as the first lines of a generated function body."""
        return (("    // (what libm / NumPy give everywhere: NaN stays NaN, overflow is inf, underflow goes through the subnormals to 0)\n"
                 "    // (k = round(x 256 / ln 2) must fit 32 bits: the clamp; inside it v_ldexp_f64 underflows to 0 through the subnormals and\n"
                 "    // overflows to inf as libm does; the clamp turns a NaN argument into a number, hence the select)\n"
                 "    const auto fexp = [&fm](double x) { const double e = fm.exp(fmin(fmax(x, -1.0e6), 1.0e3)); return x != x ? x : e; };\n" if self.fast_exp else "")
                + "    const auto beat_sel = [](bool c, double a, double b) { return c ? a : b; };\n"
                + ("    // (a % b with Python's and NumPy's meaning: fmod's result moved by b where it has the other sign; a zero takes b's sign)\n"
                   "    const auto beat_mod = [](double a, double b) {\n"
                   "      const double m = fmod(a, b);\n"
                   "      return m != 0.0 ? ((m < 0.0) != (b < 0.0) ? m + b : m) : copysign(0.0, b);\n"
                   "    };\n" if uses_mod else ""))

    def _cxx_one_stage(self, body, order, exp_name) -> None:
        """The lines of GRL1's and forward Euler's step, appended to ``body``'s (states in ``order``): per state its temporaries, the
        update and its store."""
        import os

        pr, lines = body.pr, body.lines
        for k in order:
            fk, jk = body.expr(self._sym["f"][k]), body.expr(self._sym["J"][k])
            if self._grl[k]:
                if os.environ.get("BEAT_ODE_BRANCHES") == "1":  # (the former output: see _print_Piecewise)
                    lines.append(f"    {{ const double f = {pr.doprint(fk)}; const double J = {pr.doprint(jk)};\n"
                                 f"      io.store({k}, y_{k} + (fabs(J) > 1e-8 ? f / J * ({exp_name}(J * dt) - 1.0) : f * dt)); }}")
                    continue
                lines.append(f"    {{ const double f = {pr.doprint(fk)}; const double J = {pr.doprint(jk)};\n"
                             f"      io.store({k}, y_{k} + beat_sel(fabs(J) > 1e-8, f / J * ({exp_name}(J * dt) - 1.0), f * dt)); }}")
            else:
                lines.append(f"    io.store({k}, y_{k} + dt * ({pr.doprint(fk)}));")

    def _cxx_two_stages(self, body, order, exp_name) -> None:
        """The lines of GRL2's step, appended to ``body``'s (states in ``order``).  Stage 1, state by state: f_k and J_kk at
        (y, t) and the midpoint value yh_k = y_k + phi(J, dt/2) f (GRL1 over half a step; y_k + dt/2 f where J_kk is
        identically zero) -- f and J are scoped to their state, so what stays live is the NS values yh_k next to the loaded y_k.
        Stage 2, in the one-stage schemes' order: the same expressions at (yh, t + dt/2) under names of their own
        (``_Body(second_of=...)``), b = f + J (y_k - yh_k), and y_k + phi(J, dt) b stored as soon as it is final.  y_k is the
        value loaded at the top of the step in both stages: nothing is loaded a second time (on the fused route the potential's
        load applies the pending update, and the row is overwritten in place)."""
        import os

        pr, lines = body.pr, body.lines
        branches = os.environ.get("BEAT_ODE_BRANCHES") == "1"  # (the former output: see _print_Piecewise)

        def phi_times(h):  # phi(J, h) f in GRL1's operation order
            grl, euler = f"f / J * ({exp_name}(J * {h}) - 1.0)", f"f * {h}"
            return f"(fabs(J) > 1e-8 ? {grl} : {euler})" if branches else f"beat_sel(fabs(J) > 1e-8, {grl}, {euler})"

        lines.append("    const double hdt = 0.5 * dt, th = t + hdt;  // stage 1: GRL1 over half a step, from (y, t)")
        for k in order:
            fk, jk = body.expr(self._sym["f"][k]), body.expr(self._sym["J"][k])
            if self._grl[k]:
                lines.append(f"    double yh_{k}; {{ const double f = {pr.doprint(fk)}; const double J = {pr.doprint(jk)};\n"
                             f"      yh_{k} = y_{k} + {phi_times('hdt')}; }}")
            else:
                lines.append(f"    const double yh_{k} = y_{k} + hdt * ({pr.doprint(fk)});")
        lines.append("    // stage 2: linearised about (yh, th), integrated from y over the whole step")
        second = _Body(self, self._sym["repl"], second_of=body)
        if os.environ.get("BEAT_ODE_EMIT") == "global":
            for lhs in second.temp:
                second.emit(lhs)
        for k in order:
            fk, jk = second.expr(self._sym["f"][k]), second.expr(self._sym["J"][k])
            if self._grl[k]:
                lines.append(f"    {{ const double J = {pr.doprint(jk)}; const double f = ({pr.doprint(fk)}) + J * (y_{k} - yh_{k});\n"
                             f"      io.store({k}, y_{k} + {phi_times('dt')}); }}")
            else:
                lines.append(f"    io.store({k}, y_{k} + dt * ({pr.doprint(fk)}));")
        second.loads(every_state=False)
        rows = {f"y_{k}" for k in range(body.ns, body.ns + body.nin)}  # (the second stage reads the input rows the first one loaded)
        body.used |= {s for s in second.used if str(s).startswith("p_") or str(s) in rows}

    def _cxx(self, stem: str) -> str:
        import os

        exp_name = "fexp" if self.fast_exp else "exp"
        # Order: state by state, each one's common subexpressions right ahead of its update (depth first, those not yet emitted),
        # then the update and its store -- a temporary is defined next to its first use and a state's result leaves the registers
        # when it is final.  (All temporaries first and all updates last -- the order the elimination returns them in -- keeps every
        # one of them and all NS results alive to the end: the 48-state test model needed 256 + 256 registers and 450 B of scratch
        # per lane that way.)
        body = _Body(self, self._sym["repl"])
        lines, ns_, np_ = body.lines, body.ns, body.np
        vi = self.state_index(self.v_name) if self.v_name else 0
        order = list(range(ns_))
        if os.environ.get("BEAT_ODE_V_LAST", "1") == "1" and self.v_name:  # the potential's equation sums every current: last, when the currents exist
            order = [k for k in order if k != vi] + [vi]
        if os.environ.get("BEAT_ODE_EMIT") == "global":  # every temporary first, in the elimination's order (tests: the heavily spilled form)
            for lhs in body.temp:
                body.emit(lhs)
            order = list(range(ns_))
        if self.scheme == "generalized_rush_larsen_2":
            self._cxx_two_stages(body, order, exp_name)
        else:
            self._cxx_one_stage(body, order, exp_name)
        loads, pl = body.loads(every_state=True)
        # (the missing variables are part of the name -- it is the key of the compiled kernel's cache; without any, the name of before)
        digest = hashlib.sha1(("\n".join(lines) + self.scheme + ("".join(f"|{nm}" for nm in self.missing_names))).encode()).hexdigest()[:12]
        self.cxx_name = f"Ode_{stem}_{digest}"
        nin = body.nin  # (rows NS - NIN .. NS - 1 are inputs: loaded where used, never stored; a model without any prints as before)
        return (f"// generated by beat.models.from_ode from {self.path.name} ({self.scheme}): {ns_} states, {np_} parameters"
                + (f", {nin} missing variables ({', '.join(self.missing_names)}) as input rows {ns_} .. {ns_ + nin - 1}" if nin else "") + "\n"
                f"struct {self.cxx_name} {{\n"
                f"  static constexpr int NS = {ns_ + nin}, NP = {max(np_, 1)}, V_INDEX = {vi};\n"
                + (f"  static constexpr int NIN = {nin};\n" if nin else "") +
                "  static constexpr bool REGISTER_LOOP = true;\n"
                "  static constexpr int WAVES = 1, WAVES_PER_NODE = 1;\n"
                "  struct Derived { double unused; };\n"
                "  template <class P> __host__ __device__ static Derived derive(const P&) { return Derived{0.0}; }\n"
                "  template <class IO, class P>\n"
                "  __device__ static __forceinline__ void step(const IO& io, const P& p, const Derived&, const FastMath& fm, double t, double dt) {\n"
                + self._cxx_helpers(body.uses_mod)
                + "\n".join(loads + pl + lines) + "\n  }\n};\n")

    def _monitor_cxx(self, names):
        """(struct name, source) of ``Mon_<stem>_<digest>`` for csrc/beat_ode_kernel.h's ode_monitor_kernel: the assignments ``names``
        (at most _hip.MAX_MONITORS) evaluated from the node's states and parameters and stored to output rows 0 .. M-1.  Common
        subexpressions are eliminated over the SELECTION alone; printer, helpers and the order -- a temporary next to its first
        use, an output stored as soon as it is final -- are the step's; only the states and parameters the selection uses are
        loaded."""
        import sympy

        repl, red = sympy.cse([self._mon_expr[nm] for nm in names], symbols=sympy.numbered_symbols("x_"), optimizations="basic")
        body = _Body(self, repl)
        lines = body.lines
        for j, e in enumerate(red):
            lines.append(f"    out.store({j}, {body.pr.doprint(body.expr(e))});  // {names[j]}")
        loads, pl = body.loads(every_state=False)
        digest = hashlib.sha1("\n".join(loads + pl + lines).encode()).hexdigest()[:12]
        name = f"Mon_{self._stem}_{digest}"
        return name, (f"// generated by beat.models.from_ode from {self.path.name}: {len(names)} monitored values, {len(loads)} of {body.ns + body.nin} "
                      f"{'state and input rows' if body.nin else 'states'} read\n"
                      f"struct {name} {{\n"
                      f"  static constexpr int NS = {body.ns + body.nin}, NP = {max(body.np, 1)}, NM = {len(names)};\n"
                      "  template <class IO, class P, class OUT>\n"
                      "  __device__ static __forceinline__ void eval(const IO& io, const P& p, const FastMath& fm, double t, const OUT& out) {\n"
                      + self._cxx_helpers(body.uses_mod)
                      + "\n".join(loads + pl + lines) + "\n  }\n};\n")

    def monitor_sources(self, names=None):
        """[(struct name, source, names)] -- one per launch: ``names`` (None: all) in runs of at most _hip.MAX_MONITORS."""
        from .. import _hip

        names = self._monitor_selection(names)
        return [self._monitor_cxx(names[k:k + _hip.MAX_MONITORS]) + (tuple(names[k:k + _hip.MAX_MONITORS]),)
                for k in range(0, len(names), _hip.MAX_MONITORS)]

    # ------------------------------------------------------------------------------------------------ NumPy
    def _numpy_args(self, states, t, parameters, missing_variables=None):
        """(states as (S, N), the arguments of a lambdified function over y + m + p + [t] -- m: the missing variables, none for
        most models --, whether ``states`` was (S,))."""
        rows, one_d = self._rows(states, missing_variables)
        y2, m2 = rows[: rows.shape[0] - self.num_missing_variables], rows[rows.shape[0] - self.num_missing_variables:]
        p = np.asarray(parameters, dtype=np.float64)  # (P,) or per node (P, N)
        if p.ndim == 2 and p.shape[1] != y2.shape[1]:
            raise ValueError(f"per-node parameters must have shape ({len(p)}, {y2.shape[1]}), got {p.shape}")
        # (every argument an array of the nodes' shape: NumPy's and / or of a condition on parameters alone with one on a state
        # would otherwise be a reduction over a ragged pair)
        n = y2.shape[1]
        pn = [np.broadcast_to(np.asarray(p[k], dtype=np.float64), (n,)) for k in range(len(p))]
        return y2, [y2[k] for k in range(y2.shape[0])] + [m2[k] for k in range(m2.shape[0])] + pn + [np.full(n, float(t))], one_d

    @staticmethod
    def _numpy_printer():
        """lambdify's NumPy printer with every constant at full precision: the stock one writes a Float with 15 significant
        digits (0.147058823529412 for 1/6.8), which moves exp(c V) by 2e-14 of its value at V = -95 -- the generated C++ has 17."""
        from sympy.printing.numpy import NumPyPrinter

        class FullPrecision(NumPyPrinter):
            def _print_Float(self, expr):
                return repr(float(expr))

        return FullPrecision({"fully_qualified_modules": False, "inline": True, "allow_unknown_functions": True})

    def _numpy_rhs(self):
        """The lambdified right-hand sides f and self-derivatives J (what numpy_step integrates)."""
        import sympy

        if self._numpy_fn is None:
            s = self._sym
            # (the common subexpressions found at construction are handed to lambdify as they are: local assignments in the generated function)
            self._numpy_fn = sympy.lambdify(s["y"] + s["m"] + s["p"] + [s["t"]], [s["f"], s["J"]], "numpy", cse=lambda exprs: (s["repl"], exprs),
                                            printer=self._numpy_printer())
        return self._numpy_fn

    def numpy_step(self, states, t, parameters, dt, missing_variables=None):
        """One step on the HOST with NumPy: the same expressions as the kernel's (the reference's way of evaluating ``fun``).
        ``missing_variables``: (M,) or (M, N), for a model made with ``missing=`` (TypeError where such a model gets none, or
        another model gets some); held at these values through both stages of GRL2.  Returns the S states."""
        y2, args, one_d = self._numpy_args(states, t, parameters, missing_variables)
        ns = y2.shape[0]
        if self.scheme == "generalized_rush_larsen_2":
            # stage 1 is the GRL1 step over dt / 2 (forward Euler where J_kk is identically zero); stage 2 takes f and J at
            # (yh, t + dt / 2) and integrates b = f + J (y - yh) from y over dt -- the kernel's two stages, operation by operation
            hdt = 0.5 * dt
            yh = self._numpy_update(y2, args, hdt)
            mid = [yh[k] for k in range(ns)] + args[ns:-1] + [np.full(y2.shape[1], float(t) + hdt)]
            out = self._numpy_update(y2, mid, dt, about=yh)
        else:
            out = self._numpy_update(y2, args, dt)
        return out[:, 0].copy() if one_d else out

    def _numpy_update(self, y2, args, dt, about=None):
        """y + phi(J, dt) b per state (y + dt b where J_kk is identically zero), f and J evaluated at ``args``:
        b = f, or f + J (y - about) for a linearisation about another point than y."""
        with np.errstate(all="ignore"):
            f, J = self._numpy_rhs()(*args)
        out = np.empty_like(y2)
        for k in range(y2.shape[0]):
            fk = np.broadcast_to(np.asarray(f[k], dtype=np.float64), y2[k].shape)
            if self._grl[k]:
                Jk = np.broadcast_to(np.asarray(J[k], dtype=np.float64), y2[k].shape)
                with np.errstate(all="ignore"):
                    if about is not None:
                        fk = fk + Jk * (y2[k] - about[k])
                    out[k] = y2[k] + np.where(np.abs(Jk) > 1e-8, fk / np.where(Jk == 0, 1.0, Jk) * (np.exp(Jk * dt) - 1.0), fk * dt)
            else:
                out[k] = y2[k] + dt * fk
        return out

    def monitor_index(self, name: str) -> int:
        try:
            return self.monitor_names.index(name)
        except ValueError:
            raise KeyError(f"Unknown monitor {name}") from None

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
        states, (M, N) for (S, N); parameters (P,) or per node (P, N).  What the monitor kernel is compared with, as ``numpy_step``
        is for the step.  The ``d<state>_dt`` rows are the right-hand sides ``numpy_step`` integrates, bit for bit (the same
        lambdified function); every other row comes from ONE function over all assignments, so that a selection gives the numbers
        of the matching rows of ``names=None``.  ``missing_variables``: as for ``numpy_step``."""
        import sympy

        names = self._monitor_selection(names)
        y2, args, one_d = self._numpy_args(states, t, parameters, missing_variables)
        n = y2.shape[1]
        rhs_row = {f"d{s}_dt": k for k, s in enumerate(self.state_names)}
        plain = [nm for nm in self.monitor_names if nm not in rhs_row]
        out = np.empty((len(names), n))
        with np.errstate(all="ignore"):
            if any(nm in rhs_row for nm in names):
                f, _ = self._numpy_rhs()(*args)
            if any(nm not in rhs_row for nm in names):
                if self._mon_numpy_fn is None:
                    s = self._sym
                    self._mon_numpy_fn = sympy.lambdify(s["y"] + s["m"] + s["p"] + [s["t"]], [self._mon_expr[nm] for nm in plain], "numpy", cse=True,
                                                        printer=self._numpy_printer())
                vals = dict(zip(plain, self._mon_numpy_fn(*args)))
        for j, nm in enumerate(names):
            out[j] = np.broadcast_to(np.asarray(f[rhs_row[nm]] if nm in rhs_row else vals[nm], dtype=np.float64), (n,))
        return out[:, 0].copy() if one_d else out

    # ------------------------------------------------------------------------------------------------ device
    def register(self) -> int:
        """The library's id for this model (beat_ode_model_register: the source is handed over once per process; the kernel is
        compiled when a step first needs it).  Raises BeatHipError where the library cannot compile at run time."""
        from .. import _hip

        if self._registered is None:
            if self._library_id is None:
                lib = _hip.load()
                mid = C.c_int(-1)
                _hip.check(lib.beat_ode_model_register(self.cxx_name.encode(), self.source.encode(), self.num_rows,
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
        S = self.num_states
        return rows[:S], (rows[S:] if self.missing_names else None)

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
        err = np.where(ok, np.where(np.isfinite(dev), err, np.inf), 0.0)
        return err

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
