"""Reading a gotran ``.ode`` file for ``beat.models.from_ode``: ``parse_ode(path, missing) -> OdeSource``.  The format is
Python syntax, so ``ast`` reads it; nothing here evaluates an expression, and this module needs neither SymPy nor NumPy."""

import ast
import copy
from dataclasses import dataclass
from pathlib import Path


def _walk(text: str, where: str):
    tree = ast.parse(text, filename=where)
    for node in tree.body:
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Name):
            yield "call", node.value.func.id, node.value
        elif isinstance(node, ast.Assign):
            if len(node.targets) != 1 or not isinstance(node.targets[0], ast.Name):
                raise ValueError(f"{where}:{node.lineno}: only plain assignments `name = expression` are understood")
            yield "assign", node.targets[0].id, node.value
        elif not isinstance(node, ast.Expr):  # (a docstring / bare constant is passed over)
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
        if isinstance(n, ast.Call) and (not isinstance(n.func, ast.Name) or n.func.id not in known or n.keywords):
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
    return float(ast.literal_eval(node.args[0] if isinstance(node, ast.Call) else node))  # (a call: ScalarParam(value, unit=..., ...))


def _dependency_order(assignments):
    """gotran files may use an intermediate before the line that defines it: order by dependencies (stable)."""
    defined = {name for name, _ in assignments}
    deps = {name: ({n.id for n in ast.walk(node) if isinstance(n, ast.Name)} & defined) - {name} for name, node in assignments}
    out, done, pending = [], set(), list(assignments)
    while pending:
        ready = [(n, e) for n, e in pending if deps[n] <= done]
        pending = [(n, e) for n, e in pending if not deps[n] <= done]
        if not ready:
            raise ValueError(f"cyclic definitions: {[n for n, _ in pending]}")
        out += ready
        done |= {n for n, _ in ready}
    return out


def _missing_names(path, missing, states, params, assigns) -> tuple:
    """The names ``missing`` declares (None: none; "auto": every free name of the file, sorted), checked: a ValueError names the
    file and the name that is declared or assigned in the file, reserved, used by nothing, or given twice."""
    if missing is None:
        return ()
    assigned = {nm for nm, _ in assigns}
    reserved = set(_FUNCTIONS) | set(_CONSTANTS) | {"dt"}
    used = {n.id for _, node in assigns for n in ast.walk(node) if isinstance(n, ast.Name)}
    if isinstance(missing, str):
        if missing == "auto":
            return tuple(sorted(used - set(states) - set(params) - assigned - reserved))
        missing = (missing,)
    out = []
    for nm in missing:
        if not isinstance(nm, str) or not nm.isidentifier():
            raise ValueError(f"{path}: {nm!r} is not the name of a missing variable")
        if nm in out:
            raise ValueError(f"{path}: missing variable {nm!r} is given twice")
        for what, where in (("a state", states), ("a parameter", params), ("assigned", assigned), ("a reserved name", reserved)):
            if nm in where:
                raise ValueError(f"{path}: {nm!r} cannot be a missing variable: it is {what} in the file")
        if nm not in used:
            raise ValueError(f"{path}: missing variable {nm!r} is used by no expression of the file")
        out.append(nm)
    return tuple(out)


@dataclass(frozen=True)
class OdeSource:
    """An ``.ode`` file as read: ``states`` and ``parameters`` (name -> value, in the file's order), ``assignments`` as
    (name, checked and rewritten ``ast`` node) in dependency order, and the names of the missing variables."""

    path: Path
    states: dict
    parameters: dict
    assignments: tuple
    missing_names: tuple


def parse_ode(path, missing=None) -> OdeSource:
    """``path`` read, checked and ordered; ``missing``: ``from_ode``'s.  A ValueError names the file and, where it has one, the line."""
    path = Path(path)
    tables, assigns = {"states": {}, "parameters": {}}, []
    for kind, nm, node in _walk(path.read_text(), str(path)):
        if kind == "call" and nm in tables:
            tables[nm].update((kw.arg, _number(kw.value)) for kw in node.keywords)
        elif kind == "assign":
            assigns.append((nm, node))
        # (expressions(...), component(...), comment(...): grouping only)
    states, params = tables["states"], tables["parameters"]
    if not states:
        raise ValueError(f"{path}: no states(...) found")
    assigns = _dependency_order(assigns)
    names = _missing_names(path, missing, states, params, assigns)  # (from the file's own text: the rewriting below adds names)
    checked = []
    for nm, node in assigns:
        _check_expression(node, str(path), set(_FUNCTIONS))
        checked.append((nm, ast.fix_missing_locations(_ComparisonsAsNumbers(str(path)).visit(node))))
    return OdeSource(path, states, params, tuple(checked), names)
