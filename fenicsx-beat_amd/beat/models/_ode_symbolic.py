"""The SymPy side of ``beat.models.from_ode``: an :class:`OdeSource` turned into right-hand sides f_k, TOTAL self-derivatives
J_kk = d f_k / d y_k (intermediates resolved) and their common subexpressions, for the C++ writer and the NumPy twin alike."""

import ast
from dataclasses import dataclass

import sympy

from ._ode_parse import _FUNCTIONS, _SYMPY_NAMES, OdeSource

GRL2 = "generalized_rush_larsen_2"
RUSH_LARSEN = ("generalized_rush_larsen", GRL2)  # the schemes that need the self-derivatives J_kk


def _self_derivative(expr, y, where: str):
    """d expr / d y, or a ValueError naming the equation: floor and % have no derivative the generator can print (SymPy
    leaves ``Derivative(floor(y), y)`` in the result or refuses outright), and none is made up for them here."""
    try:
        j = sympy.diff(expr, y)
    except Exception as exc:  # noqa: BLE001
        raise ValueError(f"{where}: cannot differentiate with respect to the state {y}: {exc}") from exc
    if j.has(sympy.Derivative, sympy.Subs):
        raise ValueError(f"{where}: the derivative with respect to the state {y} is not one the generator can print "
                         f"({next(iter(j.atoms(sympy.Derivative, sympy.Subs)))}): floor and % of a state have none")
    return j


@dataclass
class OdeSystem:
    """``y``, ``p``, ``m``, ``t``: the symbols of the states, parameters, missing variables and time.  ``assigned``: every assignment
    (name -> expression, in dependency order: what the monitors select from).  ``f``, ``J``: right-hand sides and self-derivatives
    after the ONE elimination of common subexpressions, ``repl`` its pairs; ``grl[k]``: J_kk is not identically zero."""

    source: OdeSource
    y: list
    p: list
    m: list
    t: sympy.Symbol
    assigned: dict
    f: list
    J: list
    grl: list
    repl: list

    @classmethod
    def from_source(cls, source: OdeSource, scheme: str) -> "OdeSystem":
        path, states = source.path, source.states
        ysym = {s: sympy.Symbol(s, real=True) for s in states}
        psym = {p: sympy.Symbol(p, real=True) for p in source.parameters}
        msym = {m: sympy.Symbol(m, real=True) for m in source.missing_names}  # constant over a step: J_kk never differentiates by one
        tsym = sympy.Symbol("time", real=True)

        ns = {nm: getattr(sympy, _SYMPY_NAMES.get(nm, nm)) for nm in _FUNCTIONS if nm != "Conditional"}
        ns.update({"Conditional": lambda c, a, b: sympy.Piecewise((a, c), (b, True)), "time": tsym, "t": tsym, "pi": sympy.pi,
                   "_indicator": lambda c: sympy.Piecewise((sympy.Integer(1), c), (sympy.Integer(0), True))})
        ns.update({**psym, **msym, **ysym})
        assigned, line = {}, {}
        for nm, node in source.assignments:
            try:  # (the node has passed _check_expression: arithmetic, comparisons and calls of the known functions alone)
                expr = sympy.sympify(eval(compile(ast.Expression(node), str(path), "eval"), {"__builtins__": {}}, ns))
            except Exception as exc:  # noqa: BLE001
                raise ValueError(f"{path}: cannot turn `{nm} = ...` into an expression: {exc}") from exc
            ns[nm] = assigned[nm] = expr
            line[nm] = node.lineno
        missing = [s for s in states if f"d{s}_dt" not in assigned]
        if missing:
            raise ValueError(f"{path}: no d<state>_dt for {missing}")
        f = [assigned[f"d{s}_dt"] for s in states]
        J = [_self_derivative(fk, ysym[s], f"{path}:{line[f'd{s}_dt']}: d{s}_dt") if scheme in RUSH_LARSEN else sympy.Integer(0)
             for s, fk in zip(states, f)]
        repl, red = sympy.cse(f + J, symbols=sympy.numbered_symbols("x_"), optimizations="basic")
        return cls(source, list(ysym.values()), list(psym.values()), list(msym.values()), tsym, assigned,
                   red[: len(f)], red[len(f):], [bool(j != 0) for j in J], repl)
