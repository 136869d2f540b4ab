"""The C++ text of ``beat.models.from_ode``: an :class:`OdeSystem` printed as the ``Model`` struct of a step (``step_struct``)
or as the struct of a selection of monitored values (``monitor_struct``) for ``csrc/beat_ode_kernel.h``."""

import hashlib
import os
from dataclasses import dataclass

import sympy
from sympy.printing.c import C99CodePrinter

from ._ode_symbolic import GRL2, OdeSystem


@dataclass(frozen=True)
class CxxOptions:
    """What decides the text besides the model: ``from_ode``'s ``fast_exp`` and the environment's switches, as a source is generated."""

    fast_exp: bool
    branches: bool     # BEAT_ODE_BRANCHES=1: conditionals as `c ? a : b` (the former output: see _print_Piecewise)
    emit_global: bool  # BEAT_ODE_EMIT=global: every temporary of a step first, in the elimination's order (tests: the heavily spilled form)
    v_last: bool       # BEAT_ODE_V_LAST, on unless 0: the potential's equation sums every current: last, when the currents exist

    @classmethod
    def from_environment(cls, fast_exp: bool) -> "CxxOptions":
        get = os.environ.get
        return cls(bool(fast_exp), get("BEAT_ODE_BRANCHES") == "1", get("BEAT_ODE_EMIT") == "global", get("BEAT_ODE_V_LAST", "1") == "1")


class _Printer(C99CodePrinter):
    """The C++ printer of the generated code (the step's and the monitors'); ``uses_mod``: it has printed a ``%``."""

    def __init__(self, opt: CxxOptions):
        # exp(): the library's table-driven evaluation (FastMath::exp of csrc/ionic_models.h, what the shipped models use: 13 VALU
        # instructions, <= 1 ulp, the 256-entry table in LDS) with the argument kept inside double range -- or libm's
        self.exp_name, self.branches, self.uses_mod = "fexp" if opt.fast_exp else "exp", opt.branches, False
        super().__init__({"contract": False, "user_functions": {"exp": self.exp_name}})

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
        self.uses_mod = True
        return f"beat_mod({self._print(expr.args[0])}, {self._print(expr.args[1])})"

    def _print_Piecewise(self, expr):
        # BRANCH-FREE: both arms evaluated, the result selected (v_cndmask).  As `c ? a : b` with the arms inline the
        # compiler builds divergent branches; a heavily spilled kernel (the reference's ToR-ORd files generate 250 - 300 spilled
        # SGPRs and 450 spilled VGPRs) then reloads registers it spilled under another lane mask -- wrong values on exactly the
        # nodes that take the other arm, in the states behind that arm, different from run to run (ROCm 7.2; seen in round 1
        # on the generated ToR-ORd kernel and reproduced in round 5: tools/diag_spill.py, profiles/r05_generated_spills.md).
        # A lane computes both arms of a divergent branch anyway.
        if self.branches:
            return super()._print_Piecewise(expr)
        args = list(expr.args)
        out = self._print(args[-1][0])
        if args[-1][1] != True:  # noqa: E712 -- no default arm: what C's chained ?: would leave undefined
            out = f"beat_sel({self._print(args[-1][1])}, {out}, 0.0)"
        for e, c in reversed(args[:-1]):
            out = f"beat_sel({self._print(c)}, {self._print(e)}, {out})"
        return out


class _Body:
    """The body of a generated function as it is being written (the step's, a monitor selection's): the printer, the file's
    states, parameters and time as y_k / p_k / t, the common subexpressions ``repl`` in those symbols, the ``lines`` so far and the
    symbols they use.

    ``second_of``: the body of a two-stage step's first stage.  This one then CONTINUES it -- same printer, same ``lines`` -- with
    the same expressions at the midpoint: the states as yh_k, the time as th, and every common subexpression that depends on a
    state or on the time under a name of its own (x_7 -> xh_7).  One that depends on parameters alone keeps its name and is not
    printed again where the first stage has it."""

    def __init__(self, system: OdeSystem, repl, opt: CxxOptions, second_of=None):
        first = second_of is None
        self.system, self.opt = system, opt
        self.ns, self.np, self.nin = len(system.y), len(system.p), len(system.m)
        self.pr, self.lines = (_Printer(opt), []) if first else (second_of.pr, second_of.lines)
        self.sub = {s: sympy.Symbol(f"y_{k}" if first else f"yh_{k}") for k, s in enumerate(system.y)}
        self.sub.update({s: sympy.Symbol(f"p_{k}") for k, s in enumerate(system.p)})
        self.sub[system.t] = sympy.Symbol("t" if first else "th")
        # a missing variable is input row S + j of the state array: y_{S+j} in either stage (held at its step-start value)
        self.sub.update({s: sympy.Symbol(f"y_{self.ns + j}") for j, s in enumerate(system.m)})
        if not first:
            moving = set(system.y) | {system.t}
            for lhs, e in repl:  # (in definition order: what a moving temporary is used in moves too)
                if e.free_symbols & moving:
                    moving.add(lhs)
            self.sub.update({lhs: sympy.Symbol(str(lhs).replace("x_", "xh_")) for lhs, _ in repl if lhs in moving})
        self.temp = {lhs.xreplace(self.sub): e.xreplace(self.sub) for lhs, e in repl}
        # the temporaries that are out (a second stage starts with the parameter-only ones the first stage has defined)
        self.emitted = set() if first else set(second_of.emitted)
        self.used = set()

    def emit(self, expr) -> None:
        """The common subexpressions ``expr`` needs and that are not out yet, appended to ``lines`` depth first."""
        temp, emitted = self.temp, self.emitted
        stack = [(sym, False) for sym in sorted(expr.free_symbols, key=str, reverse=True) if sym in temp]
        while stack:
            sym, done = stack.pop()
            if sym in emitted:
                continue
            if done:
                emitted.add(sym)
                self.lines.append(f"    const double {sym} = {self.pr.doprint(temp[sym])};")
                continue
            stack.append((sym, True))
            for dep in sorted(temp[sym].free_symbols, key=str, reverse=True):
                if dep in temp and dep not in emitted:
                    stack.append((dep, False))

    def emit_all(self) -> None:  # (every temporary now, in the elimination's order: CxxOptions.emit_global)
        for lhs in self.temp:
            self.emit(lhs)

    def expr(self, e):
        """``e`` in the body's symbols: the temporaries it needs are emitted, its symbols noted as used."""
        e = sympy.sympify(e).xreplace(self.sub)
        self.emit(e)
        self.used |= e.free_symbols
        return e

    def loads(self, every_state: bool):
        """The load lines of the states (all of them, or the used ones) and of the used input rows (a model's missing variables:
        rows S .. S + M - 1, read and never stored), and those of the used parameters, once the body is written."""
        for e in self.emitted:
            if e in self.temp:  # (a second stage's set also names the first stage's temporaries: that body accounts for them)
                self.used |= self.temp[e].free_symbols
        return ([f"    const double y_{k} = io.load({k});" for k in range(self.ns + self.nin)
                 if (every_state and k < self.ns) or sympy.Symbol(f"y_{k}") in self.used],
                [f"    const double p_{k} = p[{k}];" for k in range(self.np) if sympy.Symbol(f"p_{k}") in self.used])


def _function(body: _Body, loads) -> str:
    """A generated function from its first line to the struct's end: the lambdas the expressions call, ``loads``, the body's lines."""
    return (("    // (what libm / NumPy give everywhere: NaN stays NaN, overflow is inf, underflow goes through the subnormals to 0)\n"
             "    // (k = round(x 256 / ln 2) must fit 32 bits: the clamp; inside it v_ldexp_f64 underflows to 0 through the subnormals and\n"
             "    // overflows to inf as libm does; the clamp turns a NaN argument into a number, hence the select)\n"
             "    const auto fexp = [&fm](double x) { const double e = fm.exp(fmin(fmax(x, -1.0e6), 1.0e3)); return x != x ? x : e; };\n" if body.opt.fast_exp else "")
            + "    const auto beat_sel = [](bool c, double a, double b) { return c ? a : b; };\n"
            + ("    // (a % b with Python's and NumPy's meaning: fmod's result moved by b where it has the other sign; a zero takes b's sign)\n"
               "    const auto beat_mod = [](double a, double b) {\n"
               "      const double m = fmod(a, b);\n"
               "      return m != 0.0 ? ((m < 0.0) != (b < 0.0) ? m + b : m) : copysign(0.0, b);\n"
               "    };\n" if body.pr.uses_mod else "")
            + "\n".join(loads + body.lines) + "\n  }\n};\n")


def _name(kind: str, stem: str, text: str) -> str:  # (a generated struct's name: the key of the compiled kernel's cache)
    return f"{kind}_{stem}_{hashlib.sha1(text.encode()).hexdigest()[:12]}"


def _phi_times(pr: _Printer, h: str) -> str:
    """phi(J, h) f in GRL1's operation order: f / J (exp(J h) - 1) where |J| > 1e-8, f h elsewhere."""
    grl, euler = f"f / J * ({pr.exp_name}(J * {h}) - 1.0)", f"f * {h}"
    return f"(fabs(J) > 1e-8 ? {grl} : {euler})" if pr.branches else f"beat_sel(fabs(J) > 1e-8, {grl}, {euler})"


def _stage(body: _Body, order, h: str, about: bool, store: bool) -> None:
    """One stage, appended to ``body``'s lines -- the mirror of the twin's ``update``.  For the states in ``order``: f_k and J_kk
    at this body's point, then y_k + phi(J, ``h``) b (y_k + ``h`` f where J_kk is identically zero), with b = f, or
    f + J (y_k - yh_k) for ``about``: linearised about the midpoint, integrated from y.  ``store``: the result is stored;
    otherwise it is kept as yh_k, f and J scoped to their state: what stays live is the NS values yh_k next to the loaded y_k."""
    pr, system = body.pr, body.system
    for k in order:
        fk, jk = body.expr(system.f[k]), body.expr(system.J[k])
        if not system.grl[k]:
            body.lines.append(f"    io.store({k}, y_{k} + {h} * ({pr.doprint(fk)}));" if store else f"    const double yh_{k} = y_{k} + {h} * ({pr.doprint(fk)});")
            continue
        b = (f"const double J = {pr.doprint(jk)}; const double f = ({pr.doprint(fk)}) + J * (y_{k} - yh_{k});" if about
             else f"const double f = {pr.doprint(fk)}; const double J = {pr.doprint(jk)};")
        result = f"y_{k} + {_phi_times(pr, h)}"
        body.lines.append(f"    {{ {b}\n      io.store({k}, {result}); }}" if store else f"    double yh_{k}; {{ {b}\n      yh_{k} = {result}; }}")


def step_struct(system: OdeSystem, scheme: str, stem: str, v_index, opt: CxxOptions) -> tuple:
    """(struct name, source) of ``Ode_<stem>_<digest>``, the ``Model`` of csrc/beat_ode_kernel.h's step kernels; ``v_index``: the
    potential's state, or None.  Forward Euler and GRL1 are one stage, GRL2 two, with y_k the value loaded at the top in both:
    nothing is loaded twice (on the fused route the potential's load applies the pending update; the row is overwritten in place)."""
    # Order: state by state, each one's common subexpressions right ahead of its update (depth first, those not yet emitted),
    # then the update and its store -- a temporary is defined next to its first use and a state's result leaves the registers
    # when it is final.  (All temporaries first and all updates last -- the order the elimination returns them in -- keeps every
    # one of them and all NS results alive to the end: the 48-state test model needed 256 + 256 registers and 450 B of scratch
    # per lane that way.)
    body = _Body(system, system.repl, opt)
    ns_, np_, nin, missing = body.ns, body.np, body.nin, system.source.missing_names
    order = list(range(ns_))
    if opt.emit_global:
        body.emit_all()
    elif opt.v_last and v_index is not None:
        order = [k for k in order if k != v_index] + [v_index]
    if scheme == GRL2:
        body.lines.append("    const double hdt = 0.5 * dt, th = t + hdt;  // stage 1: GRL1 over half a step, from (y, t)")
        _stage(body, order, "hdt", about=False, store=False)
        body.lines.append("    // stage 2: linearised about (yh, th), integrated from y over the whole step")
        second = _Body(system, system.repl, opt, second_of=body)
        if opt.emit_global:
            second.emit_all()
        _stage(second, order, "dt", about=True, store=True)
        second.loads(every_state=False)
        inputs = {f"y_{k}" for k in range(ns_, ns_ + nin)}  # (the second stage reads the input rows the first one loaded)
        body.used |= {s for s in second.used if str(s).startswith("p_") or str(s) in inputs}
    else:
        _stage(body, order, "dt", about=False, store=True)
    rows, parameters = body.loads(every_state=True)
    # (the missing variables are part of the name -- it is the key of the compiled kernel's cache; without any, the name of before)
    # (rows NS - NIN .. NS - 1 are inputs: loaded where used, never stored; a model without any prints as before)
    name = _name("Ode", stem, "\n".join(body.lines) + scheme + "".join(f"|{nm}" for nm in missing))
    return name, (f"// generated by beat.models.from_ode from {system.source.path.name} ({scheme}): {ns_} states, {np_} parameters"
                  + (f", {nin} missing variables ({', '.join(missing)}) as input rows {ns_} .. {ns_ + nin - 1}" if nin else "") + "\n"
                  f"struct {name} {{\n"
                  f"  static constexpr int NS = {ns_ + nin}, NP = {max(np_, 1)}, V_INDEX = {v_index or 0};\n"
                  + (f"  static constexpr int NIN = {nin};\n" if nin else "") +
                  "  static constexpr bool REGISTER_LOOP = true;\n"
                  "  static constexpr int WAVES = 1, WAVES_PER_NODE = 1;\n"
                  "  struct Derived { double unused; };\n"
                  "  template <class P> __host__ __device__ static Derived derive(const P&) { return Derived{0.0}; }\n"
                  "  template <class IO, class P>\n"
                  "  __device__ static __forceinline__ void step(const IO& io, const P& p, const Derived&, const FastMath& fm, double t, double dt) {\n"
                  + _function(body, rows + parameters))


def monitor_struct(system: OdeSystem, names, stem: str, opt: CxxOptions) -> tuple:
    """(struct name, source) of ``Mon_<stem>_<digest>`` for csrc/beat_ode_kernel.h's ode_monitor_kernel: the assignments ``names``
    (at most _hip.MAX_MONITORS) evaluated from the node's states and parameters and stored to output rows 0 .. M-1.  Common
    subexpressions are eliminated over the SELECTION alone; printer, helpers and the order -- a temporary next to its first
    use, an output stored as soon as it is final -- are the step's; only the states and parameters the selection uses are
    loaded."""
    repl, red = sympy.cse([system.assigned[nm] for nm in names], symbols=sympy.numbered_symbols("x_"), optimizations="basic")
    body = _Body(system, repl, opt)
    for j, e in enumerate(red):
        body.lines.append(f"    out.store({j}, {body.pr.doprint(body.expr(e))});  // {names[j]}")
    rows, parameters = body.loads(every_state=False)
    name = _name("Mon", stem, "\n".join(rows + parameters + body.lines))
    return name, (f"// generated by beat.models.from_ode from {system.source.path.name}: {len(names)} monitored values, {len(rows)} of {body.ns + body.nin} "
                  f"{'state and input rows' if body.nin else 'states'} read\n"
                  f"struct {name} {{\n"
                  f"  static constexpr int NS = {body.ns + body.nin}, NP = {max(body.np, 1)}, NM = {len(names)};\n"
                  "  template <class IO, class P, class OUT>\n"
                  "  __device__ static __forceinline__ void eval(const IO& io, const P& p, const FastMath& fm, double t, const OUT& out) {\n"
                  + _function(body, rows + parameters))
