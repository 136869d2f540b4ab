"""``IrksomeMonodomainModel`` -- interface of src/beat/irksome_model.py:15-119.

Solves  C_m dv/dt = div(M grad v) + I_s  on P1 elements with the Runge-Kutta method of a Butcher tableau (``BackwardEuler()``,
``GaussLegendre(s)``, ``RadauIIA(s)``, ... from beat.butcher, or ``irksome``'s through the compat shim).  The reference hands
the stage-derivative form to Irksome and PETSc; here the PDE's linearity is used instead: a lower-triangular ``A`` is solved
stage by stage, any other ``A`` is diagonalised on the host (beat.butcher.rk_plan) and every eigenvalue leaves one shifted
solve on the device -- real for a real eigenvalue, complex (COCG, csrc/beat_pde_rk.hip) for a conjugate pair.

Constant conductivity tensors on an undivided box only: decomposed grids and per-node operators (per-cell tensors, voxel
masks) raise ``NotImplementedError``."""

from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from . import _hip, grid
from ._engine import KspResult, conductivity_array
from .base_model import BaseModel, Results, Status
from .butcher import rk_plan
from .monodomain_model import MonodomainModel

logger = logging.getLogger(__name__)


class _RkOps:
    """The constant-coefficient operator handle of the stage solves and the device fields they use."""

    def __init__(self, ctx, shape, mass_tab, stiff_tab):
        self.ctx, self.lib = ctx, ctx.lib
        nx, ny, nz = (int(v) for v in shape)
        self.n, self.plane = nx * ny * nz, nx * ny
        mt = np.ascontiguousarray(mass_tab, dtype=np.float64)
        kt = np.ascontiguousarray(stiff_tab, dtype=np.float64)
        handle = C.c_void_p()
        _hip.check(self.lib.beat_pde_create(ctx.handle, (C.c_int64 * 3)(nx, ny, nz), 1, 1, mt.ctypes.data_as(C.c_void_p),
                                            kt.ctypes.data_as(C.c_void_p), C.byref(handle)))
        self.handle = handle
        self.work = ctx.zeros(int(self.lib.beat_pde_zwork_doubles(handle)))
        self._fields = {}

    def field(self, key):
        f = self._fields.get(key)
        if f is None:
            f = self._fields[key] = self.ctx.field(self.n, self.plane)
        return f

    def rhs(self, w, gamma, y, s, r_re, r_im=None):
        """r = sum_m gamma_m w_m - K sum_j s_j y_j (gamma, s complex when r_im is given)."""
        nw, ny = len(w), len(y)
        if nw > _hip.MAX_STIM or ny > _hip.MAX_STIM:
            raise NotImplementedError(f"a stage right-hand side of {nw} load fields and {ny} stiffness terms (at most "
                                      f"{_hip.MAX_STIM} each)")
        wp = (C.c_void_p * max(1, nw))(*[f.ptr for f in w])
        yp = (C.c_void_p * max(1, ny))(*[f.ptr for f in y])
        g = np.asarray(gamma, dtype=np.complex128).reshape(-1)
        sv = np.asarray(s, dtype=np.complex128).reshape(-1)
        dbl = lambda a: (C.c_double * max(1, len(a)))(*[float(x) for x in a])  # noqa: E731
        _hip.check(self.lib.beat_pde_rk_rhs(self.handle, wp, dbl(g.real), dbl(g.imag), nw, yp, dbl(sv.real), dbl(sv.imag), ny,
                                            r_re.ptr, None if r_im is None else r_im.ptr))

    def solve(self, a, shift, rhs_re, rhs_im, x_re, x_im, rtol, atol, max_it) -> KspResult:
        """(a Mass + shift K) x = rhs; complex when x_im is given."""
        info = _hip.KspInfo()
        _hip.check(self.lib.beat_pde_zsolve(self.handle, float(a), float(np.real(shift)), float(np.imag(shift)), rhs_re.ptr,
                                            None if rhs_im is None else rhs_im.ptr, x_re.ptr, None if x_im is None else x_im.ptr,
                                            C.c_void_p(self.work.data_ptr()), float(rtol), float(atol), int(max_it), C.byref(info)),
                   allow_not_converged=True)
        return KspResult(info.iterations, info.residual_norm, info.converged_reason, info.rhs_norm)

    def update(self, v, u_re, u_im, d):
        """v += sum_i Re(d_i u_i)."""
        k = len(u_re)
        ure = (C.c_void_p * max(1, k))(*[f.ptr for f in u_re])
        uim = (C.c_void_p * max(1, k))(*[None if f is None else f.ptr for f in u_im])
        d = np.asarray(d, dtype=np.complex128)
        dre = (C.c_double * max(1, k))(*d.real)
        dim = (C.c_double * max(1, k))(*d.imag)
        _hip.check(self.lib.beat_pde_rk_update(self.handle, v.ptr, ure, uim, dre, dim, k))

    def __del__(self):  # pragma: no cover
        try:
            self.lib.beat_pde_destroy(self.handle)
        except Exception:
            pass


class IrksomeMonodomainModel(BaseModel):
    r"""Solve the monodomain model with a Runge-Kutta method given by its Butcher tableau (src/beat/irksome_model.py:15).

    Not a ``MonodomainModel``: the split step's fused routes (MonodomainSplittingSolver) are built around the theta-rule
    operator and do not apply; the literal sequence (ode step, pde step) does."""

    def __init__(self, time, mesh, M, butcher_tableau, I_s=None, params=None, C_m: float = 1.0, dx=None, **kwargs):
        self._M = M
        self.C_m = grid.Constant(mesh, C_m)
        self.butcher_tableau = butcher_tableau
        self._plan = rk_plan(butcher_tableau)  # ValueError for a tableau that cannot be diagonalised stably
        super().__init__(mesh=mesh, time=time, params=params, I_s=I_s, dx=dx, **kwargs)

    @staticmethod
    def default_parameters():
        return MonodomainModel.default_parameters()

    def _setup_state_space(self) -> None:
        k = self.parameters["degree"]
        family = self.parameters["family"]
        self.V = grid.FunctionSpace(self._mesh, family, k)
        self._state = grid.Function(self.V, name="v")

    def _setup_operators(self) -> None:
        from . import _stencil

        mesh = self._mesh
        if mesh.slab.world > 1:
            raise NotImplementedError("IrksomeMonodomainModel runs on an undivided grid (one rank)")
        M = conductivity_array(self._M, mesh)
        if M.ndim != 2 or mesh.active is not None:
            raise NotImplementedError("IrksomeMonodomainModel needs a constant conductivity tensor on an unmasked box "
                                      "(per-cell tensors and voxel masks use per-node operators)")
        mass_tab, stiff_tab = _stencil.stencil_tables(mesh.dim, mesh.h, M)
        self._ops = _RkOps(self._ctx, mesh.shape_local, mass_tab, stiff_tab)

    def _update_matrices(self):
        pass  # the stage operators are formed per solve from C_m, dt and the tableau

    def _solve_linear(self, stim_w, stim_amp) -> None:  # the theta-rule's single solve: not used here
        raise NotImplementedError

    @property
    def state(self) -> grid.Function:
        return self._state

    def assign_previous(self):
        # as the reference's: the stepper updates the state within step(), nothing to copy
        pass

    # -- one step ----------------------------------------------------------------------------------------------------------
    def _loads(self, t0: float, dt: float, stage: int):
        """(fields, amplitudes) of the load G at the stage time t0 + c_stage dt; a stimulus whose weights are re-integrated
        at every time keeps the stage's copy in a field of its own."""
        self.time.value = t0 + float(self._plan.c[stage]) * dt
        w, amp = [], []
        for k, s in enumerate(self._stimuli):
            a = s.amplitude()
            if a == 0.0 or s.field is None:
                continue
            f = s.field
            if s.general is not None:
                f = self._ops.field(("load", stage, k))
                f.copy_from(s.field)
            w.append(f)
            amp.append(a)
        return w, amp

    def _step_lower(self, v, t0, dt, tol):
        plan, ops, C_m = self._plan, self._ops, float(self.C_m)
        s = plan.b.size
        ks, recs = [], []
        for i in range(s):
            w, amp = self._loads(t0, dt, i)
            y, coef = [v], [1.0]
            for j in range(i):
                if plan.A[i, j] != 0.0:
                    y.append(ks[j])
                    coef.append(dt * plan.A[i, j])
            r = ops.field("r_re")
            ops.rhs(w, amp, y, coef, r)
            k = ops.field(("k", i))
            recs.append(ops.solve(C_m, plan.A[i, i] * dt, r, None, k, None, *tol))
            ks.append(k)
        self.time.value = t0
        use = [i for i in range(s) if plan.b[i] != 0.0]
        ops.update(v, [ks[i] for i in use], [None] * len(use), [dt * plan.b[i] for i in use])
        return recs

    def _step_diag(self, v, t0, dt, tol):
        plan, ops, C_m = self._plan, self._ops, float(self.C_m)
        s = plan.b.size
        loads = [self._loads(t0, dt, j) for j in range(s)]
        self.time.value = t0
        rowsum = plan.rowsum
        recs, u_re, u_im, d = [], [], [], []
        for i in range(plan.n_real + plan.n_pairs):
            cplx = i >= plan.n_real
            row = plan.Tinv[i] if cplx else plan.Tinv[i].real
            w, gamma = [], []
            for j, (wj, aj) in enumerate(loads):
                for f, a in zip(wj, aj):
                    w.append(f)
                    gamma.append(row[j] * a)
            w, gamma = _merge(w, gamma)
            sv = rowsum[i] if cplx else rowsum[i].real
            r_re, r_im = ops.field("r_re"), (ops.field("r_im") if cplx else None)
            ops.rhs(w, gamma, [v], [sv], r_re, r_im)
            x_re, x_im = ops.field(("u_re", i)), (ops.field(("u_im", i)) if cplx else None)
            lam = plan.lam[i] if cplx else plan.lam[i].real
            recs.append(ops.solve(C_m, lam * dt, r_re, r_im, x_re, x_im, *tol))
            u_re.append(x_re)
            u_im.append(x_im)
            d.append(2.0 * dt * plan.d[i] if cplx else dt * plan.d[i].real)
        ops.update(v, u_re, u_im, d)
        return recs

    def step(self, interval):
        t0, t1 = interval
        dt = t1 - t0
        with self.monitor.track_time("pde_total_step"):
            self.time.value = t0
            self._timestep.value = dt
            tol = self._solver_tolerances()
            v = self._state.writable_field(overwrite_all=False)
            with self.monitor.track_time("pde_linear_solve"):
                if self._plan.kind == "lower":
                    recs = self._step_lower(v, t0, dt, tol)
                else:
                    recs = self._step_diag(v, t0, dt, tol)
            self._state._touch()
            self.ksp = _combine(recs)
            self.monitor.record_ksp(self.ksp)
            self._check_converged()
        # Advance the time as the reference does after the stepper's advance()
        self.time.value = t0 + dt
        self.monitor.advance_step(t0, t1)

    def solve(self, interval, dt=None) -> Results:
        """The reference's loop (irksome_model.py:105-119)."""
        T0, T = interval
        if dt is None:
            dt = T - T0
        t0 = T0
        t1 = T0 + dt
        self.status = Status.OK
        while t1 < T + 1e-12:
            self.step((t0, t1))
            t0 = t1
            t1 = t0 + dt
        return Results(state=self.state, status=self.status)


def _merge(w, gamma):
    """One coefficient per distinct field (the same weight field at several stage times)."""
    out_w, out_g = [], []
    for f, g in zip(w, gamma):
        for k, h in enumerate(out_w):
            if h is f:
                out_g[k] += g
                break
        else:
            out_w.append(f)
            out_g.append(complex(g))
    return out_w, out_g


def _combine(recs) -> KspResult:
    """One KSP-like record per step: the iterations of all stage solves, the worst residual, a failure if any failed."""
    if not recs:
        return KspResult()
    bad = [r for r in recs if r.converged_reason < 0]
    worst = max(recs, key=lambda r: r.residual_norm)
    return KspResult(iterations=sum(r.iterations for r in recs), residual_norm=worst.residual_norm,
                     converged_reason=(bad[0] if bad else recs[-1]).converged_reason,
                     rhs_norm=max(r.rhs_norm for r in recs))
