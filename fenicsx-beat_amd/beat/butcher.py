"""Butcher tableaux and the host side of an implicit Runge-Kutta step of the monodomain PDE (beat.irksome_model).

The tableau classes are duck-typed like Irksome's (``A``, ``b``, ``c``, ``num_stages``, ``order``), so a script written for
the reference passes them where it passed ``irksome.RadauIIA(2)``.  The collocation families are built from their nodes
(any ``s`` up to 5), not from stored tables.

``rk_plan`` turns a tableau into what the device step needs.  The stage system of the linear PDE
``C_m M k_i + K (v_n + dt sum_j a_ij k_j) = G(t_i)`` is either

* solved stage by stage when ``A`` is lower triangular (one real solve with ``C_m M + a_ii dt K`` each), or
* diagonalised, ``A = T diag(lam) T^-1``: the transformed stages ``u = (T^-1 (x) I) k`` decouple into
  ``(C_m M + lam_i dt K) u_i = sum_j (T^-1)_ij G(t_j) - (sum_j (T^-1)_ij) K v_n``, one real solve per real eigenvalue and one
  complex solve per conjugate pair, and ``v_{n+1} = v_n + dt sum_i d_i u_i`` with ``d = b^T T``.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from numpy.polynomial import legendre as _leg
from numpy.polynomial import polynomial as _poly

__all__ = ["ButcherTableau", "BackwardEuler", "GaussLegendre", "RadauIIA", "LobattoIIIA", "LobattoIIIC", "Alexander",
           "RKPlan", "rk_plan"]

MAX_COLLOCATION_STAGES = 5
COND_LIMIT = 1e8


class ButcherTableau:
    """A Runge-Kutta method: ``A`` (s, s), ``b`` (s,), ``c`` (s,) and its classical ``order``."""

    def __init__(self, A, b, c, order: int, name: str = "ButcherTableau"):
        self.A = np.array(A, dtype=np.float64)
        self.b = np.array(b, dtype=np.float64)
        self.c = np.array(c, dtype=np.float64)
        self.order = int(order)
        self.name = name
        s = self.b.size
        if self.A.shape != (s, s) or self.c.shape != (s,):
            raise ValueError(f"inconsistent tableau: A {self.A.shape}, b {self.b.shape}, c {self.c.shape}")

    @property
    def num_stages(self) -> int:
        return self.b.size

    @property
    def is_explicit(self) -> bool:
        return bool(np.all(np.triu(self.A) == 0.0))

    @property
    def is_diagonally_implicit(self) -> bool:
        return bool(np.all(np.triu(self.A, 1) == 0.0))

    @property
    def is_stiffly_accurate(self) -> bool:
        return bool(np.allclose(self.A[-1], self.b, rtol=0.0, atol=1e-15))

    def __repr__(self) -> str:
        return self.name


def _compose_2x_minus_1(leg_coef) -> np.ndarray:
    p = _leg.leg2poly(leg_coef)  # power series in y
    out = np.zeros(1)
    lin = np.array([-1.0, 2.0])  # y = 2x - 1
    powk = np.array([1.0])
    for ck in p:
        out = _poly.polyadd(out, ck * powk)
        powk = _poly.polymul(powk, lin)
    return out


def _real_roots(coef) -> np.ndarray:
    r = _poly.polyroots(coef)
    return np.sort(r.real)


def _collocation(c: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """A_ij = int_0^{c_i} l_j, b_j = int_0^1 l_j for the Lagrange basis l_j on the nodes c (exact up to rounding: the
    moment system V^T x = 1/k is solved in float64 with the nodes well separated)."""
    s = c.size
    V = np.vander(c, s, increasing=True)  # V[i, k] = c_i^k
    # sum_j l_j(t) c_j^k = t^k  =>  A V = C with C[i, k] = c_i^(k+1) / (k+1); b V = 1 / (k+1)
    k = np.arange(1, s + 1)
    Cm = c[:, None] ** k[None, :] / k[None, :]
    A = np.linalg.solve(V.T, Cm.T).T
    b = np.linalg.solve(V.T, 1.0 / k)
    return A, b


def _check_stages(s: int, lo: int = 1) -> int:
    s = int(s)
    if not lo <= s <= MAX_COLLOCATION_STAGES:
        raise ValueError(f"number of stages must be in {lo}..{MAX_COLLOCATION_STAGES}, got {s}")
    return s


def GaussLegendre(num_stages: int) -> ButcherTableau:
    """Gauss-Legendre collocation: nodes = zeros of P_s(2x - 1); order 2s."""
    s = _check_stages(num_stages)
    c = _real_roots(_compose_2x_minus_1(np.eye(s + 1)[s]))
    A, b = _collocation(c)
    return ButcherTableau(A, b, c, 2 * s, f"GaussLegendre({s})")


def RadauIIA(num_stages: int) -> ButcherTableau:
    """Radau IIA collocation: nodes = zeros of P_s(2x - 1) - P_{s-1}(2x - 1) (right end point included); order 2s - 1."""
    s = _check_stages(num_stages)
    e = np.zeros(s + 1)
    e[s], e[s - 1] = 1.0, -1.0
    c = _real_roots(_compose_2x_minus_1(e))
    c[-1] = 1.0
    A, b = _collocation(c)
    return ButcherTableau(A, b, c, 2 * s - 1, f"RadauIIA({s})")


def _lobatto_nodes(s: int) -> np.ndarray:
    inner = np.array([])
    if s > 2:
        d = _poly.polyder(_compose_2x_minus_1(np.eye(s)[s - 1]))  # zeros of P'_{s-1}(2x - 1)
        inner = _real_roots(d)
    return np.concatenate([[0.0], inner, [1.0]])


def LobattoIIIA(num_stages: int) -> ButcherTableau:
    """Lobatto IIIA collocation (both end points); order 2s - 2.  LobattoIIIA(2) is the trapezoidal rule."""
    s = _check_stages(num_stages, lo=2)
    c = _lobatto_nodes(s)
    A, b = _collocation(c)
    A[0] = 0.0  # the first row is exactly zero (explicit first stage)
    return ButcherTableau(A, b, c, 2 * s - 2, f"LobattoIIIA({s})")


def LobattoIIIC(num_stages: int) -> ButcherTableau:
    """Lobatto IIIC: Lobatto nodes and weights, a_i1 = b_1 and the simplifying condition C(s-1) for the other columns;
    order 2s - 2, L-stable."""
    s = _check_stages(num_stages, lo=2)
    c = _lobatto_nodes(s)
    _, b = _collocation(c)
    A = np.zeros((s, s))
    A[:, 0] = b[0]
    # sum_{j>=2} a_ij c_j^(k-1) = c_i^k / k - b_1 0^(k-1),  k = 1..s-1
    k = np.arange(1, s)
    V = c[1:][None, :] ** (k[:, None] - 1)  # (s-1) x (s-1)
    for i in range(s):
        rhs = c[i] ** k / k - b[0] * (k == 1)
        A[i, 1:] = np.linalg.solve(V, rhs)
    return ButcherTableau(A, b, c, 2 * s - 2, f"LobattoIIIC({s})")


def BackwardEuler() -> ButcherTableau:
    return ButcherTableau([[1.0]], [1.0], [1.0], 1, "BackwardEuler()")


def Alexander() -> ButcherTableau:
    """Alexander's (1977) three-stage, third-order, L-stable SDIRK method."""
    # gamma: the root of x^3 - 3 x^2 + 3/2 x - 1/6 in (1/6, 1/2)
    r = _poly.polyroots([-1.0 / 6.0, 1.5, -3.0, 1.0])
    gamma = float([x.real for x in r if abs(x.imag) < 1e-12 and 1.0 / 6.0 < x.real < 0.5][0])
    tau2 = 0.5 * (1.0 + gamma)
    b1 = -0.25 * (6.0 * gamma**2 - 16.0 * gamma + 1.0)
    b2 = 0.25 * (6.0 * gamma**2 - 20.0 * gamma + 5.0)
    A = [[gamma, 0.0, 0.0], [tau2 - gamma, gamma, 0.0], [b1, b2, gamma]]
    return ButcherTableau(A, [b1, b2, gamma], [gamma, tau2, 1.0], 3, "Alexander()")


# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class RKPlan:
    """What the device step of a tableau does.

    kind "lower": stages in order; stage i solves (C_m M + A[i, i] dt K) k_i = G(t_i) - K (v_n + dt sum_{j<i} A[i, j] k_j),
    then v += dt sum_i b_i k_i.
    kind "diag": ``lam`` eigenvalues in the order [real ones..., one of each conjugate pair (positive imaginary part)...],
    ``T`` / ``Tinv`` the full (s, s) eigenvector matrix and its inverse, columns ordered [reals, pair members, partners];
    ``n_real`` real eigenvalues come first, then ``n_pairs`` pairs; ``d = b^T T`` (complex, length s).  Solve i of the
    ``n_real + n_pairs`` distinct ones: (C_m M + lam_i dt K) u_i = sum_j Tinv[i, j] G(t_j) - rowsum(Tinv)[i] K v_n;
    v += dt (sum_real d_i u_i + sum_pairs 2 Re(d_p u_p))."""

    kind: str
    A: np.ndarray
    b: np.ndarray
    c: np.ndarray
    lam: np.ndarray | None = None
    T: np.ndarray | None = None
    Tinv: np.ndarray | None = None
    d: np.ndarray | None = None
    n_real: int = 0
    n_pairs: int = 0
    cond: float = 1.0

    @property
    def num_solves(self) -> int:
        return self.A.shape[0] if self.kind == "lower" else self.n_real + self.n_pairs

    @property
    def rowsum(self) -> np.ndarray:
        return self.Tinv.sum(axis=1)


def rk_plan(tableau) -> RKPlan:
    """Host transform of a tableau (anything with ``A``, ``b``, ``c``).  Raises ``ValueError`` for an ``A`` that cannot be
    diagonalised stably (defective or cond(T) > 1e8) or whose shifted operators would not be definite (an eigenvalue with a
    negative real part)."""
    A = np.array(tableau.A, dtype=np.float64)
    b = np.array(tableau.b, dtype=np.float64).ravel()
    c = np.array(tableau.c, dtype=np.float64).ravel()
    s = b.size
    if A.shape != (s, s) or c.size != s:
        raise ValueError(f"inconsistent tableau: A {A.shape}, b {b.shape}, c {c.shape}")
    if not np.all(np.isfinite(A)) or not np.all(np.isfinite(b)) or not np.all(np.isfinite(c)):
        raise ValueError("tableau has non-finite entries")
    if np.all(np.triu(A, 1) == 0.0):
        if np.any(np.diag(A) < 0.0):
            raise ValueError("a negative diagonal entry of A gives an indefinite stage operator")
        return RKPlan("lower", A, b, c)
    w, V = np.linalg.eig(A)
    scale = max(1.0, float(np.abs(A).max()))
    tol = 1e-10 * scale
    real_idx = [i for i in range(s) if abs(w[i].imag) <= tol]
    pos_idx = [i for i in range(s) if w[i].imag > tol]
    neg_idx = [i for i in range(s) if w[i].imag < -tol]
    if len(pos_idx) != len(neg_idx):
        raise ValueError("eigenvalues of A do not come in conjugate pairs")
    cols, lams = [], []
    for i in real_idx:
        v = V[:, i]
        k = int(np.argmax(np.abs(v)))
        v = (v / v[k]).real  # the eigenvector of a real eigenvalue of a real matrix, made real
        cols.append(v / np.linalg.norm(v))
        lams.append(complex(w[i].real, 0.0))
    for i in pos_idx:
        cols.append(V[:, i])
        lams.append(w[i])
    for i in pos_idx:
        cols.append(np.conj(V[:, i]))
        lams.append(np.conj(w[i]))
    T = np.array(cols, dtype=np.complex128).T
    lam = np.array(lams, dtype=np.complex128)
    cond = float(np.linalg.cond(T))
    if not np.isfinite(cond) or cond > COND_LIMIT:
        raise ValueError(f"the Butcher matrix cannot be diagonalised stably (cond(T) = {cond:.3g} > {COND_LIMIT:g}: "
                         "defective or nearly so)")
    if np.linalg.norm(T @ np.diag(lam) - A @ T) > 1e-10 * scale * np.linalg.norm(T):
        raise ValueError("the Butcher matrix is defective")
    if np.any(lam.real < -tol) or np.any((np.abs(lam.imag) > tol) & (lam.real <= tol)):
        raise ValueError("an eigenvalue of A with a non-positive real part gives an indefinite stage operator")
    Tinv = np.linalg.inv(T)
    d = b @ T
    nr, npair = len(real_idx), len(pos_idx)
    return RKPlan("diag", A, b, c, lam=lam, T=T, Tinv=Tinv, d=d, n_real=nr, n_pairs=npair, cond=cond)
