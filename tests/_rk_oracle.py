"""Dense NumPy oracle of one implicit Runge-Kutta step of the P1 monodomain system (tests/test_rk_*.py):

    C_m M k_i + K (v_n + dt sum_j a_ij k_j) = G(t_n + c_i dt),      v_{n+1} = v_n + dt sum_i b_i k_i,

solved as ONE coupled (s N) x (s N) system -- no diagonalisation, no stage ordering."""

import numpy as np


def coupled_step(Mm, K, C_m, A, b, c, dt, v, G, t0):
    """Mm, K dense (N, N); G(t) -> (N,) load; returns v_{n+1}."""
    A, b, c = (np.asarray(a, dtype=np.float64) for a in (A, b, c))
    s, N = b.size, v.size
    S = np.kron(np.eye(s), C_m * Mm) + dt * np.kron(A, K)
    rhs = np.concatenate([G(t0 + c[i] * dt) - K @ v for i in range(s)])
    k = np.linalg.solve(S, rhs).reshape(s, N)
    return v + dt * (b @ k)


def semidiscrete_exact(Mm, K, C_m, v0, f_spatial, T):
    """Exact solution at T of  C_m M v' + K v = f_spatial (cos t + 8 pi^2 sin t)  from v(0) = v0, by the generalised
    eigendecomposition K X = M X diag(mu) (X^T M X = I): each mode solves y' = -(mu/C_m) y + g_i(t)/C_m."""
    import scipy.linalg as sla

    mu, X = sla.eigh(K, Mm)
    y0 = X.T @ Mm @ v0
    g = X.T @ f_spatial  # load coefficient of each mode
    lam = mu / C_m
    # y' = -lam y + (g/C_m)(cos t + w sin t), w = 8 pi^2:  particular solution P cos t + Q sin t
    w = 8 * np.pi**2
    den = lam**2 + 1.0
    gc = g / C_m
    P = gc * (lam - w) / den
    Q = gc * (1.0 + lam * w) / den
    y = (y0 - P) * np.exp(-lam * T) + P * np.cos(T) + Q * np.sin(T)
    return X @ y
