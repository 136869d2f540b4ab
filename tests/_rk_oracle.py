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


def jacobi_cocg(S, b, rtol, atol, max_it, dtype=np.clongdouble):
    """Host restatement of the stage solve of csrc/beat_pde_rk.hip: Jacobi-preconditioned COCG from x0 = 0 on the sparse S
    (complex symmetric; real for a real dtype: plain Jacobi-PCG), in the precision of `dtype`.

    r^T z and p^T q are unconjugated, rr = ||r||^2 is conjugated; tol^2 = max(rtol^2 ||b||^2, atol^2).  Reasons: 2 (rtol
    met), 3 (atol met), -3 (max_it), -5 (p^T q = 0, or r^T z = 0 with r unconverged), checked in zscalar_kernel's order.
    Returns (x, iterations, reason, sqrt(rr), sqrt(bb), history) with history[k] = rr / tol^2 after iteration k + 1."""
    S = S.tocsr().astype(dtype)
    b = np.asarray(b).astype(dtype)
    d = S.diagonal()
    dinv = np.zeros_like(d)
    nz = d != 0
    dinv[nz] = 1 / d[nz]
    x = np.zeros_like(b)
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rz = r @ z
    rr = np.real(np.vdot(r, r))
    bb = rr
    tr = rtol * rtol * bb
    tol2 = max(tr, atol * atol)
    its, reason, hist = 0, 0, []
    if rr <= tol2:
        reason = 2 if rr <= tr else 3
    while reason == 0:
        q = S @ p
        pq = p @ q
        if pq == 0:
            reason = -5
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        rzn = r @ z
        rr = np.real(np.vdot(r, r))
        beta = rzn / rz
        rz = rzn
        its += 1
        hist.append(float(rr / tol2) if tol2 > 0 else np.inf)
        if rr <= tol2:
            reason = 2 if rr <= tr else 3
        elif its >= max_it:
            reason = -3
        elif rzn == 0:
            reason = -5
        else:
            p = z + beta * p
    return x, its, reason, float(np.sqrt(rr)), float(np.sqrt(bb)), hist
