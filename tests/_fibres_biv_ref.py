"""NumPy restatement of the bi-ventricular fibre rule (include/beat_hip.h: beat_fibres_biv_rule), written from the rule's text and not
from csrc/beat_fibres_kernel.h, and the inputs the CPU and the GPU tests share (test_fibres_biv_cpu.py, test_fibres_biv_gpu.py).

Frames are 3 x 3 matrices [f | n | s] here, and ``bislerp`` takes and returns matrices: each blend goes matrix -> quaternion -> matrix,
where the header keeps quaternions from the first frame to the last.  Voxels, nodes and corners are numbered as in _fibres_ref.py,
whose grids, spacings, conductivities, axis, mask and gradient this file uses."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from _fibres_ref import AXIS, GRIDS, H, S_L, S_T, corners, gradient, mask  # noqa: F401  (the tests read them from here)

ANGLES = (40.0, -50.0, 20.0, -20.0)  # alpha_endo, alpha_epi, beta_endo, beta_epi in degrees
REGIONS = ("lv wall", "septum", "rv wall")
RMIN, GAP_MIN = 0.5, 0.01  # the conditions under which TOL holds (assert_conditions)

# TOL, per component of f, s, n, header and device against this file.  Errors counted as small rotations of a frame, u = 1.1e-16:
#   one frame     ~40 rounded operations and four sin / cos of a few ulp each, amplified at most 1 / |r|^2 <= 4 by the two
#                 normalisations: <~ 4 * 60 u = 3e-14 (the bound _fibres_ref.py rounds up to 1e-13)
#   to quaternion Shepperd's divisor is >= 2, so a component of q moves by at most the matrix entries' error; ~10 operations: + 1e-15
#   one blend     c >= 1/2, so theta <= pi / 3 and sin(t theta) / sigma <= theta / sin(theta) <= 1.21: the result moves by at most
#                 1.21 (error of q_a + error of q_b), plus ~40 operations and one atan2, sin and cos on numbers <= 1.05: + 1e-14.
#                 (The candidate is the same on both sides because its |<q_c, q_b>| leads the next by >= GAP_MIN >> 1e-13.)
#   to matrix     entries are 2 (products of two components), sum |q_i| <= 2: a component error e gives at most 4 e
# Q_endo: 1.21 (3e-14 + 3e-14 + 2e-15) + 1e-14 = 9e-14.  Q: 1.21 (9e-14 + 3e-14 + 1e-15) + 1e-14 = 1.6e-13.  As a matrix: 6.3e-13.
# This file turns Q_endo into a matrix and back in between, which is within the same bound (4 e out, e / 2 * 2 back in: the divisor).
# So 1e-12, the single-ventricle rule's bound, holds here too.
TOL = 1e-12


def frame(l, t, alpha, beta):
    """Step 1: ([f | n | s], |r|), or (None, |r| or NaN) where the frame is undefined."""
    nl, nt = np.linalg.norm(l), np.linalg.norm(t)
    if not nl > 0.0 or not nt > 0.0:
        return None, np.nan
    e_l = l / nl
    r = t / nt - np.dot(e_l, t / nt) * e_l
    nr = np.linalg.norm(r)
    if not nr > 1e-12:
        return None, nr
    e_t = r / nr
    e_c = np.cross(e_l, e_t)
    f = np.cos(alpha) * e_c + np.sin(alpha) * e_l
    g = -np.sin(alpha) * e_c + np.cos(alpha) * e_l
    s = np.sin(beta) * g + np.cos(beta) * e_t
    n = np.cos(beta) * g - np.sin(beta) * e_t
    return np.stack([f, n, s], axis=1), nr


def to_quaternion(R):
    """Step 2, Shepperd: (w, x, y, z) of the rotation matrix R."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    which = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
    if which == 0:
        S = 2.0 * np.sqrt(1.0 + tr)
        q = [0.25 * S, (R[2, 1] - R[1, 2]) / S, (R[0, 2] - R[2, 0]) / S, (R[1, 0] - R[0, 1]) / S]
    elif which == 1:
        S = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / S, 0.25 * S, (R[0, 1] + R[1, 0]) / S, (R[0, 2] + R[2, 0]) / S]
    elif which == 2:
        S = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / S, (R[0, 1] + R[1, 0]) / S, 0.25 * S, (R[1, 2] + R[2, 1]) / S]
    else:
        S = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / S, (R[0, 2] + R[2, 0]) / S, (R[1, 2] + R[2, 1]) / S, 0.25 * S]
    return np.array(q)


def to_matrix(q):
    """The rotation matrix of the quaternion q, normalised first."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def multiply(p, q):
    """The Hamilton product p (x) q."""
    pw, px, py, pz = p
    qw, qx, qy, qz = q
    return np.array([pw * qw - px * qx - py * qy - pz * qz, pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw])


UNITS = (np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0]))


def bislerp(Qa, Qb, t):
    """Step 3 on matrices: (the blended frame, the index of the chosen candidate, best |<q_c, q_b>| minus the second best)."""
    qa, qb = to_quaternion(Qa), to_quaternion(Qb)
    cands = [multiply(qa, u) for u in UNITS]
    dots = np.array([np.dot(qc, qb) for qc in cands])
    k = int(np.argmax(np.abs(dots)))  # (argmax returns the first of equal maxima)
    ranked = np.sort(np.abs(dots))
    qc = cands[k] if dots[k] >= 0.0 else -cands[k]
    c = np.dot(qc, qb)
    w = qb - c * qc
    sigma = np.linalg.norm(w)
    if sigma > 0.0:
        theta = np.arctan2(sigma, c)
        qc = np.cos(t * theta) * qc + np.sin(t * theta) * w / sigma
    return to_matrix(qc), k, ranked[3] - ranked[2]


def rule(cells, h, phi_lv, phi_rv, phi_epi, longitudinal, angles_deg=ANGLES, active=None, s_l=S_L, s_t=S_T):
    """Step 4 on every voxel.  ``longitudinal``: nodal values of psi, or a 3-vector.  Returns f, s, n (nvoxels, 3), M (nvoxels, 3, 3), the
    bool mask and the number of the degenerate voxels, and per voxel the record the tolerance's conditions are read from: ``r``
    (nvoxels, 3) = |r| of Q_lv, Q_rv, Q_epi (NaN: not formed), ``candidate`` (nvoxels, 2) = the candidate the endocardial and the
    endo -> epi blend chose (-1: no blend), ``gap`` (nvoxels, 2) = how far its |<q_c, q_b>| leads the second best (NaN: no blend)."""
    nvox = int(np.prod(cells))
    act = np.ones(nvox, dtype=bool) if active is None else np.asarray(active, dtype=bool).ravel()
    c_lv, c_rv, c_epi = (corners(p, cells) for p in (phi_lv, phi_rv, phi_epi))
    g_lv, g_rv, g_epi = (gradient(c, h) for c in (c_lv, c_rv, c_epi))
    longitudinal = np.asarray(longitudinal, dtype=np.float64)
    g_psi = np.tile(longitudinal, (nvox, 1)) if longitudinal.shape == (3,) else gradient(corners(longitudinal, cells), h)
    m_lv, m_rv, m_epi = (np.clip(c.reshape(8, -1).mean(axis=0), 0.0, 1.0) for c in (c_lv, c_rv, c_epi))
    a_endo, a_epi, b_endo, b_epi = np.deg2rad(np.asarray(angles_deg, dtype=np.float64))
    f, s, n = np.zeros((nvox, 3)), np.zeros((nvox, 3)), np.zeros((nvox, 3))
    rnorm = np.full((nvox, 3), np.nan)
    candidate = np.full((nvox, 2), -1)
    gap = np.full((nvox, 2), np.nan)
    degenerate = np.zeros(nvox, dtype=bool)
    for v in np.nonzero(act)[0]:
        total = m_lv[v] + m_rv[v]
        d = m_rv[v] / total if total != 0.0 else 0.0
        alpha_s, beta_s = a_endo * (1.0 - 2.0 * d), b_endo * (1.0 - 2.0 * d)
        alpha_w = a_endo * (1.0 - m_epi[v]) + a_epi * m_epi[v]
        beta_w = b_endo * (1.0 - m_epi[v]) + b_epi * m_epi[v]
        Q_lv, rnorm[v, 0] = frame(g_psi[v], -g_lv[v], alpha_s, beta_s)
        Q_rv, rnorm[v, 1] = frame(g_psi[v], g_rv[v], alpha_s, beta_s)
        Q_epi, rnorm[v, 2] = frame(g_psi[v], g_epi[v], alpha_w, beta_w)
        if Q_lv is not None and Q_rv is not None:
            Q_endo, candidate[v, 0], gap[v, 0] = bislerp(Q_lv, Q_rv, d)
        else:
            Q_endo = Q_lv if Q_lv is not None else Q_rv
        if Q_endo is not None and Q_epi is not None:
            Q, candidate[v, 1], gap[v, 1] = bislerp(Q_endo, Q_epi, m_epi[v])
        else:
            Q = Q_endo if Q_endo is not None else Q_epi
        if Q is None:
            degenerate[v] = True
            continue
        f[v], n[v], s[v] = Q[:, 0], Q[:, 1], Q[:, 2]
    M = s_t * np.eye(3)[None] + (s_l - s_t) * np.einsum("vi,vj->vij", f, f)
    M[~act] = 0.0
    return SimpleNamespace(f=f, s=s, n=n, M=M, degenerate=degenerate, count=int(degenerate.sum()), r=rnorm, candidate=candidate, gap=gap,
                           active=act)


def ramp(cells, direction, rng):
    """A nodal field that rises from 0 to 1 across the box along the unit vector ``direction``, plus 10 % seeded noise: the node's
    position along it plus 0.1 min(H) u, u uniform in [0, 1), over the box's extent along it."""
    cx, cy, cz = cells
    shape = (cz + 1, cy + 1, cx + 1)
    iz, iy, ix = np.meshgrid(*(np.arange(m, dtype=np.float64) for m in shape), indexing="ij")
    k = np.asarray(direction, dtype=np.float64)
    along = k[0] * H[0] * ix + k[1] * H[1] * iy + k[2] * H[2] * iz
    noise = 0.1 * min(H)
    return ((along - along.min() + noise * rng.random(shape)) / (along.max() - along.min() + noise)).ravel()


def _turned(degrees):
    """The unit vector in the (x, y) plane at this angle to x: about the long axis, which is z or near it."""
    a = np.deg2rad(degrees)
    return np.array([np.cos(a), np.sin(a), 0.0])


def fields(cells, region, rng):
    """phi_lv, phi_rv, phi_epi of one region; x is the transmural direction, the wall's endocardium is at x = 0.
    lv wall: phi_lv falls and phi_epi rises along x; phi_rv is small, its gradient 30 degrees from -grad phi_lv.
    septum:  phi_lv falls and phi_rv rises along x (10 degrees apart); phi_epi is small, its gradient 60 degrees from x.
    rv wall: phi_rv falls and phi_epi rises along x; phi_lv is small and falls along a direction 30 degrees from x (the LV lies
             behind the RV cavity), so -grad phi_lv is 150 degrees from grad phi_rv about the long axis: not the 90 of an exact tie."""
    x = _turned(0.0)
    if region == "lv wall":
        return 1.0 - 0.8 * ramp(cells, x, rng), 0.1 * ramp(cells, _turned(30.0), rng), 0.8 * ramp(cells, x, rng)
    if region == "septum":
        return 0.9 - 0.8 * ramp(cells, x, rng), 0.1 + 0.8 * ramp(cells, _turned(10.0), rng), 0.1 * ramp(cells, _turned(60.0), rng)
    if region == "rv wall":
        return 0.1 * (1.0 - ramp(cells, _turned(30.0), rng)), 1.0 - 0.8 * ramp(cells, x, rng), 0.8 * ramp(cells, x, rng)
    raise ValueError(region)


@lru_cache(maxsize=None)
def case(cells, psi_as_field, masked, region):
    """Inputs and reference of one case, computed once and read-only."""
    cx, cy, cz = cells
    rng = np.random.default_rng(4321 + cx + 7 * cy + 31 * cz + 101 * REGIONS.index(region))
    phi_lv, phi_rv, phi_epi = fields(cells, region, rng)
    psi = ramp(cells, (0.0, 0.0, 1.0), rng)
    active = mask(cells) if masked else None
    ref = rule(cells, H, phi_lv, phi_rv, phi_epi, psi if psi_as_field else np.array(AXIS), ANGLES, active)
    for a in (phi_lv, phi_rv, phi_epi, psi, ref.f, ref.s, ref.n, ref.M):
        a.setflags(write=False)
    return SimpleNamespace(cells=cells, h=H, phi_lv=phi_lv, phi_rv=phi_rv, phi_epi=phi_epi, psi=psi if psi_as_field else None,
                           axis=None if psi_as_field else np.array(AXIS), active=active, region=region, ref=ref)


CASES = [(cells, psi_as_field, masked, region) for cells in GRIDS for psi_as_field in (True, False) for masked in (False, True)
         for region in REGIONS]


def assert_conditions(ref):
    """What TOL rests on, asserted before anything is compared: no degenerate voxel, all three frames formed with |r| >= 0.5, and
    both blends' candidates chosen by a margin of at least 0.01 (so that every implementation takes the same branch)."""
    assert ref.count == 0
    r, gap = ref.r[ref.active], ref.gap[ref.active]
    assert np.isfinite(r).all() and r.min() >= RMIN, r.min()
    assert np.isfinite(gap).all() and gap.min() >= GAP_MIN, gap.min()


def slab(cells=(8, 4, 4), L=(2.0, 1.0, 1.0)):
    """The box of the closed forms: cells, spacings, lengths and the nodal x and z."""
    cx, cy, cz = cells
    h = tuple(l / c for l, c in zip(L, cells))
    x = np.tile(np.arange(cx + 1) * h[0], (cz + 1) * (cy + 1))
    z = np.repeat(np.arange(cz + 1) * h[2], (cy + 1) * (cx + 1))
    return cells, h, L, x, z


def closed_form(region, angles_deg, cells=(8, 4, 4)):
    """The three closed forms with exactly linear fields on the slab, e_l = z: the nodal fields as functions of X = x / L, and per
    voxel the angle of the fibre in the (y, z) plane, f = +-(0, cos a, sin a).
    lv wall: phi_lv = 1 - X, phi_rv = 0, phi_epi = X: a = alpha_endo + c^2 (alpha_epi - alpha_endo), c = c_epi
    septum:  phi_lv = 1 - X, phi_rv = X, phi_epi = 0: a = alpha_endo (1 - 2 X)
    rv wall: phi_rv = 1 - X, phi_lv = 0, phi_epi = X: the lv wall's law."""
    xc = np.tile((np.arange(cells[0]) + 0.5) / cells[0], cells[1] * cells[2])
    a_endo, a_epi = np.deg2rad(angles_deg[0]), np.deg2rad(angles_deg[1])
    if region == "septum":
        return (lambda X: 1.0 - X, lambda X: X, lambda X: 0.0 * X), a_endo * (1.0 - 2.0 * xc)
    wall = (lambda X: 1.0 - X, lambda X: 0.0 * X, lambda X: X)
    angle = a_endo + xc**2 * (a_epi - a_endo)
    return (wall if region == "lv wall" else (wall[1], wall[0], wall[2])), angle
