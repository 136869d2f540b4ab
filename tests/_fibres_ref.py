"""NumPy restatement of the rule-based fibre rule (include/beat_hip.h: beat_fibres_rule), written from the rule's text, and the inputs
the CPU and the GPU tests share (test_fibres_cpu.py, test_fibres_gpu.py).

Voxels and nodes are numbered x fastest; a voxel's corner (i, j, k) in {0, 1}^3 is the node at that offset from its lowest one."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

GRIDS = ((1, 1, 1), (5, 3, 2), (65, 2, 2), (130, 3, 3))  # a row that crosses a wave, one that crosses a 256-thread block in x
H = (0.3, 0.2, 0.25)
ANGLES = (60.0, -60.0, 20.0, -20.0)  # alpha_endo, alpha_epi, beta_endo, beta_epi in degrees
AXIS = (0.2, -0.1, 1.0)
S_L, S_T = 9.5301e-4, 1.2576e-4
TOL = 1e-12  # per component of f, s, n, header and device against this file: ~40 rounded operations and two sin / cos of a few ulp
# each, amplified at most 1 / |r|^2 <= 4 by the normalisations, is <~ 1e-13


def corners(field, cells):
    """(2, 2, 2, nvoxels): [i, j, k, v] = the nodal value at corner (i, j, k) of voxel v."""
    cx, cy, cz = cells
    a = np.asarray(field, dtype=np.float64).reshape(cz + 1, cy + 1, cx + 1)
    out = np.empty((2, 2, 2, cx * cy * cz))
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                out[i, j, k] = a[k : k + cz, j : j + cy, i : i + cx].ravel()
    return out


def gradient(c, h):
    """(nvoxels, 3): the trilinear field's gradient at the voxel centre = per axis the mean of the four edge differences / spacing."""
    dx = (c[1] - c[0]).reshape(4, -1).mean(axis=0) / h[0]
    dy = (c[:, 1] - c[:, 0]).reshape(4, -1).mean(axis=0) / h[1]
    dz = (c[:, :, 1] - c[:, :, 0]).reshape(4, -1).mean(axis=0) / h[2]
    return np.stack([dx, dy, dz], axis=1)


def rule(cells, h, phi, longitudinal, angles_deg=ANGLES, active=None, s_l=S_L, s_t=S_T):
    """The rule on every voxel.  ``longitudinal``: nodal values of psi, or a 3-vector.  Returns f, s, n (nvoxels, 3), M (nvoxels, 3, 3),
    the bool mask and the number of the degenerate voxels, and ``r`` = |r| of step 3 (NaN where it is not defined)."""
    nvox = int(np.prod(cells))
    act = np.ones(nvox, dtype=bool) if active is None else np.asarray(active, dtype=bool).ravel()
    cphi = corners(phi, cells)
    gphi = gradient(cphi, h)
    longitudinal = np.asarray(longitudinal, dtype=np.float64)
    gpsi = np.tile(longitudinal, (nvox, 1)) if longitudinal.shape == (3,) else gradient(corners(longitudinal, cells), h)
    phic = np.clip(cphi.reshape(8, -1).mean(axis=0), 0.0, 1.0)
    a_endo, a_epi, b_endo, b_epi = np.deg2rad(np.asarray(angles_deg, dtype=np.float64))
    f, s, n = np.zeros((nvox, 3)), np.zeros((nvox, 3)), np.zeros((nvox, 3))
    rnorm = np.full(nvox, np.nan)
    degenerate = np.zeros(nvox, dtype=bool)
    for v in np.nonzero(act)[0]:
        nphi, npsi = np.linalg.norm(gphi[v]), np.linalg.norm(gpsi[v])
        if nphi == 0.0 or npsi == 0.0:
            degenerate[v] = True
            continue
        e_l = gpsi[v] / npsi
        t = gphi[v] / nphi
        r = t - np.dot(e_l, t) * e_l
        rnorm[v] = np.linalg.norm(r)
        if rnorm[v] <= 1e-12:
            degenerate[v] = True
            continue
        e_t = r / rnorm[v]
        e_c = np.cross(e_l, e_t)
        alpha = a_endo * (1.0 - phic[v]) + a_epi * phic[v]
        beta = b_endo * (1.0 - phic[v]) + b_epi * phic[v]
        f[v] = np.cos(alpha) * e_c + np.sin(alpha) * e_l
        g = -np.sin(alpha) * e_c + np.cos(alpha) * e_l
        s[v] = np.sin(beta) * g + np.cos(beta) * e_t
        n[v] = np.cos(beta) * g - np.sin(beta) * e_t
    M = s_t * np.eye(3)[None] + (s_l - s_t) * np.einsum("vi,vj->vij", f, f)
    M[~act] = 0.0
    return SimpleNamespace(f=f, s=s, n=n, M=M, degenerate=degenerate, count=int(degenerate.sum()), r=rnorm, active=act)


def mask(cells):
    """One mask with isolated and missing voxels (the single voxel of (1, 1, 1) stays)."""
    nvox = int(np.prod(cells))
    rng = np.random.default_rng(20260 + nvox)
    m = rng.random(nvox) < 0.6
    m[0] = True
    return m


@lru_cache(maxsize=None)
def case(cells, psi_as_field, masked):
    """Inputs and reference of one case, computed once: phi = (ix + 0.1 u) / cx, psi = (iz + 0.1 u') / cz at the nodes, u, u' uniform in
    [0, 1) from a fixed seed; the longitudinal input is psi or the constant AXIS."""
    cx, cy, cz = cells
    rng = np.random.default_rng(1234 + cx + 7 * cy + 31 * cz)
    shape = (cz + 1, cy + 1, cx + 1)
    iz, _, ix = np.meshgrid(*(np.arange(m, dtype=np.float64) for m in shape), indexing="ij")
    phi = ((ix + 0.1 * rng.random(shape)) / cx).ravel()
    psi = ((iz + 0.1 * rng.random(shape)) / cz).ravel()
    active = mask(cells) if masked else None
    ref = rule(cells, H, phi, psi if psi_as_field else np.array(AXIS), ANGLES, active)
    for a in (phi, psi, ref.f, ref.s, ref.n, ref.M):
        a.setflags(write=False)
    return SimpleNamespace(cells=cells, h=H, phi=phi, psi=psi if psi_as_field else None, axis=None if psi_as_field else np.array(AXIS),
                           active=active, ref=ref)


CASES = [(cells, psi_as_field, masked) for cells in GRIDS for psi_as_field in (True, False) for masked in (False, True)]


def assert_well_conditioned(ref):
    """The tolerance's condition: on these inputs the sine of the angle between the two directions is >= 0.5."""
    r = ref.r[ref.active]
    assert np.isfinite(r).all() and r.min() >= 0.5, r.min()
