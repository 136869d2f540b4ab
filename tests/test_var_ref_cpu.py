"""The host reference of tests/_var_ref.py held to account, and the conditions its cases must meet for
tests/test_var_iterates_gpu.py to mean what it says: the expanded coefficient rows are the matrices oracle/fem assembles cell by
cell, the tissue is what the active cells touch, every mask has the features it is named for (computed from the mask), the
reference converges, no stop is a near tie (so the device's iteration count can be asked to EQUAL the host's), every cut can
happen, and the yardstick sees the kind of slip the GPU test is there for."""
from pathlib import Path

import numpy as np
import pytest
from scipy.sparse.csgraph import connected_components

import _pcg_ref as ref
import _var_ref as vr

CASES = list(vr.CASES)
# (case, set): every case under cn, as before the sets had names (and under the same test ids), then the pairs off theta = 1/2
PAIRS = [(c, "cn") for c in CASES] + [(c, name) for c in vr.OPSET_CASES for name in ref.NEW_SETS]
GUESS_PAIRS = [(c, "cn") for c in vr.GUESS_CASES] + [(c, name) for c in vr.OPSET_GUESS_CASES for name in ref.NEW_SETS]
SEG = 62  # x-nodes per segment of the tile kernels (csrc/beat_pde_vtl.hip, csrc/beat_pde_vrr.hip)


def grid(cs, a):
    """A per-node array as [z, y, x]."""
    nx, ny, nz = cs.shape
    return np.asarray(a).reshape(nz, ny, nx)


def gaps_along_z(cs) -> set:
    """Lengths of the runs of node planes without tissue that lie BETWEEN planes with tissue."""
    has = grid(cs, cs.tissue).any(axis=(1, 2))
    at = np.nonzero(has)[0]
    return {int(b - a - 1) for a, b in zip(at[:-1], at[1:]) if b - a > 1}


def test_case_table_is_consistent():
    assert len(CASES) == len(set(CASES)) and len({vr.seed_of(c) for c in CASES}) == len(CASES)
    assert all(s in vr.SHAPES and m in vr.MASKS for s, m in CASES)
    assert {s for s, _ in CASES} == set(vr.SHAPES) and all((s, "full") in CASES for s in vr.SHAPES)
    assert all((s, m) in CASES for s in vr.ALL_ROUTE_SHAPES for m in vr.MASKS)  # every route meets every mask
    assert set(vr.GUESS_CASES) <= set(CASES)
    assert max(int(np.prod(s)) for s in vr.SHAPES) <= 45_000  # the sizes at which the tiling branches, not the workload
    # off theta = 1/2: a few thousand nodes; a dense and a masked box on 8-row tiles, one on 4-row tiles; guess cases of GUESS_CASES
    assert set(vr.OPSET_CASES) <= set(CASES) and set(vr.OPSET_GUESS_CASES) <= set(vr.OPSET_CASES) & set(vr.GUESS_CASES)
    assert max(int(np.prod(s)) for s, _ in vr.OPSET_CASES) <= 8192
    assert any(m == "full" and s[1] >= 16 for s, m in vr.OPSET_CASES) and any(m != "full" and s[1] >= 16 for s, m in vr.OPSET_CASES)
    assert any(s[1] < 16 for s, _ in vr.OPSET_CASES)
    assert all(c in dict(vr.DIST_CASES) and w in dict(vr.DIST_CASES)[c] for c, w in vr.DIST_OPSET_CASES) and set(vr.DIST_OPSET_GUESS) <= set(vr.DIST_GUESS_CASES)
    src = (Path(__file__).resolve().parents[1] / "fenicsx-beat_amd" / "csrc" / "beat_pde_internal.h").read_text()
    assert f"constexpr int PRING_MAX = {vr.RING};" in src and f"constexpr int PRING = {vr.RING_SHORT};" in src
    assert vr.CUTS[-1] == vr.RING + 1 and vr.CUTS_SHORT[-1] == vr.RING_SHORT + 1
    # what the shapes are there for
    assert -(-125 // SEG) == 3 and 125 % SEG == 1 and -(-18 // 8) == 3 and 18 % 8 == 2 and 20 > 16
    assert -(-63 // SEG) == 2 and 63 % SEG == 1 and 16 % 8 == 0
    assert 62 == SEG and 9 < 16 and 70 % 8 == 6


@pytest.mark.parametrize("c", CASES, ids=vr.case_key)
def test_expanded_rows_are_the_assembled_matrices_on_the_tissue(c):
    """The rows the device is given, expanded over the box and cut to the tissue, against oracle/fem's cell-by-cell assembly over
    the active simplices with the per-cell tensors.  Measured: <= 1.1e-14 max|entry| (125 x 18 x 20 specks), 0 - 1e-14 elsewhere;
    the bound is that of tests/test_pcg_ref_cpu.py -- the assembly takes a cell's geometry from its nodes' coordinates, u *
    coordinate / h --: 4 max(shape) 2^-53 (5.6e-14 on the largest box, 8.9e-16 on 2 x 2 x 2).  Nothing of the rows lies outside the
    tissue block, exactly: the cut loses nothing."""
    cs = vr.case(c)
    p = cs.problem
    Mass, K = vr.assembled(cs)
    t = cs.tissue
    # the tissue is the set of nodes an active cell touches, from the mask alone
    nx, ny, nz = cs.shape
    c3 = list(cs.cells) + [1] * (3 - cs.dim)
    act = cs.active.reshape(c3[2], c3[1], c3[0])
    touched = np.zeros((nz, ny, nx), dtype=bool)
    for corner in range(2 ** cs.dim):
        o = [(corner >> a) & 1 if a < cs.dim else 0 for a in range(3)]
        touched[o[2]: o[2] + c3[2], o[1]: o[1] + c3[1], o[0]: o[0] + c3[0]] |= act
    assert np.array_equal(t, touched.ravel())
    assert np.array_equal(t, Mass.diagonal() > 0)
    assert 0 < p.n == int(t.sum()) and (c[1] == "full") == bool(t.all())
    noise = 4 * max(cs.shape) * 2.0**-53
    for name, mine, rows, theirs in (("mass", p.mass, cs.mass_rows, Mass), ("stiffness", p.stiff, cs.stiff_rows, K)):
        assert vr.dropped_entries(rows, cs.shape, t) == 0.0, name
        sub = theirs.tocsr()[t][:, t]
        dist = abs(mine - sub).max() / abs(theirs).max()
        print(f"{vr.case_key(c)} {name}: rows against assembly {dist:.2e} (bound {noise:.2e})")
        assert dist <= noise, (name, dist, noise)
        off = theirs.tocsr()[~t]
        assert off.nnz == 0 or abs(off).max() == 0.0
    assert abs(p.A - p.A.T).max() <= 8 * 2.0**-53 * abs(p.A).max()
    assert (p.mass.diagonal() > 0).all() and (p.A.diagonal() > 0).all()
    # the stimuli act on the tissue, differ, and are not everywhere
    w0, w1 = p.weights
    assert (w0 > 0).any() and (w1 > 0).any() and not np.array_equal(w0 > 0, w1 > 0)


@pytest.mark.parametrize("c", CASES, ids=vr.case_key)
def test_mask_has_the_features_it_is_named_for(c):
    cs = vr.case(c)
    shape, mask = c
    nx, ny, nz = shape
    t = grid(cs, cs.tissue)
    faces = [t[:, :, 0], t[:, :, -1]] + ([t[:, 0, :], t[:, -1, :]] if cs.dim >= 2 else []) + ([t[0], t[-1]] if cs.dim == 3 else [])
    nseg = -(-nx // SEG)
    with_tissue = [bool(t[:, :, s * SEG: (s + 1) * SEG].any()) for s in range(nseg)]
    if mask in ("full", "cutshell", "layers"):
        assert all(with_tissue), with_tissue  # every x-segment of the box holds tissue
    if mask == "full":
        assert t.all()
    if mask in ("full", "cutshell"):
        assert all(f.any() for f in faces)  # tissue on each face of the box
    if mask == "cutshell":
        assert not t.all() and not cs.active.all()
        if cs.dim >= 2:
            assert all(not f.all() for f in faces)  # the shell CUTS each face: tissue-free nodes on it too
        else:
            assert not t[0, 0, nx // 2]  # 1-D: two pieces of tissue
    if nx % SEG == 1:
        assert nseg >= 2 and t[:, :, nx - 1].any() and with_tissue[-1]  # the last segment is one node, and holds tissue
    if mask == "layers":
        planes = t.any(axis=(1, 2))
        assert all(t[z].all() or not t[z].any() for z in range(nz))  # whole planes
        assert gaps_along_z(cs) == vr.layers_gaps(cs.cells[2]) and 1 in gaps_along_z(cs)
        assert planes[0] and t[0].all()  # the z = 0 face is tissue
    if mask == "specks":
        cx, cy, cz = cs.cells
        act = np.pad(cs.active.reshape(cz, cy, cx), 1)
        around = sum(act[1 + dz: 1 + dz + cz, 1 + dy: 1 + dy + cy, 1 + dx: 1 + dx + cx]
                     for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        lone = act[1:-1, 1:-1, 1:-1] & (around == 1)
        assert lone.sum() >= 4
        # ... which is a system of 8 unknowns of its own in the matrix
        coupled = cs.problem.A.copy()
        coupled.eliminate_zeros()  # (the pattern keeps zero entries between neighbouring nodes of different pieces)
        ncomp, label = connected_components(coupled, directed=False)
        sizes = np.bincount(label)
        assert (sizes == 8).sum() == lone.sum() and ncomp > lone.sum()
        assert lone[0].any() and lone[:, 0].any() and lone[:, :, 0].any()  # some of them on the faces z = 0, y = 0, x = 0
        f = vr.specks_features(shape)
        assert f["x_line_crosses_61_62"] != f["x_line_ends_at_61"]
        assert t[1, 2, 58:62].all() and not t[1, 2, 57]
        if f["x_line_crosses_61_62"]:
            assert t[1, 2, 61] and t[1, 2, 62] and nseg >= 2
        else:
            assert nx == SEG and t[1, 2, nx - 1]
        assert f["y_line_crosses_7_8"] and t[1, 7, 6] and t[1, 8, 6] and not t[1, 4, 6]
        assert t[nz - 1, :, nx - 1].any() and not t[nz - 1, :, nx - 1].all() and not t[nz - 1, :, nx - 3].any()
        assert with_tissue[-1] and all(with_tissue)


def test_the_masks_together_hold_every_gap_and_every_line_feature():
    gaps = set()
    for c in CASES:
        if c[1] == "layers":
            gaps |= gaps_along_z(vr.case(c))
    assert gaps == {1, 2, 3}  # csrc/beat_var_plan.h (grow_runs) grows a run over gaps of 1 and 2 planes and cuts it at 3
    assert gaps_along_z(vr.case(((125, 18, 20), "layers"))) == {1, 2, 3}
    feats = [vr.specks_features(s) for s, m in CASES if m == "specks"]
    assert any(f["x_line_crosses_61_62"] for f in feats) and any(f["x_line_ends_at_61"] for f in feats)


def test_masked_case_off_cn_has_tissue_meeting_across_tile_edges():
    """63 x 16 x 6 cutshell: tissue on both sides of the edge between the x-segments (nodes 61 | 62) and between the two 8-row blocks
    (rows 7 | 8), coupled across them by rows of K."""
    cs = vr.case(((63, 16, 6), "cutshell"))
    t = grid(cs, cs.tissue)
    assert (t[:, :, 61] & t[:, :, 62]).any() and (t[:, 7, :] & t[:, 8, :]).any() and not t.all()
    kx = [k for k, o in enumerate(fem_offsets()) if o == (1, 0, 0)][0]
    ky = [k for k, o in enumerate(fem_offsets()) if o == (0, 1, 0)][0]
    assert (grid(cs, cs.stiff_rows[kx])[:, :, 61] != 0).any() and (grid(cs, cs.stiff_rows[ky])[:, 7, :] != 0).any()


def fem_offsets():
    from oracle import fem

    return [tuple(o) for o in fem.STENCIL_OFFSETS]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda pair: vr.opset_key(*pair))
def test_reference_converges_and_no_stop_is_a_near_tie(pair):
    c, ops = pair[0], ref.opset(pair[1])
    cs, r = vr.case(c), vr.plain_reference(c, ops)
    p = vr.problem_of(c, ops)
    assert p.ops == ops and p.mass is cs.problem.mass
    v = vr.field(cs)
    assert abs(v.mean()) < 1e-12 and 0.1 < np.abs(v).max() < 10.0 and np.array_equal(v, vr.field(cs))
    box = vr.on_box(cs, v)
    assert np.array_equal(box[cs.tissue], v) and (box[~cs.tissue] >= 1000.0).all()
    bL = ref.rhs_longdouble(p, v)
    C_m, theta, dt = ops.triple
    b64 = C_m * (p.mass @ v) - (1 - theta) * dt * (p.stiff @ v) + dt * sum(a * w for a, w in zip(ref.STIM_AMPS, p.weights))
    assert np.array_equal(b64, p.rhs_float64(v))
    assert abs(p.A - (C_m * p.mass + theta * dt * p.stiff)).max() <= 2 * 2.0**-53 * abs(p.A).max()
    assert np.abs(bL.astype(np.float64) - b64).max() <= 16 * 2.0**-53 * np.abs(b64).max()
    assert r.kmax == vr.kmax_of(cs) <= ref.KMAX
    assert r.rL[r.kmax] <= np.longdouble(1e-9) * r.bL
    # converged: the residual of the float64 matrix at the last iterate
    res = b64 - p.A @ r.xL[r.kmax].astype(np.float64)
    assert np.linalg.norm(res) <= 1e-12 * np.linalg.norm(b64)
    for rtol in ref.RTOLS:
        k = r.stop(rtol)
        thr = np.longdouble(rtol) * r.bL
        assert r.rL[k] <= thr * (1 - 1e-6), (rtol, k, float(r.rL[k] / thr))
        if k > 1:
            assert r.rL[k - 1] >= thr * (1 + 1e-6), (rtol, k, float(r.rL[k - 1] / thr))
        assert k <= r.kmax
    for cuts in (vr.CUTS, vr.CUTS_SHORT):
        ks = vr.cuts_of(cs, cuts)
        assert ks and all(k <= cs.n and k <= r.kmax for k in ks)
        assert ks == cuts or cs.n < max(cuts)
        for k in ks:
            assert 0.0 < r.x_bound(k) <= 1e-12 * max(1.0, np.abs(r.xL[k]).max()) and r.residual_bound(k) > 0.0
    assert r.rhs_norm_bound() > 0.0
    if cs.n > 100:  # the cut behind the ring flush happens while the iterate still moves
        assert r.rL[vr.RING + 1] > np.longdouble(1e-9) * r.bL and r.stop(ref.RTOLS[0]) >= vr.RING
    if ops != ref.CN:  # the conditions of tests/test_pcg_ref_cpu.py, in full: converged to 1e-12 at KMAX, a cut at 7 is a cut
        assert r.rL[r.kmax] <= np.longdouble(1e-12) * r.bL and r.rL[7] > np.longdouble(1e-12) * r.bL
        assert r.rL[max(vr.CUTS)] > np.longdouble(1e-12) * r.bL


@pytest.mark.parametrize("c", CASES, ids=vr.case_key)
def test_yardstick_sees_a_partial_sum_counted_twice(c):
    """One plausible slip, emulated on the host in longdouble: the partial of p.Ap of one tile (the nodes of the first 62 x 8 x 16
    block of the box that are tissue) added twice in the first iteration.  The step length is wrong by the tile's share, the
    iterate 1 moves by far more than x_bound(1) -- and a converged solve would not notice.  Likewise beta dropped on a few nodes
    of the direction of iteration 2."""
    L = np.longdouble
    cs, r = vr.case(c), vr.plain_reference(c)
    p = cs.problem
    A = p.operator(L)
    v = vr.field(cs).astype(L)
    b = ref.rhs_longdouble(p, vr.field(cs))
    dinv = L(1) / p.diagonal(L)
    res = b - ref.matvec(A, v, L)
    z = dinv * res
    q = ref.matvec(A, z, L)
    alpha = (res @ z) / (z @ q)
    x1 = v + alpha * z
    assert np.abs(x1 - r.xL[1]).max() <= 2.0**-58 * np.abs(r.xL[1]).max()
    nx, ny, nz = cs.shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    tile = ((ix < SEG) & (iy < 8) & (iz < 16)).ravel()[cs.tissue]
    assert tile.any()
    twice = (res @ z) / (z @ q + z[tile] @ q[tile])
    moved = float(np.abs(v + twice * z - r.xL[1]).max())
    assert moved > 1e6 * r.x_bound(1), (moved, r.x_bound(1))
    if cs.n > 2:
        # iteration 2 with beta dropped on the last tissue node of the direction
        res1 = res - alpha * q
        z1 = dinv * res1
        beta = (res1 @ z1) / (res @ z)
        p1 = z1 + beta * z
        assert np.abs(x1 + (res1 @ z1) / (p1 @ ref.matvec(A, p1, L)) * p1 - r.xL[2]).max() <= 2.0**-56 * np.abs(r.xL[2]).max()
        p1[-1] = z1[-1]
        slipped = x1 + (res1 @ z1) / (p1 @ ref.matvec(A, p1, L)) * p1
        assert float(np.abs(slipped - r.xL[2]).max()) > 1e3 * r.x_bound(2)


@pytest.mark.parametrize("pair", GUESS_PAIRS, ids=lambda pair: vr.opset_key(*pair))
def test_guess_sequence_moves_and_its_cuts_happen_before_convergence(pair):
    """The fields of the guess cases with the host's own converged solves in place of the device's: the extrapolated start is still
    O(1) wrong, so the cut iterates (k = 1, 3) are far from converged."""
    c = pair[0]
    cs = vr.case(c)
    p = vr.problem_of(*pair)
    incs = []
    for j in range(1, ref.GUESS_SOLVES + 1):
        v = vr.field(cs, j)
        x = ref.reference(p, ref.rhs_longdouble(p, v), v.astype(np.longdouble), 40).xD[40]
        incs.insert(0, x - v)
    v = vr.field(cs, ref.GUESS_SOLVES + 1)
    bL = ref.rhs_longdouble(p, v)
    for order in ref.GUESS_ORDERS:
        e = ref.guess_increment(order, incs)
        r = ref.reference(p, bL, v.astype(np.longdouble) + e, max(ref.GUESS_CUTS))
        assert r.rL[max(ref.GUESS_CUTS)] > np.longdouble(1e-12) * r.bL
        assert r.rL[1] > np.longdouble(1e-3) * r.bL  # the guess did not all but solve it
        for k in ref.GUESS_CUTS:
            assert r.x_bound(k) > 0.0
