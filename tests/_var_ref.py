"""Host reference of the per-node-coefficient diffusion solve (csrc/beat_pde_var.hip, the workgroup tiles of
csrc/beat_pde_vtl.hip, the opt-in csrc/beat_pde_vrr.hip) on voxel masks with a fibre field, iterate by iterate, and the table of
cases tests/test_var_iterates_gpu.py holds those kernels to it on; tests/test_var_ref_cpu.py checks the reference and the cases.

The PCG, the bounds and the constants are those of tests/_pcg_ref.py (pcg_iterates, reference, Reference, FACTOR, ...): nothing of
them is restated here.  What is new is the operator.  The device is given the (15, n) coefficient rows of
beat._stencil.stencil_fields(dim, cells, h, M, active); the host expands THOSE float64 rows over oracle.fem.STENCIL_OFFSETS into
CSR matrices, as _pcg_ref.expand does for the tables, and keeps the principal submatrix on the tissue nodes (mass_row[0] != 0):
the same numbers on both sides.  (The matrices oracle/fem assembles cell by cell differ from the rows by 1e-14 relative, which
would be operator noise in the yardstick; the CPU test compares the two.)  Plain numpy; no GPU code is imported.

Masks, each a deterministic function of the cell grid (cells are numbered x fastest):
  full      every cell;
  cutshell  the ellipsoidal shell 0.6 < r < 1.25 of tests/test_var_gpu.py's _shell_case, scaled so that it cuts every face of the
            box: tissue and tissue-free nodes on each of them;
  layers    single cell layers along z, layer c active where c % 12 is 0, 3 or 7: 2, 3 and 4 inactive layers between them, i.e.
            1, 2 and 3 node planes without tissue -- csrc/beat_var_plan.h (grow_runs) grows a run of planes over gaps of up to two and
            cuts it at three.  A box of fewer than 13 cell layers holds the first gaps only (layers_gaps says which);
  specks    isolated single cells (an 8-node system of their own each; those at i, j or k = 0 lie on a face), a line of cells along
            x over the cells 58 .. 64, whose nodes cross the end of the first 62-node x-segment (node 61 / 62), a line along y over
            the cells 5 .. 8, whose nodes cross the end of the first 8-row block (row 7 / 8), and every third cell of the last x column
            on the top plane.  The lines are what of them lies in the box: in a box 62 nodes wide the x line ENDS at node 61, in one of 9
            rows the y line ends on row 8 (specks_features says which feature a box holds).
A pair of box and mask exists where the box has room for what the mask is named for (CASES); the mask is never bent to fit."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import _pcg_ref as ref
from oracle import fem

MASKS = ("full", "cutshell", "layers", "specks")
# nodes (nx, ny, nz) -> dimension
SHAPES = {
    (125, 18, 20): 3,   # three x-segments, the last of one node; 8-row tiles with row blocks 8, 8, 2; more planes than a 16-plane run
    (63, 16, 6): 3,     # the second segment holds one node; exactly two full 8-row blocks
    (62, 9, 5): 3,      # exactly one segment; ny < 16: 4-row tiles, the right-hand side by the gather kernel
    (3, 70, 3): 3,      # many row blocks, ny % 8 = 6
    (6, 4, 71): 3,      # many runs along z
    (2, 2, 2): 3,       # the smallest box the tiles take
    (41, 32, 1): 2,     # 2-D and 1-D: the tile plan declines (vtl_sizes_declined, csrc/beat_var_plan.h), the segment-list kernels run
    (65, 1, 1): 1,
}
ALL_ROUTE_SHAPES = ((125, 18, 20), (62, 9, 5))  # every route of the GPU test runs on these, with every mask
# where a box has room for the mask's features (a shell needs a few cells per axis to be one: on 2 x 69 x 2 or 1 x 1 x 1 cells it is
# the full box or nothing; layers need four cell layers for their first gap; specks a column of cells beside their lines)
CASES = [(s, "full") for s in SHAPES] + \
    [(s, "cutshell") for s in ((125, 18, 20), (63, 16, 6), (62, 9, 5), (6, 4, 71), (41, 32, 1), (65, 1, 1))] + \
    [(s, "layers") for s in ((125, 18, 20), (63, 16, 6), (62, 9, 5), (6, 4, 71))] + \
    [(s, "specks") for s in ((125, 18, 20), (63, 16, 6), (62, 9, 5))]
GUESS_CASES = (((125, 18, 20), "cutshell"), ((63, 16, 6), "full"), ((62, 9, 5), "layers"))
RING = 12                       # PRING_MAX of csrc/beat_pde_internal.h: the directions a single slab keeps before x is updated
RING_SHORT = 6                  # PRING: BEAT_VAR_RING=6
CUTS = (1, 2, 3, RING + 1)      # max_it of the cut solves: 13 = a full ring flushed and the first direction of the second cycle
CUTS_SHORT = (1, 2, 3, RING_SHORT + 1)
# The slab-decomposed solve (tests/test_dist_iterates_gpu.py): (case, numbers of ranks); tests/test_dist_cases_cpu.py holds what each
# line is there for to the masks and to beat._engine.Slab
DIST_CASES = [(((125, 18, 20), m), (2, 3, 4)) for m in MASKS] + [  # 8-row tiles with a 2-row remainder; runs of planes cut by slab faces
    (((63, 16, 6), "full"), (2, 3)),       # two full row blocks
    (((63, 16, 6), "specks"), (2, 3)),
    (((63, 16, 6), "layers"), (2, 6)),     # 6 ranks: one-plane slabs, ranks 2 and 5 own no tissue node
    (((62, 9, 5), "full"), (2, 5)),        # 4-row tiles: no fused pass; the gather right-hand side in parts
    (((62, 9, 5), "layers"), (2, 5)),
    (((3, 70, 3), "full"), (3,)),          # one-plane slabs; ny % 8 = 6
    (((6, 4, 71), "layers"), (2, 8)),      # many runs along z, cut at 7 faces
    (((2, 2, 2), "full"), (2,)),           # the smallest box that can be cut
]
DIST_GUESS_CASES = ((((63, 16, 6), "full"), 2), (((125, 18, 20), "cutshell"), 3))  # (case, world)
# The cases off theta = 1/2 (sets of tests/_pcg_ref.py), each at both of ref.NEW_SETS: a dense box whose right-hand side runs on the
# 8-row tiles (the rows of B var_form_A_kernel forms), a shell on the same box, whose tissue meets across the edges of the x-segments
# and of the row blocks, and a box of 4-row tiles, whose right-hand side is the gather kernel's on every route.  All three hold every
# condition of a case under both sets (tests/test_var_ref_cpu.py; no mask or shape had to be moved).  Boxes of a few thousand nodes: the
# 45 000 nodes of 125 x 18 x 20 add nothing that tells one factor from another.
OPSET_CASES = (((63, 16, 6), "full"), ((63, 16, 6), "cutshell"), ((62, 9, 5), "layers"))
OPSET_GUESS_CASES = (((63, 16, 6), "full"), ((62, 9, 5), "layers"))  # of GUESS_CASES
OPSET_ROUTES = ("default", "three", "rows")  # of tests/test_var_iterates_gpu.py: the tile right-hand side twice, the gather kernel's
DIST_OPSET_CASES = {(((63, 16, 6), "full"), 3): ref.NEW_SETS}   # (case, world) of DIST_CASES
DIST_OPSET_GUESS = {(((63, 16, 6), "full"), 2): ("skew",)}      # of DIST_GUESS_CASES, the one of a few thousand nodes
SEED_SHIFT: dict = {}           # case -> added to its seed, should a seed put a stop within 1e-6 of its threshold (test_var_ref_cpu)


def case_key(case) -> str:
    return f"{ref.shape_key(case[0])}-{case[1]}"


def cells_of(shape) -> tuple:
    return tuple(s - 1 for s in shape[: SHAPES[tuple(shape)]])


def seed_of(case) -> int:
    shape, mask = case
    nx, ny, nz = shape
    return 7_000_003 * nx + 10_007 * ny + 101 * nz + MASKS.index(mask) + SEED_SHIFT.get((tuple(shape), mask), 0)


def cell_centres(cells) -> np.ndarray:
    """Cell centres in [0, 1]^d, cells numbered x fastest (as _shell_case of tests/test_var_gpu.py)."""
    d = len(cells)
    cc = np.stack(np.meshgrid(*[(np.arange(c) + 0.5) / c for c in reversed(cells)], indexing="ij"), axis=-1)[..., ::-1]
    return cc.reshape(-1, d)


def layers_gaps(cells_z: int) -> set:
    """The gaps (node planes without tissue between planes with tissue) the layers mask has in a box of cells_z cell layers."""
    return {g for g, need in ((1, 4), (2, 8), (3, 13)) if cells_z >= need}


def specks_features(shape) -> dict:
    nx, ny, _ = shape
    return {"x_line_crosses_61_62": nx >= 63, "x_line_ends_at_61": nx == 62, "y_line_crosses_7_8": ny >= 9}


def _dilate(a: np.ndarray) -> np.ndarray:
    """a, grown by one cell in every direction (diagonals included)."""
    out = a.copy()
    for axis in range(a.ndim):
        grown = out.copy()
        lo, hi = [slice(None)] * a.ndim, [slice(None)] * a.ndim
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        grown[tuple(lo)] |= out[tuple(hi)]
        grown[tuple(hi)] |= out[tuple(lo)]
        out = grown
    return out


def mask_of(cells, name: str) -> np.ndarray:
    """bool per box cell, x fastest."""
    d = len(cells)
    if name == "full":
        return np.ones(int(np.prod(cells)), dtype=bool)
    if name == "cutshell":
        r = np.sqrt((((cell_centres(cells) - 0.5) / 0.5) ** 2).sum(axis=1))
        return (r > 0.6) & (r < 1.25)
    assert d == 3, "layers and specks are masks of 3-D boxes"
    cx, cy, cz = cells
    k, j, i = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
    if name == "layers":
        return np.isin(k % 12, (0, 3, 7)).ravel()
    if name == "specks":
        lines = ((i >= 58) & (i <= 64) & (j == 2) & (k == 1)) | ((j >= 5) & (j <= 8) & (i == 6) & (k == 1)) | \
                ((i == cx - 1) & (k == cz - 1) & (j % 3 == 0))
        lone = (i % 4 == 0) & (j % 4 == 0) & (k % 3 == 0) & ~_dilate(lines)
        return (lines | lone).ravel()
    raise KeyError(name)


def fibre_tensors(cells, seed: int) -> np.ndarray:
    """Per-cell conductivity of a fibre field that rotates along x, with noise (as _shell_case of tests/test_var_gpu.py)."""
    rng = np.random.default_rng(seed)
    d = len(cells)
    cc = cell_centres(cells)
    ang = np.pi * cc[:, 0] + 0.3 * rng.standard_normal(len(cc))
    f = np.zeros((len(cc), d))
    f[:, 0] = np.cos(ang)
    if d > 1:
        f[:, 1] = np.sin(ang)
    s_l, s_t = 9.5e-4, 1.25e-4
    return s_t * np.eye(d)[None] + (s_l - s_t) * f[:, :, None] * f[:, None, :]


def expand_rows(rows: np.ndarray, shape, keep: np.ndarray) -> sp.csr_matrix:
    """The matrix the (15, n) rows apply -- entry (i, i + offset k) = rows[k, i] for every offset that stays inside the box -- cut
    to the nodes of ``keep`` (rows and columns, renumbered in node order); zero entries kept: one pattern for every operator."""
    nx, ny, nz = shape
    n = nx * ny * nz
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    new = np.full(n, -1, dtype=np.int64)
    new[keep] = np.arange(int(keep.sum()))
    r_, c_, v_ = [], [], []
    for k, (ox, oy, oz) in enumerate(fem.STENCIL_OFFSETS):
        jx, jy, jz = ix + ox, iy + oy, iz + oz
        ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny) & (jz >= 0) & (jz < nz)
        row = np.nonzero(ok)[0]
        col = (jx + nx * (jy + ny * jz))[ok]
        both = keep[row] & keep[col]
        r_.append(new[row[both]])
        c_.append(new[col[both]])
        v_.append(rows[k, row[both]])
    r_, c_, v_ = np.concatenate(r_), np.concatenate(c_), np.concatenate(v_)
    order = np.lexsort((c_, r_))
    m = int(keep.sum())
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r_, minlength=m))])
    out = sp.csr_matrix((v_[order], c_[order], indptr), shape=(m, m))
    assert out.has_sorted_indices and (np.diff(out.indptr) > 0).all()
    return out


def dropped_entries(rows: np.ndarray, shape, keep: np.ndarray) -> float:
    """max |entry| of what expand_rows leaves out: couplings of a kept node with a node that is not kept or not in the box, and the
    rows of the nodes that are not kept.  Zero for coefficient rows of a mask, exactly (test_var_ref_cpu)."""
    nx, ny, nz = shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    worst = 0.0
    for k, (ox, oy, oz) in enumerate(fem.STENCIL_OFFSETS):
        jx, jy, jz = ix + ox, iy + oy, iz + oz
        ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny) & (jz >= 0) & (jz < nz)
        col = np.where(ok, jx + nx * (jy + ny * jz), 0)
        kept = ok & keep & keep[col]
        worst = max(worst, float(np.abs(rows[k][~kept]).max(initial=0.0)))
    return worst


@dataclass
class Case:
    shape: tuple
    mask: str
    dim: int
    cells: tuple
    active: np.ndarray        # bool per box cell
    M: np.ndarray             # (cells, dim, dim)
    mass_rows: np.ndarray     # the (15, n) rows the device is given ...
    stiff_rows: np.ndarray
    tissue: np.ndarray        # bool per node: mass_rows[0] != 0
    problem: ref.Problem      # ... and the same numbers as matrices on the tissue nodes (n = their number)
    stim_cells: tuple         # two sets of simplices (ids of oracle/fem's mesh of the box)

    @property
    def n_nodes(self) -> int:
        return int(np.prod(self.shape))

    @property
    def n(self) -> int:
        return self.problem.n


_cases: dict = {}


def mesh_of(cells) -> fem.BoxMesh:
    return fem.BoxMesh(tuple(cells), tuple(ref.H * c for c in cells))


def simplices_per_cell(dim: int) -> int:
    return {1: 1, 2: 2, 3: 6}[dim]


def case(c) -> Case:
    shape, mask = tuple(int(s) for s in c[0]), c[1]
    key = (shape, mask)
    if key in _cases:
        return _cases[key]
    from beat import _stencil  # (numpy only)

    dim, cells = SHAPES[shape], cells_of(shape)
    active = mask_of(cells, mask)
    M = fibre_tensors(cells, seed_of(key))
    mf, kf = _stencil.stencil_fields(dim, cells, (ref.H,) * dim, M, active)
    assert mf.shape == kf.shape == (15, int(np.prod(shape))) and mf.dtype == np.float64
    tissue = mf[0] != 0.0
    mass, stiff = expand_rows(mf, shape, tissue), expand_rows(kf, shape, tissue)
    assert np.array_equal(mass.indices, stiff.indices) and np.array_equal(mass.indptr, stiff.indptr)
    A = sp.csr_matrix((ref.CN.c_m * mass.data + ref.CN.theta * ref.CN.dt * stiff.data, mass.indices, mass.indptr), shape=mass.shape)
    # two stimuli over subsets of the active simplices: the first third, and every third of the second half
    act_s = np.nonzero(np.repeat(active, simplices_per_cell(dim)))[0]
    na = len(act_s)
    sets = (act_s[: max(1, na // 3)], act_s[na // 2:][1::3] if na >= 6 else act_s[-1:])
    mesh = mesh_of(cells)
    weights = [fem.stimulus_weights(mesh, s)[tissue] for s in sets]
    p = ref.Problem(shape, dim, mf, kf, mass, stiff, A, weights, mass.shape[0], ref.CN)
    _cases[key] = Case(shape, mask, dim, cells, active, M, mf, kf, tissue, p, sets)
    return _cases[key]


def assembled(cs: Case):
    """(Mass, K) assembled cell by cell by oracle/fem over the active simplices with the per-cell tensors, on ALL nodes of the box."""
    spc = simplices_per_cell(cs.dim)
    act_s = np.repeat(cs.active, spc)
    Ms = np.repeat(cs.M, spc, axis=0) * act_s[:, None, None]
    mesh = mesh_of(cs.cells)
    return fem.assemble_mass(mesh, np.nonzero(act_s)[0]), fem.assemble_stiffness(mesh, Ms)


def field(cs: Case, j: int = 0) -> np.ndarray:
    """v of solve j on the tissue nodes: _pcg_ref.field's recipe (zero-mean O(1) noise; for j >= 1 plus two more noise fields whose
    weights move between solves) with the case's seed."""
    rng = np.random.default_rng(seed_of((cs.shape, cs.mask)) + 17)
    v0, w1, w2 = (rng.standard_normal(cs.n) for _ in range(3))
    v0, w1, w2 = v0 - v0.mean(), w1 - w1.mean(), w2 - w2.mean()
    if j == 0:
        return v0
    return v0 + np.sin(0.9 * j) * w1 + np.cos(1.7 * j) * w2


def off_tissue_marks(cs: Case) -> np.ndarray:
    """What v holds off the tissue: 1000 + node index -- recognisable, so 'untouched' can be told from 'copied' or 'zeroed'."""
    return 1000.0 + np.nonzero(~cs.tissue)[0].astype(np.float64)


def on_box(cs: Case, v_tissue: np.ndarray) -> np.ndarray:
    """The field of all nodes of the box the device is given: v on the tissue, the marks off it."""
    out = np.empty(cs.n_nodes)
    out[cs.tissue] = v_tissue
    out[~cs.tissue] = off_tissue_marks(cs)
    return out


def weights_on_box(cs: Case) -> list:
    out = []
    for w in cs.problem.weights:
        full = np.zeros(cs.n_nodes)
        full[cs.tissue] = w
        out.append(full)
    return out


def kmax_of(cs: Case) -> int:
    """KMAX, or the number of tissue unknowns where that is smaller."""
    return min(ref.KMAX, cs.n)


def cuts_of(cs: Case, cuts=CUTS) -> tuple:
    """The cuts that happen no later than CG can run: at most the number of unknowns."""
    return tuple(k for k in cuts if k <= cs.n)


_plain: dict = {}
_problems: dict = {}


def problem_of(c, ops="cn") -> ref.Problem:
    """The case's matrices under a set of ref.OPSETS (case(c).problem is the one under cn)."""
    cs, ops = case(c), ref.opset(ops)
    if ops == ref.CN:
        return cs.problem
    key = (cs.shape, cs.mask, ops)
    if key not in _problems:
        _problems[key] = cs.problem.with_ops(ops)
    return _problems[key]


def opset_key(c, ops="cn") -> str:
    """case_key for cn (the keys from before the sets had names do not change), case@set otherwise."""
    name = ref.opset(ops).name
    return case_key(c) if name == "cn" else f"{case_key(c)}@{name}"


def plain_reference(c, ops="cn") -> ref.Reference:
    """The solve from x0 = v = field(case), kmax_of iterations; computed once per case and set."""
    cs, ops = case(c), ref.opset(ops)
    key = (cs.shape, cs.mask) if ops == ref.CN else (cs.shape, cs.mask, ops)
    if key not in _plain:
        v, p = field(cs), problem_of(c, ops)
        _plain[key] = ref.reference(p, ref.rhs_longdouble(p, v), v.astype(np.longdouble), kmax_of(cs))
    return _plain[key]
