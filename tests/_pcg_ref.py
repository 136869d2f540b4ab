"""Host reference of the production diffusion solve, iterate by iterate, and the tables of cases the register-row kernels
(csrc/beat_pde_rr.hip; SHAPES, tests/test_rr_iterates_gpu.py runs them) and the one-launch solve of small grids
(csrc/beat_pde_small.hip; SMALL_SHAPES, tests/test_small_iterates_gpu.py) are held to it on; tests/test_pcg_ref_cpu.py checks the
reference and the cases themselves.

pcg_iterates is the textbook Jacobi-PCG of oracle/fem.pcg_jacobi without a stopping test, in np.longdouble (64-bit mantissa) or
np.float64; the matrices are the assembled P1 matrices of oracle/fem.  The distance between the two precisions, per case and per
iterate, is the yardstick the device's iterates are measured with: no tolerance here comes from the device.  Plain numpy; no GPU
code is imported."""
from __future__ import annotations

from dataclasses import dataclass
from math import comb
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

from oracle import fem



class OpSet(NamedTuple):
    """(C_m, theta, dt) of A = C_m Mass + theta dt K and B = C_m Mass - (1 - theta) dt K: a property of a case, not of the module."""
    name: str
    c_m: float
    theta: float
    dt: float

    @property
    def triple(self) -> tuple:
        return (self.c_m, self.theta, self.dt)


# cn:   Crank-Nicolson, the operator of every case from before the sets had names: the factor of K in A equals the one in B, so a
#       theta written for 1 - theta, or the reverse, changes nothing there;
# be:   backward Euler: (1 - theta) dt = 0 exactly, B = C_m Mass, theta dt = dt -- which is why be alone cannot tell theta dt from dt;
# skew: C_m = 0.013, theta dt = 0.02, (1 - theta) dt = 0.06 and dt = 0.08 are four different numbers: every factor told from every other.
OPSETS = {"cn": OpSet("cn", 0.01, 0.5, 0.05), "be": OpSet("be", 0.01, 1.0, 0.05), "skew": OpSet("skew", 0.013, 0.25, 0.08)}
CN = OPSETS["cn"]
NEW_SETS = ("be", "skew")
_, C_M, THETA, DT = CN  # the default set, for the modules whose cases are not diffusion cases of this table
H = 0.1
STIM_AMPS = (0.3, -0.15)  # dt amp / C_m = 1.5 and -0.75: the stimuli move x by as much as the noise in v does
CUTS = (1, 2, 3, 7)       # max_it of the cut solves: the ring holds 6 directions, 7 = a full ring flush and a second cycle
GUESS_CUTS = (1, 3)
GUESS_ORDERS = (1, 3)
GUESS_SOLVES = 4          # converged solves (GUESS_RTOL) in front of a cut solve that starts from an extrapolated guess
GUESS_RTOL = 1e-11
RTOLS = (1e-6, 1e-9)
KMAX = 60                 # iterations of the reference: every case is converged far beyond 1e-9 there (asserted on the CPU)
FACTOR = 16.0             # device against longdouble <= FACTOR * (float64 against longdouble, or the floor)
U = 2.0**-53

# nodes (nx, ny, nz) -> dimension of the stencil tables
SHAPES = {
    (64, 4, 3): 3,      # one aligned segment, one row block at RY = 4
    (63, 5, 4): 3,      # the second segment of the iteration passes holds one node ...
    (65, 3, 5): 3,      # ... all of whose neighbours arrive through halo lanes
    (62, 3, 3): 3,      # the 62-node segments of the right-hand side
    (125, 4, 2): 3,
    (128, 2, 2): 3,     # a few rows and columns around the segment widths
    (127, 9, 3): 3,
    (129, 7, 6): 3,
    (130, 6, 9): 3,     # three segments
    (3, 70, 2): 3,      # many row blocks, ny % 4 = 2
    (2, 2, 2): 3,       # degenerate boxes
    (1, 1, 7): 3,
    (257, 5, 1): 2,     # one plane
    (64, 1, 1): 1,      # one row
    (65, 1, 1): 1,
}
# The one-launch solve (pcg_small_kernel<M> of csrc/beat_pde_small.hip: 512 threads, thread t owns nodes t, t + 512, ...; M = 2, 4,
# 6, 8, 10, 12 or 16 register slots per thread; the search direction in LDS between two zero margins of about a plane).  Kept apart
# from SHAPES, which drives every child process of the register-row test.
SMALL_SHAPES = {
    (128, 2, 2): 3,     # <2>: 512 nodes, one per thread, slot j = 1 empty in every thread
    (3, 3, 57): 3,      # <2>: 513 nodes, one thread owns two
    (5, 5, 41): 3,      # <4>: 1025 nodes, the 2 -> 4 switch
    (64, 32, 1): 2,     # <4> full, one plane (a margin of about n)
    (43, 9, 7): 3,      # <6>
    (16, 16, 16): 3,    # <8> full
    (41, 15, 7): 3,     # <10>: the Niederer slab at dx = 0.5 mm, which the kernel was written for
    (129, 7, 6): 3,     # <12>
    (130, 6, 9): 3,     # <16>: 7020 nodes, slots 14 and 15 empty in every thread
    (32, 16, 16): 3,    # <16> full: the size limit
    (2, 2, 2048): 3,    # <16> full, the smallest plane
    (64, 94, 1): 2,     # the largest LDS request taken (SMALL_LDS_LIMIT) ...
    (64, 95, 1): 2,     # ... and one row more: not taken
    (23, 1, 1): 1,      # fewer nodes than one wave
    (1, 1, 7): 3,       # an axis of one node IN FRONT of a longer one under tables of higher dimension: the flat LDS index of its
    (1, 5, 4): 3,       # neighbours (which are outside the box, with 'interior' coefficients that are not zero) is that of a node
    (6, 1, 5): 3,       # in the box, so the one-launch solve declines these (small_declines_collapsed) and the multi-launch
    (1, 9, 1): 3,       # kernels solve them
}
SMALL_GUESS_SHAPES = ((41, 15, 7), (129, 7, 6), (64, 32, 1), (32, 16, 16))
SMALL_THREADS, SMALL_MAX_PER_THREAD, SMALL_TABW, SMALL_LDS_LIMIT = 512, 16, 16, 150 * 1024
CHUNK_SHAPES = ((130, 6, 9), (129, 7, 6), (63, 5, 4), (1, 1, 7))  # every z-chunk length BEAT_RR_BLOCKS can ask for
GUESS_SHAPES = ((65, 3, 5), (129, 7, 6), (130, 6, 9), (257, 5, 1))
# The slab-decomposed solve (tests/test_dist_iterates_gpu.py): shape -> numbers of ranks.  beat._engine.Slab(nz, rank, world) deals
# the planes evenly, the first ranks take the extra one; tests/test_dist_cases_cpu.py holds what each line is there for to the tables.
DIST_CASES = {
    (64, 4, 3): (2, 3),        # one aligned segment; 2 + 1 planes; three one-plane slabs
    (63, 5, 4): (2, 4),        # second segment of one node; ny % 4 = 1
    (65, 3, 5): (2, 3, 5),     # halo-lane-only segment; 3 + 2, 2 + 2 + 1, five one-plane slabs
    (129, 7, 6): (2, 3),       # three segments; ny % 2 = 1
    (130, 6, 9): (2, 3, 4),    # three segments; 5 + 4, 3 + 3 + 3, 3 + 2 + 2 + 2
    (3, 70, 2): (2,),          # many row blocks; both slabs one plane, one ghost plane each
    (125, 4, 2): (2,),         # one-plane slabs
    (128, 2, 2): (2,),
    (2, 2, 2): (2,),           # the smallest box that can be cut
    (1, 1, 7): (2, 7),         # collapsed axes in front of z; seven one-node slabs
}
DIST_GUESS_CASES = (((65, 3, 5), 3), ((130, 6, 9), 2))  # (shape, world): the ghost plane of the guess increment travels with v_
DIST_RY4_MIN_NY = 4        # BEAT_RR_RY=4 runs on the shapes with at least one full block of four rows
# The cases off theta = 1/2: shape -> sets (tests/test_pcg_ref_cpu.py holds every pair to the conditions of a case).  skew on a 1-D row
# converges by iterate 7 (r_7 / ||b|| = 8.5e-14 on 64 x 1 x 1: no cut at 7), so the rows take be only.
OPSET_SHAPES = {(65, 3, 5): NEW_SETS, (129, 7, 6): NEW_SETS, (257, 5, 1): NEW_SETS, (64, 1, 1): ("be",)}   # the register-row children
OPSET_GUESS_SHAPES = ((65, 3, 5), (129, 7, 6))
SMALL_OPSET_SHAPES = {(41, 15, 7): NEW_SETS, (64, 32, 1): NEW_SETS, (1, 5, 4): NEW_SETS}  # one-launch; 1 x 5 x 4 is declined: multi-launch
SMALL_OPSET_GUESS_SHAPES = ((41, 15, 7), (64, 32, 1))
DIST_OPSET_CASES = {((65, 3, 5), 3): NEW_SETS, ((130, 6, 9), 2): NEW_SETS}  # (shape, world) of DIST_CASES; these are DIST_GUESS_CASES too
DIST_OPSET_GUESS = {((65, 3, 5), 3): ("skew",), ((130, 6, 9), 2): ("skew",)}
RETIME = ("cn", "skew", "cn")  # a live handle: GUESS_SOLVES solves with a guess of order 3 under cn, set_timestep(skew), the cuts; back
SEED_SHIFT: dict = {}  # shape -> added to its seed, should a seed put a stop within 1e-6 of its threshold (test_pcg_ref_cpu)


def all_shapes() -> list:
    """SHAPES, then what SMALL_SHAPES adds to them."""
    return list(SHAPES) + [s for s in SMALL_SHAPES if s not in SHAPES]


def opset(ops) -> OpSet:
    """An OpSet from its name or itself."""
    return ops if isinstance(ops, OpSet) else OPSETS[ops]


def opset_pairs() -> list:
    """Every (shape, set name) off cn that a constant-coefficient GPU test runs, each once."""
    pairs = []
    for table in (OPSET_SHAPES, SMALL_OPSET_SHAPES, {s: sets for (s, _), sets in DIST_OPSET_CASES.items()}):
        pairs += [(s, name) for s, sets in table.items() for name in sets if (s, name) not in pairs]
    return pairs


def case_key(shape, ops="cn") -> str:
    """shape_key for cn (the keys from before the sets had names do not change), shape@set otherwise."""
    name = opset(ops).name
    return shape_key(shape) if name == "cn" else f"{shape_key(shape)}@{name}"


def dim_of(shape) -> int:
    """The table dimension of a shape of either table (test_pcg_ref_cpu: a shape in both has one dimension)."""
    shape = tuple(shape)
    return SHAPES[shape] if shape in SHAPES else SMALL_SHAPES[shape]


def small_lds_bytes(shape) -> int:
    """The dynamic LDS the one-launch solve asks for (small_lds_bytes and small_margin of csrc/beat_pde_small.hip, written out):
    two (27, TABW) tables, 6 x 8 reduction partials, 32 slots of 1 / diag, and n doubles between two margins of plane + nx + 1
    rounded up to 8."""
    nx, ny, nz = shape
    margin = (nx * ny + nx + 1 + 7) // 8 * 8
    return 8 * (2 * 27 * SMALL_TABW + 6 * (SMALL_THREADS // 64) + 32 + nx * ny * nz + 2 * margin)


def small_declines_collapsed(shape) -> bool:
    """beat_small_available's rule for an axis of one node in front of a longer one."""
    nx, ny, nz = shape
    return (nx == 1 and nx * ny * nz > 1) or (ny == 1 and nz > 1)


def small_takes(shape) -> bool:
    """Whether beat_small_available takes a constant-coefficient Jacobi operator of this shape on one slab."""
    n = int(np.prod(shape))
    return n <= SMALL_THREADS * SMALL_MAX_PER_THREAD and small_lds_bytes(shape) <= SMALL_LDS_LIMIT and not small_declines_collapsed(shape)


def small_instance(shape) -> int:
    """M of the pcg_small_kernel<M> beat_small_launch picks."""
    per_thread = -(-int(np.prod(shape)) // SMALL_THREADS)
    return next(m for m in (2, 4, 6, 8, 10, 12, 16) if per_thread <= m)


def shape_key(shape) -> str:
    return "x".join(str(int(s)) for s in shape)


def seed_of(shape) -> int:
    nx, ny, nz = shape
    return 1_000_003 * nx + 1_009 * ny + nz + SEED_SHIFT.get(tuple(shape), 0)


def conductivity(dim: int):
    """3-D: the fibre tensor of the suite's "aniso3"; 2-D / 1-D: off-diagonal / scalar of the same size."""
    if dim == 3:
        f0 = np.array([np.cos(np.pi / 6), np.sin(np.pi / 6), 0.0])
        return 9.5e-4 * np.outer(f0, f0) + 1.25e-4 * (np.eye(3) - np.outer(f0, f0))
    if dim == 2:
        return 1e-3 * np.array([[2.0, 0.3], [0.3, 1.0]])
    return 1e-3


def _centred(rng, n):
    v = rng.standard_normal(n)
    return v - v.mean()


def field(shape, j: int = 0) -> np.ndarray:
    """v of solve j of the shape's sequence.  j = 0: white noise of zero mean (the first iterations move x by O(1): an error in a
    step length shows in full; a field centred at -85 would hide it under ulp(85)).  j >= 1: the same noise plus two more noise
    fields whose weights move between solves, neither linearly nor slowly (an extrapolated guess stays O(1) wrong)."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed_of(shape))
    v0, w1, w2 = _centred(rng, n), _centred(rng, n), _centred(rng, n)
    if j == 0:
        return v0
    return v0 + np.sin(0.9 * j) * w1 + np.cos(1.7 * j) * w2


class Csr:
    """The three arrays of a CSR matrix whose data may be longdouble (scipy's matrices cannot hold it)."""

    def __init__(self, data, indices, indptr):
        self.data, self.indices, self.indptr = data, indices, indptr


@dataclass
class Problem:
    shape: tuple
    dim: int
    mass_tab: np.ndarray      # the (27, 15) tables the device is given ...
    stiff_tab: np.ndarray
    mass: sp.csr_matrix       # ... and the same numbers as matrices: one pattern, rows sorted, no empty row
    stiff: sp.csr_matrix
    A: sp.csr_matrix          # C_m Mass + theta dt K formed in float64
    weights: list             # two stimulus weight vectors (float64)
    n: int
    ops: OpSet = CN           # the (C_m, theta, dt) A was formed with and the right-hand side is formed with

    def with_ops(self, ops) -> "Problem":
        """The same matrices, tables and stimuli under another set."""
        ops = opset(ops)
        A = sp.csr_matrix((ops.c_m * self.mass.data + ops.theta * ops.dt * self.stiff.data, self.mass.indices, self.mass.indptr), shape=self.mass.shape)
        return Problem(self.shape, self.dim, self.mass_tab, self.stiff_tab, self.mass, self.stiff, A, self.weights, self.n, ops)

    def rhs_float64(self, v: np.ndarray) -> np.ndarray:
        """b in float64, the expression of rhs_longdouble written out again (the CPU tests hold the two together)."""
        o = self.ops
        return o.c_m * (self.mass @ v) - (1 - o.theta) * o.dt * (self.stiff @ v) + o.dt * sum(a * w for a, w in zip(STIM_AMPS, self.weights))

    def operator(self, dtype):
        """A = C_m Mass + theta dt K formed in ``dtype`` from the float64 entries of Mass and K."""
        if dtype is np.float64:
            return self.A
        L, o = np.longdouble, self.ops
        return Csr(L(o.c_m) * self.mass.data.astype(L) + L(o.theta) * L(o.dt) * self.stiff.data.astype(L), self.mass.indices, self.mass.indptr)

    def diagonal(self, dtype) -> np.ndarray:
        """diag A formed in ``dtype``, as operator forms A."""
        o = self.ops
        return dtype(o.c_m) * self.mass.diagonal().astype(dtype) + dtype(o.theta) * dtype(o.dt) * self.stiff.diagonal().astype(dtype)


_problems: dict = {}
_tables: dict = {}


def tables(dim: int):
    """(mass_tab, stiff_tab) per node type, by oracle/fem's literal element assembly (assemble_mass, assemble_stiffness on a mesh of
    two cells per axis).  The device is given THESE tables and the host their expansion: the same float64 numbers on both sides.
    (Matrices assembled on the whole mesh differ from them in the last digits, from node to node -- 0.1 is no dyadic spacing --
    and x = A^-1 b moves by ~20 ulp with them, which has nothing to do with the kernels; test_pcg_ref_cpu compares the two.)"""
    if dim not in _tables:  # (C_m and theta dt are not folded into the tables: one pair of tables serves every set)
        _tables[dim] = fem.stencil_table(dim, (H,) * dim, conductivity(dim), CN.c_m, CN.theta * CN.dt)
    return _tables[dim]


def expand(tab: np.ndarray, shape) -> sp.csr_matrix:
    """The matrix fem.apply_stencil(tab, shape, .) applies: all 15 offsets that stay inside the box, zero entries kept (one pattern
    for every table); an axis of one node is 'interior' with its neighbours outside the box."""
    nx, ny, nz = shape
    n = nx * ny * nz
    typ = fem.node_types(shape)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    rows, cols, vals = [], [], []
    for k, (ox, oy, oz) in enumerate(fem.STENCIL_OFFSETS):
        jx, jy, jz = ix + ox, iy + oy, iz + oz
        ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny) & (jz >= 0) & (jz < nz)
        rows.append(np.nonzero(ok)[0])
        cols.append((jx + nx * (jy + ny * jz))[ok])
        vals.append(tab[typ[ok], k])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    m = sp.csr_matrix((vals[order], cols[order], indptr), shape=(n, n))
    assert m.has_sorted_indices and (np.diff(m.indptr) > 0).all()
    return m


def assembled(shape):
    """(Mass, K, stimulus weights) assembled on the whole mesh.  An axis of one node under tables of higher dimension (the
    degenerate boxes) is what the kernels make of it: the node is 'interior' along that axis and its neighbours there are not in
    the box -- the principal submatrix, on the centre nodes, of the matrices of a mesh with three nodes along that axis."""
    dim = dim_of(shape)
    assert all(s == 1 for s in shape[dim:])
    nodes = shape[:dim]
    mesh_nodes = tuple(3 if m == 1 else m for m in nodes)
    mesh = fem.BoxMesh(tuple(m - 1 for m in mesh_nodes), tuple(H * (m - 1) for m in mesh_nodes))
    idx = np.meshgrid(*[np.arange(m) if m == k else np.array([1]) for m, k in zip(nodes[::-1], mesh_nodes[::-1])], indexing="ij")[::-1]
    keep, stride = np.zeros(idx[0].shape, dtype=np.int64), 1
    for a in range(dim):
        keep = keep + stride * idx[a]
        stride *= mesh_nodes[a]
    keep = keep.ravel()  # x fastest, as the device numbers its nodes
    sub = lambda m: m.tocsr()[keep][:, keep].tocsr()  # noqa: E731
    nc = len(mesh.cells)
    sets = (np.arange(nc)[: max(1, nc // 3)], np.arange(nc)[nc // 2:][1::3] if nc >= 6 else np.arange(nc)[-1:])
    weights = [fem.stimulus_weights(mesh, c)[keep] for c in sets]
    return sub(fem.assemble_mass(mesh)), sub(fem.assemble_stiffness(mesh, conductivity(dim))), weights


def problem(shape, ops="cn") -> Problem:
    shape, ops = tuple(int(s) for s in shape), opset(ops)
    if ops != CN:
        if (shape, ops) not in _problems:
            _problems[(shape, ops)] = problem(shape).with_ops(ops)
        return _problems[(shape, ops)]
    if shape in _problems:
        return _problems[shape]
    dim = dim_of(shape)
    mt, kt = tables(dim)
    mass, stiff = expand(mt, shape), expand(kt, shape)
    assert np.array_equal(mass.indices, stiff.indices) and np.array_equal(mass.indptr, stiff.indptr)
    A = sp.csr_matrix((CN.c_m * mass.data + CN.theta * CN.dt * stiff.data, mass.indices, mass.indptr), shape=mass.shape)
    p = Problem(shape, dim, mt, kt, mass, stiff, A, assembled(shape)[2], mass.shape[0], CN)
    assert p.n == int(np.prod(shape))
    _problems[shape] = p
    return p


def matvec(m, x: np.ndarray, dtype) -> np.ndarray:
    """m @ x with products and sums in ``dtype`` (scipy does not multiply in longdouble); m has no empty row."""
    return np.add.reduceat(m.data.astype(dtype) * x[m.indices], m.indptr[:-1])


def rhs_longdouble(p: Problem, v: np.ndarray) -> np.ndarray:
    """b = (C_m Mass - (1 - theta) dt K) v + dt sum amp_j w_j, in longdouble, under the problem's set."""
    L = np.longdouble
    C_M, THETA, DT = p.ops.triple
    assert np.finfo(L).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"
    vl = v.astype(L)
    b = L(C_M) * matvec(p.mass, vl, L) - (L(1) - L(THETA)) * L(DT) * matvec(p.stiff, vl, L)
    for amp, w in zip(STIM_AMPS, p.weights):
        b = b + L(DT) * L(amp) * w.astype(L)
    return b


def guess_increment(order: int, increments) -> np.ndarray:
    """e = sum_{i=1..m} (-1)^(i+1) C(m, i) d_i in longdouble; increments[0] = d_1 is the latest (the header of csrc/beat_guess.h)."""
    L = np.longdouble
    m = min(order, len(increments))
    e = np.zeros(len(increments[0]), dtype=L)
    for i in range(1, m + 1):
        e = e + L((-1) ** (i + 1) * comb(m, i)) * increments[i - 1].astype(L)
    return e


def slab_counts(nz: int, world: int) -> list:
    """Planes per rank as beat._engine.Slab deals them without weights (tests/test_dist_cases_cpu.py holds the two together)."""
    base, extra = divmod(nz, world)
    return [base + (1 if r < extra else 0) for r in range(world)]


def slab_dot(bounds):
    """a . b summed slab by slab (entries [bounds[r], bounds[r + 1]) are rank r's) and the slabs in rank order: the order the
    decomposed solve reduces in."""
    def dot(a, b):
        total = a[bounds[0]:bounds[1]] @ b[bounds[0]:bounds[1]]
        for lo, hi in zip(bounds[1:-1], bounds[2:]):
            total = total + a[lo:hi] @ b[lo:hi]
        return total
    return dot


def pcg_iterates(A, b, x0, dinv, kmax: int, dtype, dot=None):
    """Jacobi-PCG (oracle/fem.pcg_jacobi) in ``dtype`` (np.longdouble or np.float64) without a stopping test:
    ([x_1 .. x_kmax], [||r_1|| .. ||r_kmax||] of the recurrence residual, ||b||).  The single-reduction form of the decomposed
    solve computes the same iterates in exact arithmetic (Chronopoulos & Gear), so this serves it too.  ``dot``: the dot product
    (default a @ b; slab_dot for the summation order of a decomposition)."""
    if dot is None:
        dot = lambda a, b: a @ b  # noqa: E731
    if dtype is np.longdouble:
        assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"
    else:
        assert dtype is np.float64
    b, x, dinv = np.asarray(b).astype(dtype), np.asarray(x0).astype(dtype), np.asarray(dinv).astype(dtype)
    r = b - matvec(A, x, dtype)
    z = dinv * r
    p = z.copy()
    rz = dot(r, z)
    xs, rnorms = [], []
    for _ in range(kmax):
        q = matvec(A, p, dtype)
        alpha = rz / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        z = dinv * r
        rz_new = dot(r, z)
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        xs.append(x)
        rnorms.append(np.sqrt(dot(r, r)))
    return xs, rnorms, np.sqrt(dot(b, b))


@dataclass
class Reference:
    """Both host runs of one system: x[k], r[k] for k = 1..kmax (index 0 unused), in longdouble (L) and float64 (D)."""
    xL: list
    xD: list
    rL: list
    rD: list
    bL: np.longdouble
    bD: float
    kmax: int

    def stop(self, rtol: float) -> int:
        """The first k with ||r_k|| <= rtol ||b|| of the longdouble run."""
        for k in range(1, self.kmax + 1):
            if self.rL[k] <= np.longdouble(rtol) * self.bL:
                return k
        raise AssertionError(f"not converged to {rtol} within {self.kmax} iterations")

    def delta(self, k: int) -> float:
        return float(np.abs(self.xD[k].astype(np.longdouble) - self.xL[k]).max())

    def x_floor(self, k: int) -> float:
        return float(2.0 * U * np.abs(self.xL[k]).max())

    def x_bound(self, k: int) -> float:
        return FACTOR * max(self.delta(k), self.x_floor(k))

    def x_error(self, k: int, x_dev: np.ndarray) -> float:
        return float(np.abs(x_dev.astype(np.longdouble) - self.xL[k]).max())

    def rhs_norm_bound(self) -> float:
        return FACTOR * max(abs(float(np.longdouble(self.bD) - self.bL)), 4 * 2 * U * float(self.bL))

    def residual_bound(self, k: int) -> float:
        """16 max(float64 deviation, 4 ulp) and the absolute floor 16 k 2^-53 ||b||: a recurrence residual loses relative accuracy
        as it shrinks."""
        dev = abs(float(np.longdouble(self.rD[k]) - self.rL[k]))
        return FACTOR * max(dev, 4 * 2 * U * float(self.rL[k])) + FACTOR * k * U * float(self.bL)


def reference(p: Problem, bL: np.ndarray, x0L: np.ndarray, kmax: int) -> Reference:
    """x0L, bL in longdouble; the float64 run starts from their roundings."""
    L, D = np.longdouble, np.float64
    AL = p.operator(L)
    diag = p.mass.diagonal() != 0  # (position of the diagonal in the shared pattern)
    at = np.nonzero(p.mass.indices == np.repeat(np.arange(p.n), np.diff(p.mass.indptr)))[0]
    assert diag.all() and len(at) == p.n
    xL, rL, bnL = pcg_iterates(AL, bL, x0L, L(1) / AL.data[at], kmax, L)
    xD, rD, bnD = pcg_iterates(p.A, bL.astype(D), x0L.astype(D), 1.0 / p.A.data[at], kmax, D)
    return Reference([None] + xL, [None] + xD, [None] + rL, [None] + rD, bnL, float(bnD), kmax)


def kmax_of(shape) -> int:
    """KMAX, or the number of unknowns where that is smaller: CG ends there (the residual of the next step is 0 / 0)."""
    return min(KMAX, int(np.prod(shape)))


_plain: dict = {}


def plain_reference(shape, ops="cn") -> Reference:
    """The solve from x0 = v = field(shape), kmax_of(shape) iterations; computed once per shape and set."""
    key = (tuple(shape), opset(ops))
    if key not in _plain:
        p, v = problem(*key), field(shape)
        _plain[key] = reference(p, rhs_longdouble(p, v), v.astype(np.longdouble), kmax_of(shape))
    return _plain[key]
