"""Shared by the tests of the rows plan (test_rows_layout_cpu.py, test_rows_host_cpu.py, test_rows_gpu.py): marker patterns on small
boxes, the arrays DolfinMultiODESolver would hold for them, a brute-force statement of which source element a node has, and the
expand / collapse of whole arrays in NumPy.  Every value is a copy: comparisons are exact."""
from dataclasses import dataclass

import numpy as np

OUTSIDE = 9  # a marker value that init_states does not list


def markers(shape, pattern, seed=0):
    """A marker per node of a box of ``shape`` = (nx, ny, nz) nodes, x fastest: values 0, 1, 2 or OUTSIDE."""
    nx, ny, nz = shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    if pattern in ("checker", "checker_holes"):
        m = (ix + iy + iz) % 3  # every wave of 64 nodes holds all three
        if pattern == "checker_holes":
            m = m.copy()
            m[np.random.default_rng(seed).random(m.size) < 0.1] = OUTSIDE
    elif pattern == "thirds":
        m = np.minimum(ix * 3 // nx, 2)
    elif pattern == "runs":  # runs of 37 nodes, every fourth run without a model
        run = np.arange(ix.size) // 37
        m = np.where(run % 4 == 3, OUTSIDE, run % 4)
    else:
        raise ValueError(pattern)
    return m.astype(np.int64)


def cls_full(marker_arr, values=(0, 1, 2)):
    cls = np.full(marker_arr.size, 255, dtype=np.uint8)
    for k, v in enumerate(values):
        cls[marker_arr == v] = k
    return cls


def compact_arrays(cls, k, tile=256):
    """node_idx and cls of the compact array as DolfinMultiODESolver._setup_one_launch lays it out: a run of whole tiles per class,
    then the nodes without a model (class 255); padding entries carry class 254 and node 0."""
    runs = [(c, np.nonzero(cls == c)[0]) for c in range(k)] + [(255, np.nonzero(cls == 255)[0])]
    nodes, classes = [], []
    for c, idx in runs:
        pad = (-idx.size) % tile
        nodes += [idx, np.zeros(pad, dtype=np.int64)]
        classes += [np.full(idx.size, c, dtype=np.uint8), np.full(pad, 254, dtype=np.uint8)]
    return np.concatenate(nodes), np.concatenate(classes)


def index_lists(cls, k):
    return [np.nonzero(cls == c)[0] for c in range(k)]


def brute_force(n, claims):
    """``claims``: (class, node, position) triples.  (cls uint8[n], pos int64[n]) by a plain loop; a node claimed twice is an error."""
    cls, pos = np.full(n, 255, dtype=np.uint8), np.zeros(n, dtype=np.int64)
    for c, node, p in claims:
        assert cls[node] == 255, node
        cls[node], pos[node] = c, p
    return cls, pos


@dataclass
class Problem:
    """Sources in one arena of doubles: class c has ``rows[c]`` rows of ``cn[c]`` doubles, ``ld[c]`` apart from element ``base[c]``."""
    n: int
    cls: np.ndarray
    pos: np.ndarray | None
    base: list
    ld: list
    cn: list
    rows: list
    arena: int

    @property
    def k(self):
        return len(self.base)

    def element(self, c, r, p):
        return self.base[c] + r * self.ld[c] + p


def shared_problem(layout, S=5, pad=7, lead=3):
    """Every class shares one (S, class_n) array (the grid-spanning and the compact layout), rows ``class_n + pad`` apart."""
    k, cn = len(layout.class_n), int(layout.class_n[0])
    ld = cn + pad
    return Problem(layout.cls.size, layout.cls, layout.pos, [lead] * k, [ld] * k, [cn] * k, [S] * k, lead + S * ld + 5)


def separate_problem(layout, S=(4, 6, 5), lead=2):
    """One array per class with its own base, leading dimension and number of rows (the per-marker layout)."""
    base, ld, off = [], [], lead
    for c, m in enumerate(layout.class_n):
        base.append(off)
        ld.append(int(m) + 3 + 2 * c)
        off += S[c] * ld[-1] + 4
    return Problem(layout.cls.size, layout.cls, layout.pos, base, ld, [int(m) for m in layout.class_n], list(S[: len(base)]), off + 3)


def source_elements(pb, rows_f):
    """Element of the arena per node for a field whose row in class c is ``rows_f[c]``, -1 without a source.  A plain loop."""
    out = np.full(pb.n, -1, dtype=np.int64)
    for i in range(pb.n):
        c = int(pb.cls[i])
        if c >= pb.k:
            continue
        p = i if pb.pos is None else int(pb.pos[i])
        if 0 <= p < pb.cn[c]:
            out[i] = pb.element(c, rows_f[c], p)
    return out


def expand_ref(pb, arena, rows, prior, fill=None):
    """rows[f][c]; prior[f]: what the outputs held.  KEEP with ``fill`` None."""
    outs = []
    for f, rows_f in enumerate(rows):
        e = source_elements(pb, rows_f)
        out = np.array(prior[f], dtype=np.float64)
        if fill is not None:
            out[:] = fill
        out[e >= 0] = arena[e[e >= 0]]
        outs.append(out)
    return outs


def collapse_ref(pb, arena, rows, fields):
    arena = arena.copy()
    for f, rows_f in enumerate(rows):
        e = source_elements(pb, rows_f)
        arena[e[e >= 0]] = np.asarray(fields[f])[e >= 0]
    return arena


def pick_rows(pb, nfields, seed=0):
    """Distinct rows per class for every field (so that collapse is allowed), different from class to class."""
    assert nfields <= min(pb.rows)
    rng = np.random.default_rng(seed)
    per_class = [rng.permutation(pb.rows[c]) for c in range(pb.k)]
    return [[int(per_class[c][f % pb.rows[c]]) for c in range(pb.k)] for f in range(nfields)]
