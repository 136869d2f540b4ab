"""Where every node's cell states live, as a rows plan takes it (include/beat_hip.h: beat_rows_plan_create): a class byte per node of
the grid, a position per node (or none: the arrays span the grid) and the size of every class's array.  ``DolfinMultiODESolver``
keeps its states in one of three layouts; one function per layout turns what the solver already holds into those arguments.  NumPy
only: nothing here needs a device.

Class bytes at or above the number of classes have no source: ``NO_MODEL`` (255) is a tissue node without a cell model, ``PADDING``
(254) an entry of the compact array that is no node at all."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

MAX_CLASSES = 32  # BEAT_MAX_CLASSES
NO_MODEL = 255
PADDING = 254
_LIMIT = 2**31


class RowsLayout(NamedTuple):
    cls: np.ndarray          # uint8[n]: the node's class, or NO_MODEL
    pos: np.ndarray | None   # int32[n]: the node's column in its class's array; None: column = node
    class_n: tuple           # columns of every class's array
    class_rows: tuple        # rows (states) of every class's array


def check_sizes(n, class_n) -> None:
    """The plan holds 32-bit positions: the grid and every class's array must be smaller than 2^31."""
    if not 0 <= int(n) < _LIMIT:
        raise ValueError(f"a grid of {int(n)} nodes does not fit 32-bit positions (below 2^31)")
    if not 1 <= len(class_n) <= MAX_CLASSES:
        raise ValueError(f"1..{MAX_CLASSES} classes expected, got {len(class_n)}")
    for c, m in enumerate(class_n):
        if not 0 <= int(m) < _LIMIT:
            raise ValueError(f"class {c}: an array of {int(m)} columns does not fit 32-bit positions (below 2^31)")


def _rows(class_rows, k):
    rows = (int(class_rows),) * k if np.ndim(class_rows) == 0 else tuple(int(r) for r in class_rows)
    if len(rows) != k or any(r < 1 for r in rows):
        raise ValueError(f"one positive row count per class ({k}) expected, got {class_rows!r}")
    return rows


def grid_layout(cls_full, num_classes, class_rows) -> RowsLayout:
    """One (S, n) array over the grid and a class byte per node (``cls_full``, NO_MODEL where no marker applies): every class shares
    the array, a node's column is the node."""
    cls = np.ascontiguousarray(cls_full, dtype=np.uint8)
    n = cls.size
    check_sizes(n, (n,) * int(num_classes))
    return RowsLayout(cls, None, (n,) * int(num_classes), _rows(class_rows, int(num_classes)))


def compact_layout(n, node_idx, cls, num_classes, class_rows) -> RowsLayout:
    """One compact (S, n_c) array: entry e is node ``node_idx[e]`` with class ``cls[e]`` -- whole runs per class, PADDING entries
    between them (their node index means nothing), NO_MODEL entries for tissue without a model.  Only entries with a class below
    ``num_classes`` are sources; no position points at any other.  Every class shares the array: class_n = n_c for all."""
    node_idx, cls = np.asarray(node_idx), np.asarray(cls, dtype=np.uint8)
    if node_idx.shape != cls.shape or node_idx.ndim != 1:
        raise ValueError(f"node_idx {node_idx.shape} and cls {cls.shape}: one entry each per column of the compact array expected")
    k, n_c = int(num_classes), int(cls.size)
    check_sizes(n, (n_c,) * k)
    entries = np.nonzero(cls < k)[0]
    nodes = node_idx[entries].astype(np.int64)
    _check_nodes(nodes, int(n))
    grid_cls = np.full(int(n), NO_MODEL, dtype=np.uint8)
    pos = np.zeros(int(n), dtype=np.int32)
    grid_cls[nodes] = cls[entries]
    pos[nodes] = entries
    return RowsLayout(grid_cls, pos, (n_c,) * k, _rows(class_rows, k))


def marker_layout(n, index_lists, class_rows, class_n=None) -> RowsLayout:
    """One array per marker: ``index_lists[c]`` holds the nodes of class c in the order of its array's columns.  ``class_n``: the
    columns of every array when it has more than its list (default: the list's length)."""
    k = len(index_lists)
    lists = [np.asarray(ix).astype(np.int64).ravel() for ix in index_lists]
    class_n = tuple(int(ix.size) for ix in lists) if class_n is None else tuple(int(m) for m in class_n)
    if len(class_n) != k:
        raise ValueError(f"{k} index lists, {len(class_n)} sizes")
    check_sizes(n, class_n)
    for c, ix in enumerate(lists):
        if ix.size > class_n[c]:
            raise ValueError(f"class {c}: position {class_n[c]} is outside its array of {class_n[c]} columns ({ix.size} nodes listed)")
    _check_nodes(np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64), int(n))
    grid_cls = np.full(int(n), NO_MODEL, dtype=np.uint8)
    pos = np.zeros(int(n), dtype=np.int32)
    for c, ix in enumerate(lists):
        grid_cls[ix] = c
        pos[ix] = np.arange(ix.size, dtype=np.int32)
    return RowsLayout(grid_cls, pos, class_n, _rows(class_rows, k))


def _check_nodes(nodes, n) -> None:
    if nodes.size and (nodes.min() < 0 or nodes.max() >= n):
        bad = nodes[(nodes < 0) | (nodes >= n)][0]
        raise ValueError(f"node {int(bad)} is outside the grid of {n} nodes")
    uniq, counts = np.unique(nodes, return_counts=True)
    if (counts > 1).any():
        raise ValueError(f"node {int(uniq[counts > 1][0])} is claimed twice")

