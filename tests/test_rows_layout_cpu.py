"""beat._rows_layout: the three layouts DolfinMultiODESolver keeps its states in, as (class byte, position) per node of the grid,
against a brute-force loop."""
import numpy as np
import pytest

import _rows_cases as cases
from beat import _rows_layout as rl

SHAPE = (6, 5, 4)
N = 6 * 5 * 4
PATTERNS = ("checker", "checker_holes", "thirds")


def _cls(pattern):
    return cases.cls_full(cases.markers(SHAPE, pattern))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_grid_layout(pattern):
    cls = _cls(pattern)
    lay = rl.grid_layout(cls, 3, 19)
    want_cls, want_pos = cases.brute_force(N, [(int(c), i, i) for i, c in enumerate(cls) if c < 3])
    assert lay.pos is None and lay.cls.dtype == np.uint8
    np.testing.assert_array_equal(lay.cls, want_cls)
    assert lay.class_n == (N, N, N) and lay.class_rows == (19, 19, 19)
    if pattern == "checker_holes":
        assert 0 < (lay.cls == rl.NO_MODEL).sum() < N // 4  # (about a tenth of the nodes carry the other marker)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_marker_layout(pattern):
    cls = _cls(pattern)
    lists = cases.index_lists(cls, 3)
    lay = rl.marker_layout(N, lists, (19, 4, 7))
    want_cls, want_pos = cases.brute_force(N, [(c, int(node), p) for c, ix in enumerate(lists) for p, node in enumerate(ix)])
    np.testing.assert_array_equal(lay.cls, want_cls)
    assert lay.pos.dtype == np.int32
    np.testing.assert_array_equal(lay.pos[want_cls != 255], want_pos[want_cls != 255])
    assert lay.class_n == tuple(len(ix) for ix in lists) and lay.class_rows == (19, 4, 7)
    # a boolean mask per marker, as the solver's _inds holds them, is the same thing as its nonzero()
    same = rl.marker_layout(N, [np.nonzero(cls == c)[0] for c in range(3)], 19)
    np.testing.assert_array_equal(same.pos, lay.pos)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_compact_layout(pattern):
    cls = _cls(pattern)
    node_idx, ccls = cases.compact_arrays(cls, 3)
    assert (ccls == rl.PADDING).any() and ccls.size % 256 == 0
    lay = rl.compact_layout(N, node_idx, ccls, 3, 19)
    want_cls, want_pos = cases.brute_force(N, [(int(c), int(node), e) for e, (node, c) in enumerate(zip(node_idx, ccls)) if c < 3])
    np.testing.assert_array_equal(lay.cls, want_cls)
    np.testing.assert_array_equal(lay.cls, cls)  # (class-255 entries of the array give no source: the node stays 255)
    marked = want_cls != 255
    np.testing.assert_array_equal(lay.pos[marked], want_pos[marked])
    # no position points at a padding entry or at an entry without a model
    assert (ccls[lay.pos[marked]] < 3).all()
    assert not np.isin(np.nonzero(ccls >= 3)[0], lay.pos[marked]).any()
    assert lay.class_n == (ccls.size,) * 3  # every class shares the one array


def test_refusals():
    cls = _cls("thirds")
    lists = cases.index_lists(cls, 3)
    twice = [lists[0], np.append(lists[1], lists[0][2]), lists[2]]
    with pytest.raises(ValueError, match="claimed twice"):
        rl.marker_layout(N, twice, 19)
    node_idx, ccls = cases.compact_arrays(cls, 3)
    node_idx = node_idx.copy()
    node_idx[1] = node_idx[0]
    with pytest.raises(ValueError, match="claimed twice"):
        rl.compact_layout(N, node_idx, ccls, 3, 19)
    with pytest.raises(ValueError, match="outside its array"):  # a position at or past its class's n
        rl.marker_layout(N, lists, 19, class_n=(len(lists[0]), len(lists[1]) - 1, len(lists[2])))
    with pytest.raises(ValueError, match="outside the grid"):
        rl.marker_layout(N, [np.array([0, N])], 19)
    # sizes that do not fit int32, given as sizes
    with pytest.raises(ValueError, match="2\\^31"):
        rl.check_sizes(2**31, (5,))
    with pytest.raises(ValueError, match="2\\^31"):
        rl.check_sizes(100, (5, 2**31))
    rl.check_sizes(2**31 - 1, (2**31 - 1,))
    with pytest.raises(ValueError, match="2\\^31"):
        rl.compact_layout(2**31, np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.uint8), 1, 19)
    with pytest.raises(ValueError, match="2\\^31"):
        rl.marker_layout(N, lists, 19, class_n=(2**31, 50, 50))
    with pytest.raises(ValueError, match="classes"):
        rl.check_sizes(10, (1,) * 33)
    with pytest.raises(ValueError, match="classes"):
        rl.check_sizes(10, ())
