"""The cases tests/test_dist_iterates_gpu.py runs the slab-decomposed solve on (DIST_CASES of tests/_pcg_ref.py and tests/_var_ref.py),
held to what their tables say they are there for -- from the masks and from beat._engine.Slab, no GPU code imported -- and the
bound of tests/_pcg_check.py shown to admit a decomposition as such: a float64 host PCG whose three dot products are summed slab by
slab and the slabs in rank order (the order the thread world of tests/_thread_world.py reduces in) passes Check.cut at every cut and
Check.uncut at every stop against the longdouble run, for every (case, world).  A device that misses the bound there is wrong, not
reordered.

Measured here (the bound is 16): the worst err / max(delta_k, 2^-52 max|x|) of the slab-ordered float64 run is 1.84 with constant
coefficients (2 x 2 x 2 on 2 ranks, k = 1) and 2.16 with per-node rows (62 x 9 x 5 full on 5 ranks, k = 1); the norms reach 0.51
(65 x 3 x 5 on 2 ranks, k = 1) and 0.36 (2 x 2 x 2 full on 2 ranks, k = 1) of their yardstick.  Every stop is the longdouble run's.
No seed had to be moved (both SEED_SHIFT tables stay empty)."""
import numpy as np
import pytest

import _pcg_ref as ref
import _var_ref as vr
from _pcg_check import Check

CONST = [(s, w) for s, worlds in ref.DIST_CASES.items() for w in worlds]
VAR = [(c, w) for c, worlds in vr.DIST_CASES for w in worlds]
# the worlds off theta = 1/2: (shape or case, world, set)
CONST_SETS = [(s, w, name) for (s, w), sets in ref.DIST_OPSET_CASES.items() for name in sets]
VAR_SETS = [(c, w, name) for (c, w), sets in vr.DIST_OPSET_CASES.items() for name in sets] + \
    [(c, w, name) for (c, w), sets in vr.DIST_OPSET_GUESS.items() for name in sets if (c, w) not in vr.DIST_OPSET_CASES]
# planes per rank the tables claim
COUNTS = {
    ((64, 4, 3), 2): (2, 1), ((64, 4, 3), 3): (1, 1, 1),
    ((63, 5, 4), 2): (2, 2), ((63, 5, 4), 4): (1, 1, 1, 1),
    ((65, 3, 5), 2): (3, 2), ((65, 3, 5), 3): (2, 2, 1), ((65, 3, 5), 5): (1, 1, 1, 1, 1),
    ((129, 7, 6), 2): (3, 3), ((129, 7, 6), 3): (2, 2, 2),
    ((130, 6, 9), 2): (5, 4), ((130, 6, 9), 3): (3, 3, 3), ((130, 6, 9), 4): (3, 2, 2, 2),
    ((3, 70, 2), 2): (1, 1), ((125, 4, 2), 2): (1, 1), ((128, 2, 2), 2): (1, 1), ((2, 2, 2), 2): (1, 1),
    ((1, 1, 7), 2): (4, 3), ((1, 1, 7), 7): (1,) * 7,
    ((125, 18, 20), 2): (10, 10), ((125, 18, 20), 3): (7, 7, 6), ((125, 18, 20), 4): (5, 5, 5, 5),
    ((63, 16, 6), 2): (3, 3), ((63, 16, 6), 3): (2, 2, 2), ((63, 16, 6), 6): (1,) * 6,
    ((62, 9, 5), 2): (3, 2), ((62, 9, 5), 5): (1,) * 5,
    ((3, 70, 3), 3): (1, 1, 1),
    ((6, 4, 71), 2): (36, 35), ((6, 4, 71), 8): (9, 9, 9, 9, 9, 9, 9, 8),
    ((2, 2, 2), 2): (1, 1),
}


def slabs(nz, world):
    from beat._engine import Slab

    return [Slab(nz, r, world) for r in range(world)]


def test_tables_are_consistent():
    assert set(ref.DIST_CASES) <= set(ref.SHAPES) and all(ref.SHAPES[s] == 3 for s in ref.DIST_CASES)
    assert all(c in vr.CASES and vr.SHAPES[c[0]] == 3 for c, _ in vr.DIST_CASES) and len({c for c, _ in vr.DIST_CASES}) == len(vr.DIST_CASES)
    for shape, world in CONST + [(c[0], w) for c, w in VAR]:
        assert 2 <= world <= min(shape[2], 8), (shape, world)
        assert (shape, world) in COUNTS
    assert all((s, w) in CONST for s, w in ref.DIST_GUESS_CASES) and all((c, w) in VAR for c, w in vr.DIST_GUESS_CASES)
    assert all(s in ref.GUESS_SHAPES for s, _ in ref.DIST_GUESS_CASES)
    assert all((s, w) in CONST for s, w, _ in CONST_SETS) and all((c, w) in VAR for c, w, _ in VAR_SETS)
    assert {(s, w) for s, w, _ in CONST_SETS} == {((65, 3, 5), 3), ((130, 6, 9), 2)} and any(w == 3 for _, w, _ in VAR_SETS)
    # BEAT_RR_RY=4 runs on the shapes with a full block of four rows, and those keep a one-plane slab and a middle slab
    ry4 = [(s, w) for s, w in CONST if s[1] >= ref.DIST_RY4_MIN_NY]
    assert {s for s, _ in ry4} == {(64, 4, 3), (63, 5, 4), (129, 7, 6), (130, 6, 9), (3, 70, 2), (125, 4, 2)}


@pytest.mark.parametrize("shape,world", sorted(COUNTS), ids=lambda v: ref.shape_key(v) if isinstance(v, tuple) else str(v))
def test_slab_deals_the_counts_the_tables_claim(shape, world):
    parts = slabs(shape[2], world)
    assert tuple(s.nz for s in parts) == COUNTS[(shape, world)] == tuple(ref.slab_counts(shape[2], world))
    assert parts[0].z0 == 0 and parts[-1].z1 == shape[2] and all(a.z1 == b.z0 for a, b in zip(parts, parts[1:]))
    assert [s.lo_phys for s in parts] == [r == 0 for r in range(world)] and [s.hi_phys for s in parts] == [r == world - 1 for r in range(world)]


def one_plane(shape, world):
    return 1 in ref.slab_counts(shape[2], world)


def test_every_named_feature_holds():
    # constant coefficients: the segment and row-block features are those of tests/test_pcg_ref_cpu.py's shapes; here what the cut adds
    assert one_plane((64, 4, 3), 2) and one_plane((64, 4, 3), 3) and one_plane((65, 3, 5), 3) and one_plane((63, 5, 4), 4)
    for shape in ((3, 70, 2), (125, 4, 2), (128, 2, 2), (2, 2, 2)):
        assert ref.slab_counts(shape[2], 2) == [1, 1]
    assert ref.slab_counts(7, 7) == [1] * 7 and ref.slab_counts(5, 5) == [1] * 5
    assert 63 % 62 == 1 and 5 % 4 == 1 and 65 - 62 == 3 and 7 % 2 == 1 and -(-129 // 62) == 3 and -(-130 // 62) == 3 and 70 % 4 == 2
    # a middle slab (both ghost planes live) of more than one plane, of one plane, and a one-plane slab at a face of the whole grid
    assert ref.slab_counts(9, 3)[1] == 3 and ref.slab_counts(9, 4)[1:3] == [2, 2] and ref.slab_counts(5, 3) == [2, 2, 1]
    # per-node rows
    assert 18 % 8 == 2 and 125 - 2 * 62 == 1 and 16 % 8 == 0 and 9 < 16 and 70 % 8 == 6
    for mask in vr.MASKS:  # every slab of 125 x 18 x 20 holds tissue, and every face cuts a run of tissue planes in two
        cs = vr.case(((125, 18, 20), mask))
        per_plane = cs.tissue.reshape(20, -1).sum(axis=1)
        for world in (2, 3, 4):
            for s in slabs(20, world):
                assert per_plane[s.z0 : s.z1].sum() > 0, (mask, world, s.rank)
        if mask in ("full", "cutshell"):
            assert all(per_plane[s.z0 - 1] > 0 and per_plane[s.z0] > 0 for world in (2, 3, 4) for s in slabs(20, world)[1:])
    layers = vr.case(((125, 18, 20), "layers")).tissue.reshape(20, -1).any(axis=1)
    assert np.nonzero(layers)[0].tolist() == [0, 1, 3, 4, 7, 8, 12, 13, 15, 16]
    assert not layers[5] and layers[4] and not layers[10] and not layers[9] and layers[15] and not layers[14]  # faces 5, 10, 15 of 4 ranks
    # 63 x 16 x 6 layers on 6 ranks: cell layers 0 and 3 -> node planes 0, 1, 3, 4; ranks 2 and 5 own no tissue node
    cs = vr.case(((63, 16, 6), "layers"))
    owns = [bool(cs.tissue[s.z0 * 63 * 16 : s.z1 * 63 * 16].any()) for s in slabs(6, 6)]
    assert owns == [True, True, False, True, True, False]
    assert all(cs.tissue[s.z0 * 63 * 16 : s.z1 * 63 * 16].any() for s in slabs(6, 2))
    for mask in ("full", "specks"):
        cs = vr.case(((63, 16, 6), mask))
        assert all(cs.tissue[s.z0 * 1008 : s.z1 * 1008].any() for w in (2, 3) for s in slabs(6, w)), mask
    # 6 x 4 x 71 layers on 8 ranks: faces in front of planes 9, 18, ..., 63; behind a run of tissue planes, in front of one, and in a gap
    cs = vr.case(((6, 4, 71), "layers"))
    planes = cs.tissue.reshape(71, -1).any(axis=1)
    faces = [s.z0 for s in slabs(71, 8)[1:]]
    assert faces == [9, 18, 27, 36, 45, 54, 63]
    kinds = {(bool(planes[z - 1]), bool(planes[z])) for z in faces}
    assert kinds == {(True, False), (False, True), (False, False)}
    assert all(planes[s.z0 : s.z1].any() for s in slabs(71, 8))
    runs = np.diff(np.concatenate([[0], planes.astype(int), [0]]))
    assert (runs == 1).sum() >= 17  # many runs along z
    # what keeps a rank off the tiles: a slab of one plane (vtl_sizes_declined); the cases with such a slab
    assert {(c[0], w) for c, w in VAR if one_plane(c[0], w)} == {((63, 16, 6), 6), ((62, 9, 5), 5), ((3, 70, 3), 3), ((2, 2, 2), 2)}


WORST = {"const": [(0.0, None), (0.0, None)], "var": [(0.0, None), (0.0, None)]}


def slab_ordered_run_passes(kind, key, p, r, bounds, v, cuts):
    """The float64 PCG of the case with slab-ordered dot products, as a device's results, through the device's checks."""
    A = p.A
    xs, rn, bn = ref.pcg_iterates(A, r_rhs(p, v), v, 1.0 / A.diagonal(), r.kmax, np.float64, dot=ref.slab_dot(bounds))
    data = {}
    for k in cuts:
        data[f"{key}/k={k}|x"] = xs[k - 1]
        data[f"{key}/k={k}|rec"] = np.array([k, -3, rn[k - 1], bn])
    for rtol in ref.RTOLS:
        k = next(k for k in range(1, r.kmax + 1) if rn[k - 1] <= rtol * bn)
        data[f"{key}/rtol={rtol:g}|x"] = xs[k - 1]
        data[f"{key}/rtol={rtol:g}|rec"] = np.array([k, 2, rn[k - 1], bn])
    c = Check(data)
    for k in cuts:
        c.cut(f"{key}/k={k}", r, k)
    for rtol in ref.RTOLS:
        c.uncut(f"{key}/rtol={rtol:g}", r, rtol)
    WORST[kind][0] = max(WORST[kind][0], c.worst, key=lambda w: w[0])
    WORST[kind][1] = max(WORST[kind][1], c.worst_norm, key=lambda w: w[0])
    print(f"{key}: err / yardstick {c.worst[0]:.2f} ({c.worst[1]}), norm / yardstick {c.worst_norm[0]:.2f} ({c.worst_norm[1]}); so far {WORST[kind]}")
    assert not c.failures, "the case is unfit (move its seed with SEED_SHIFT):\n" + "\n".join(c.failures)


def r_rhs(p, v):
    return ref.rhs_longdouble(p, v).astype(np.float64)  # (what reference() starts its float64 run from)


@pytest.mark.parametrize("shape,world", CONST, ids=lambda v: ref.shape_key(v) if isinstance(v, tuple) else f"w{v}")
def test_bound_admits_the_decomposition_constant_coefficients(shape, world, ops="cn"):
    p, r = ref.problem(shape, ops), ref.plain_reference(shape, ops)
    plane = shape[0] * shape[1]
    bounds = [0] + [int(z) * plane for z in np.cumsum(ref.slab_counts(shape[2], world))]
    slab_ordered_run_passes("const", f"{ref.case_key(shape, ops)}/w{world}", p, r, bounds, ref.field(shape), ref.CUTS)


@pytest.mark.parametrize("shape,world,ops", CONST_SETS, ids=lambda v: v if isinstance(v, str) else ref.shape_key(v) if isinstance(v, tuple) else f"w{v}")
def test_bound_admits_the_decomposition_off_theta_one_half_constant_coefficients(shape, world, ops):
    test_bound_admits_the_decomposition_constant_coefficients(shape, world, ops)


@pytest.mark.parametrize("case,world", VAR, ids=lambda v: vr.case_key(v) if isinstance(v, tuple) else f"w{v}")
def test_bound_admits_the_decomposition_per_node_rows(case, world, ops="cn"):
    cs, r = vr.case(case), vr.plain_reference(case, ops)
    plane = cs.shape[0] * cs.shape[1]
    before = np.concatenate([[0], np.cumsum(cs.tissue)])  # tissue nodes in front of a node
    bounds = [0] + [int(before[int(z) * plane]) for z in np.cumsum(ref.slab_counts(cs.shape[2], world))]
    assert bounds[-1] == cs.n
    slab_ordered_run_passes("var", f"{vr.opset_key(case, ops)}/w{world}", vr.problem_of(case, ops), r, bounds, vr.field(cs), vr.cuts_of(cs, vr.CUTS_SHORT))


@pytest.mark.parametrize("case,world,ops", VAR_SETS, ids=lambda v: v if isinstance(v, str) else vr.case_key(v) if isinstance(v, tuple) else f"w{v}")
def test_bound_admits_the_decomposition_off_theta_one_half_per_node_rows(case, world, ops):
    test_bound_admits_the_decomposition_per_node_rows(case, world, ops)
