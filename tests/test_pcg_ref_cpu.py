"""The host PCG of tests/_pcg_ref.py held to account, and the conditions its cases must meet for tests/test_rr_iterates_gpu.py and
tests/test_small_iterates_gpu.py to mean what they say: the reference converges to a direct solve and counts like oracle/fem.pcg_jacobi, no stop is a near tie (so
the device's iteration count can be asked to EQUAL the host's), every cut happens while the iterate still moves, and every
bound is positive."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import _pcg_ref as ref
from oracle import fem

SHAPES = ref.all_shapes()  # the register-row cases, then what the one-launch cases add
GUESS_SHAPES = list(ref.GUESS_SHAPES) + [s for s in ref.SMALL_GUESS_SHAPES if s not in ref.GUESS_SHAPES]
# (shape, set): every shape under cn, as before the sets had names (and under the same test ids), then the pairs off theta = 1/2
PAIRS = [(s, "cn") for s in SHAPES] + ref.opset_pairs()
GUESS_PAIRS = [(s, "cn") for s in GUESS_SHAPES] + [(s, name) for s in ref.OPSET_GUESS_SHAPES + ref.SMALL_OPSET_GUESS_SHAPES for name in ref.NEW_SETS] + \
    [(s, name) for (s, _), sets in ref.DIST_OPSET_GUESS.items() for name in sets]
GUESS_PAIRS = list(dict.fromkeys(GUESS_PAIRS))


def pair_id(pair) -> str:
    return ref.case_key(*pair)


def test_longdouble_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


def test_case_table_is_consistent():
    assert set(ref.CHUNK_SHAPES) <= set(ref.SHAPES) and set(ref.GUESS_SHAPES) <= set(ref.SHAPES)
    assert set(ref.SMALL_GUESS_SHAPES) <= set(ref.SMALL_SHAPES)
    assert all(ref.SHAPES[s] == ref.SMALL_SHAPES[s] for s in set(ref.SHAPES) & set(ref.SMALL_SHAPES))
    assert len(SHAPES) == len(set(SHAPES)) == len(set(ref.SHAPES) | set(ref.SMALL_SHAPES))
    assert len({ref.seed_of(s) for s in SHAPES}) == len(SHAPES)
    assert max(int(np.prod(s)) for s in SHAPES) <= 8192  # a few thousand nodes: where the index arithmetic branches, not the workload
    # the sets: cn is the operator of every case from before the sets had names; skew tells every factor from every other
    assert ref.OPSETS["cn"].triple == (0.01, 0.5, 0.05) == (ref.C_M, ref.THETA, ref.DT) and ref.OPSETS["be"].triple == (0.01, 1.0, 0.05)
    assert ref.OPSETS["skew"].triple == (0.013, 0.25, 0.08) and all(o.name == name for name, o in ref.OPSETS.items())
    be, skew = ref.OPSETS["be"], ref.OPSETS["skew"]
    assert (1 - be.theta) * be.dt == 0.0 and be.theta * be.dt == be.dt
    assert len({skew.c_m, skew.theta * skew.dt, (1 - skew.theta) * skew.dt, skew.dt, skew.theta, 1 - skew.theta}) == 6
    assert set(ref.OPSET_SHAPES) <= set(ref.SHAPES) and set(ref.OPSET_GUESS_SHAPES) <= set(ref.OPSET_SHAPES) & set(ref.GUESS_SHAPES)
    assert set(ref.SMALL_OPSET_SHAPES) <= set(ref.SMALL_SHAPES) and set(ref.SMALL_OPSET_GUESS_SHAPES) <= set(ref.SMALL_OPSET_SHAPES) & set(ref.SMALL_GUESS_SHAPES)
    assert sorted(s for s in ref.SMALL_OPSET_SHAPES if not ref.small_takes(s)) == [(1, 5, 4)]  # the fallback under the one-launch solve
    assert all(s in ref.DIST_CASES and w in ref.DIST_CASES[s] for s, w in ref.DIST_OPSET_CASES) and set(ref.DIST_OPSET_GUESS) <= set(ref.DIST_GUESS_CASES)
    for table in (ref.OPSET_SHAPES, ref.SMALL_OPSET_SHAPES, ref.DIST_OPSET_CASES):
        assert all(set(sets) <= set(ref.NEW_SETS) and "be" in sets for sets in table.values())
        assert all("skew" in sets or ref.dim_of(k if len(k) == 3 else k[0]) == 1 for k, sets in table.items())  # 1-D rows take be only
    assert ref.RETIME == ("cn", "skew", "cn")
    assert len(PAIRS) == len(set(PAIRS)) and max(int(np.prod(s)) for s, _ in PAIRS) <= 8192
    assert ref.problem((65, 3, 5), "be").mass is ref.problem((65, 3, 5)).mass and ref.problem((65, 3, 5), "be").ops == be
    for s in SHAPES:
        v = ref.field(s)
        assert abs(v.mean()) < 1e-12 and 0.1 < np.abs(v).max() < 10.0
        assert np.array_equal(v, ref.field(s))  # fixed seeds


def test_one_launch_cases_aim_at_what_they_say():
    """The sizes of SMALL_SHAPES against the kernel's constants, its LDS request by small_lds_bytes / small_margin of
    csrc/beat_pde_small.hip written out: every template instance is launched, by a full and by a partly empty register array where
    there are both, and the LDS limit is met from both sides."""
    assert ref.SMALL_THREADS * ref.SMALL_MAX_PER_THREAD == 8192 and ref.SMALL_LDS_LIMIT == 153_600

    def lds(shape):  # tables A and B, 6 x 8 partials, 1 / diag, margin + n + margin
        nx, ny, nz = shape
        margin = -(-(nx * ny + nx + 1) // 8) * 8
        return 8 * (2 * 27 * 16 + 6 * 8 + 32 + nx * ny * nz + 2 * margin)

    assert all(ref.small_lds_bytes(s) == lds(s) for s in ref.SMALL_SHAPES)
    assert lds((64, 94, 1)) == 153_088 and lds((64, 95, 1)) == 154_624
    assert ref.small_takes((64, 94, 1)) and not ref.small_takes((64, 95, 1)) and int(np.prod((64, 95, 1))) <= 8192
    assert max(lds(s) for s in ref.SMALL_SHAPES if ref.small_takes(s)) == lds((64, 94, 1))
    taken = [s for s in ref.SMALL_SHAPES if ref.small_takes(s)]
    assert {ref.small_instance(s) for s in taken} == {2, 4, 6, 8, 10, 12, 16}
    nodes = {s: int(np.prod(s)) for s in ref.SMALL_SHAPES}
    assert nodes[(128, 2, 2)] == 512 and nodes[(3, 3, 57)] == 513 and nodes[(5, 5, 41)] == 1025 and ref.small_instance((5, 5, 41)) == 4
    assert nodes[(64, 32, 1)] == 4 * 512 and nodes[(16, 16, 16)] == 8 * 512 and nodes[(32, 16, 16)] == nodes[(2, 2, 2048)] == 8192
    assert ref.small_instance((41, 15, 7)) == 10 and ref.small_instance((129, 7, 6)) == 12 and ref.small_instance((43, 9, 7)) == 6
    assert ref.small_instance((130, 6, 9)) == 16 and nodes[(130, 6, 9)] <= 14 * 512  # slots 14 and 15 empty in every thread
    assert not ref.small_takes((2, 2, 2049)) and ref.small_lds_bytes((2, 2, 2049)) < ref.SMALL_LDS_LIMIT // 2  # the node count alone
    assert sorted(s for s in ref.SMALL_SHAPES if not ref.small_takes(s)) == [(1, 1, 7), (1, 5, 4), (1, 9, 1), (6, 1, 5), (64, 95, 1)]


@pytest.mark.parametrize("shape", SHAPES + [(5, 4, 1), (1, 1, 1), (7, 1, 1)], ids=ref.shape_key)
def test_flat_neighbour_index_is_right_where_the_one_launch_solve_takes_the_box(shape):
    """pcg_small_kernel's stencil sum, s = sum_k tab[type][k] p[i + doff[k]] with ONE linear offset per stencil point into a vector
    between zero margins, emulated in numpy: it is A p on every box beat_small_available's rule for collapsed axes lets through, and
    wrong by O(1) on those of the cases it declines (an axis of one node in front of a longer one, under tables of higher
    dimension: its 'interior' coefficients meet a node of the box)."""
    dim = ref.dim_of(shape) if shape in SHAPES else 3
    mt, kt = ref.tables(dim)
    tab = ref.C_M * mt + ref.THETA * ref.DT * kt
    nx, ny, nz = shape
    n, margin = nx * ny * nz, nx * ny + nx + 1
    x = np.random.default_rng(ref.seed_of(shape)).standard_normal(n)
    p = np.concatenate([np.zeros(margin), x, np.zeros(margin)])
    typ, at = fem.node_types(shape), margin + np.arange(n)
    y = sum(tab[typ, k] * p[at + ox + nx * oy + nx * ny * oz] for k, (ox, oy, oz) in enumerate(fem.STENCIL_OFFSETS))
    want = fem.apply_stencil(tab, shape, x)
    err = np.abs(y - want).max() / np.abs(want).max()
    if ref.small_declines_collapsed(shape):
        assert err > 0.01, err
    else:
        assert err <= 16 * 2.0**-53, err


def test_matvec_matches_scipy_and_gains_precision():
    p = ref.problem((65, 3, 5))
    x = ref.field(p.shape)
    y64 = ref.matvec(p.A, x, np.float64)
    yL = ref.matvec(p.A, x.astype(np.longdouble), np.longdouble)
    scale = np.abs(p.A).dot(np.abs(x)).max()
    assert np.abs(y64 - p.A @ x).max() <= 8 * 2.0**-53 * scale
    # one row in exact rational arithmetic
    from fractions import Fraction

    row = 567
    sl = slice(p.A.indptr[row], p.A.indptr[row + 1])
    exact = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(p.A.data[sl], x[p.A.indices[sl]]))
    hi = float(yL[row])
    got = Fraction(hi) + Fraction(float(yL[row] - np.longdouble(hi)))
    assert abs(got - exact) <= Fraction(2.0**-60 * scale)
    assert abs(Fraction(float(y64[row])) - exact) <= Fraction(8 * 2.0**-53 * scale)


@pytest.mark.parametrize("shape", SHAPES, ids=ref.shape_key)
def test_expanded_tables_are_the_assembled_matrices(shape):
    """The matrices of a case -- oracle/fem's per-node-type tables, which the device is given, expanded over the box -- are the
    P1 matrices assembled on the whole mesh, an axis of one node 'interior' with its neighbours outside the box, up to the last
    digits (in which the assembled entries differ from node to node); and the product's own tables agree with them as closely."""
    from beat import _stencil

    p = ref.problem(shape)
    mass, stiff, _ = ref.assembled(shape)
    noise = 4 * max(shape) * 2.0**-53  # the assembly takes a cell's geometry from its nodes' coordinates: u * coordinate / h
    for mine, theirs in ((p.mass, mass), (p.stiff, stiff)):
        assert abs(mine - theirs).max() <= noise * abs(theirs).max()
    mt, kt = _stencil.stencil_tables(p.dim, (ref.H,) * p.dim, ref.conductivity(p.dim))
    assert np.abs(mt - p.mass_tab).max() <= 64 * 2.0**-53 * np.abs(mt).max() and np.abs(kt - p.stiff_tab).max() <= 64 * 2.0**-53 * np.abs(kt).max()
    x = ref.field(shape)
    np.testing.assert_allclose(p.A @ x, fem.apply_stencil(ref.C_M * p.mass_tab + ref.THETA * ref.DT * p.stiff_tab, shape, x), rtol=0,
                               atol=8 * 2.0**-53 * np.abs(p.A).dot(np.abs(x)).max())
    assert (p.A != p.A.T).nnz == 0 or abs(p.A - p.A.T).max() <= 8 * 2.0**-53 * abs(p.A).max()


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_reference_is_right_and_no_stop_is_a_near_tie(pair):
    shape, ops = pair[0], ref.opset(pair[1])
    p, r = ref.problem(shape, ops), ref.plain_reference(shape, ops)
    assert p.ops == ops
    v = ref.field(shape)
    bL = ref.rhs_longdouble(p, v)
    # the right-hand side: the float64 form of the same expression, the set's numbers written where they belong
    C_m, theta, dt = ops.triple
    b64 = C_m * (p.mass @ v) - (1 - theta) * dt * (p.stiff @ v) + dt * sum(a * w for a, w in zip(ref.STIM_AMPS, p.weights))
    assert np.array_equal(b64, p.rhs_float64(v))
    assert abs(p.A - (C_m * p.mass + theta * dt * p.stiff)).max() <= 2 * 2.0**-53 * abs(p.A).max()
    if ops.name == "be":  # B = C_m Mass: K has no part in b
        assert np.array_equal(b64, C_m * (p.mass @ v) + dt * sum(a * w for a, w in zip(ref.STIM_AMPS, p.weights)))
    assert np.abs(bL.astype(np.float64) - b64).max() <= 16 * 2.0**-53 * np.abs(b64).max()
    assert float(r.bL) == pytest.approx(np.linalg.norm(b64), rel=1e-14)
    # converged: the direct solve
    x = spla.spsolve(p.A.tocsc(), bL.astype(np.float64))
    assert np.abs(r.xL[r.kmax].astype(np.float64) - x).max() <= 1e-12 * np.abs(x).max()
    for rtol in ref.RTOLS:
        k = r.stop(rtol)
        _, its, _ = fem.pcg_jacobi(p.A, b64, v.copy(), rtol=rtol, atol=1e-300, maxit=ref.KMAX)
        assert its == k, (rtol, its, k)
        thr = np.longdouble(rtol) * r.bL
        assert r.rL[k] <= thr * (1 - 1e-6), (rtol, k, float(r.rL[k] / thr))
        below = r.rL[k - 1] if k > 1 else None
        if below is not None:
            assert below >= thr * (1 + 1e-6), (rtol, k, float(below / thr))
        assert k < ref.KMAX - 5 and k <= r.kmax
    # every cut happens before convergence: the iterate it is compared with is still moving.  The one exception there can be is
    # (1, 1, 7): CG on 7 unknowns ends with its 7th step, so the cut at 7 compares the solution itself; its cuts below 7 move.
    if p.n > max(ref.CUTS):
        assert r.rL[max(ref.CUTS)] > np.longdouble(1e-12) * r.bL
    else:
        assert shape == (1, 1, 7)
        assert r.rL[p.n - 1] > np.longdouble(1e-12) * r.bL and r.rL[p.n] <= np.longdouble(1e-12) * r.bL
    assert r.stop(ref.RTOLS[0]) >= 1
    for k in ref.CUTS:
        assert r.x_bound(k) > 0.0 and r.residual_bound(k) > 0.0 and np.isfinite(r.x_bound(k))
        assert r.delta(k) > 0.0 or r.x_floor(k) > 0.0
        assert r.x_bound(k) <= 1e-12 * max(1.0, np.abs(r.xL[k]).max())  # the yardstick is rounding error, nothing coarser
    assert r.rhs_norm_bound() > 0.0


@pytest.mark.parametrize("pair", GUESS_PAIRS, ids=pair_id)
def test_guess_sequence_moves_and_its_cuts_happen_before_convergence(pair):
    """The fields of the guess cases with exact increments in place of the device's: the extrapolated start is still O(1) wrong, so
    the cut iterates (k = 1, 3) are far from converged."""
    shape = pair[0]
    p = ref.problem(*pair)
    solve = spla.factorized(p.A.tocsc())
    incs = []
    for j in range(1, ref.GUESS_SOLVES + 1):
        v = ref.field(shape, j)
        incs.insert(0, solve(ref.rhs_longdouble(p, v).astype(np.float64)) - v)
    v = ref.field(shape, ref.GUESS_SOLVES + 1)
    bL = ref.rhs_longdouble(p, v)
    for order in ref.GUESS_ORDERS:
        e = ref.guess_increment(order, incs)
        expect = {1: incs[0], 3: 3 * incs[0] - 3 * incs[1] + incs[2]}[order]
        np.testing.assert_allclose(e.astype(np.float64), expect, rtol=0, atol=1e-14 * np.abs(expect).max())
        r = ref.reference(p, bL, v.astype(np.longdouble) + e, max(ref.GUESS_CUTS))
        assert r.rL[max(ref.GUESS_CUTS)] > np.longdouble(1e-12) * r.bL
        assert r.rL[1] > np.longdouble(1e-3) * r.bL  # the guess did not all but solve it
        for k in ref.GUESS_CUTS:
            assert r.x_bound(k) > 0.0


def test_single_reduction_recurrence_gives_the_same_iterates():
    """Chronopoulos & Gear's step lengths (beat_pcg_merged_next's expressions), in longdouble: the iterates of the classic loop."""
    L = np.longdouble
    shape = (65, 3, 5)
    p, r = ref.problem(shape), ref.plain_reference(shape)
    v = ref.field(shape).astype(L)
    b = ref.rhs_longdouble(p, ref.field(shape))
    A = p.operator(L)
    dinv = L(1) / p.diagonal(L)
    x, res = v.copy(), b - ref.matvec(A, v, L)
    pdir, alpha, g_old = np.zeros_like(x), L(0), L(0)
    for k in range(1, 9):
        u = dinv * res
        g, d = res @ u, u @ ref.matvec(A, u, L)
        beta = L(0) if k == 1 else g / g_old
        alpha = g / d if k == 1 else g / (d - beta * g / alpha)
        pdir = u + beta * pdir
        x = x + alpha * pdir
        res = res - alpha * ref.matvec(A, pdir, L)
        g_old = g
        assert np.abs(x - r.xL[k]).max() <= 2.0**-56 * np.abs(r.xL[k]).max(), k
