"""CPU: the bi-ventricular fibre rule (Bayer's, with bislerp).  tests/_fibres_biv_ref.py (NumPy, written from the rule's text in
include/beat_hip.h) is held to the closed forms of an LV wall, a septum and an RV wall, to the frame's properties and to the exact
degenerate cases; the bi-ventricular half of csrc/beat_fibres_kernel.h -- the text the kernel runs -- is built with g++ into
tests/fibres_biv_host_harness.cpp, once plain and once with the address and undefined-behaviour sanitizers, and held to the reference,
bislerp and the quaternion conversions on their own as well; the binding's argument list is held to the header; beat.fibres refuses
what it does not do before a device is touched."""
import ctypes as C
import logging
import re
from pathlib import Path

import numpy as np
import pytest

import _fibres_biv_host as host
import _fibres_biv_ref as ref

ROOT = Path(__file__).resolve().parents[1]
Z = np.array([0.0, 0.0, 1.0])


def _up_to_sign(got, want):
    """max |got - (+-want)|, the sign chosen per voxel: a fibre is a line, and bislerp may hand back a frame with two vectors negated."""
    sign = np.where((got * want).sum(axis=1) < 0.0, -1.0, 1.0)[:, None]
    return np.abs(got - sign * want).max()


# ---- the reference itself ----------------------------------------------------------------------------------------------------------

def _closed(region, angles):
    cells, h, L, x, _ = ref.slab()
    fields, angle = ref.closed_form(region, angles)
    return ref.rule(cells, h, *(fn(x / L[0]) for fn in fields), Z, angles), angle


@pytest.mark.parametrize("region", ref.REGIONS)
def test_closed_forms(region):
    """(1) exactly linear fields on the (8, 4, 4) slab, e_l = z, beta = 0, angles (40, -50): the fibre lies in the (y, z) plane at
    alpha_endo + c^2 (alpha_epi - alpha_endo) in both walls and at alpha_endo (1 - 2 x / L) in the septum, up to sign, to 1e-14; the
    RV wall is the case in which the endo -> epi blend has to take a flipped candidate."""
    out, angle = _closed(region, (40.0, -50.0, 0.0, 0.0))
    assert out.count == 0
    want = np.stack([np.zeros_like(angle), np.cos(angle), np.sin(angle)], axis=1)
    assert _up_to_sign(out.f, want) <= 1e-14
    assert _up_to_sign(out.s, np.broadcast_to(np.array([1.0, 0.0, 0.0]), want.shape)) <= 1e-14
    wall = out.candidate[:, 1]
    if region == "lv wall":
        assert (wall == 0).all() and (out.candidate[:, 0] == -1).all()  # (phi_rv = 0: no endocardial blend)
    elif region == "rv wall":
        assert (wall != 0).all()
    else:
        assert (wall == -1).all() and (out.candidate[:, 0] == 0).all()  # (phi_epi = 0: no endo -> epi blend)


def test_rv_wall_sheets_are_the_lv_wall_s():
    """(1, last) with beta = (20, -20) the RV wall's sheet -- and the whole frame -- is the LV wall's up to sign."""
    angles = (40.0, -50.0, 20.0, -20.0)
    lv, _ = _closed("lv wall", angles)
    rv, _ = _closed("rv wall", angles)
    assert np.abs(lv.s[:, 1:]).max() > 0.1  # (the sheets do leave x)
    for name in ("s", "f", "n"):
        assert _up_to_sign(getattr(rv, name), getattr(lv, name)) <= 1e-14, name


@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_frame_properties(case):
    """(2) unit length, mutual orthogonality and f x n = s, to 1e-14, on the shared inputs, which meet the tolerance's conditions."""
    r = ref.case(*case).ref
    ref.assert_conditions(r)
    act = r.active
    f, s, n = r.f[act], r.s[act], r.n[act]
    for v in (f, s, n):
        assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 1e-14
    for a, b in ((f, s), (f, n), (s, n)):
        assert np.abs((a * b).sum(axis=1)).max() <= 1e-14
    assert np.abs(np.cross(f, n) - s).max() <= 1e-14


def test_blends_over_the_shared_cases():
    """The RV-wall cases take a flipped candidate in the endo -> epi blend on at least one voxel, the LV-wall cases never do."""
    for region, flipped in (("rv wall", True), ("lv wall", False)):
        chosen = np.concatenate([ref.case(*c).ref.candidate[ref.case(*c).ref.active, 1] for c in ref.CASES if c[3] == region])
        assert (chosen >= 0).all()
        assert (chosen != 0).any() if flipped else (chosen == 0).all(), region


VOXEL = 3 + 8 * (2 + 4 * 1)  # voxel (3, 2, 1) of the slab: its 8 corners are nodes [1:3, 2:4, 3:5]


def _pin(field, value):
    out = field.copy()
    out.reshape(5, 5, 9)[1:3, 2:4, 3:5] = value
    return out


def _degenerate_problems():
    """The exact cases of (3) on the slab: name -> (phi_lv, phi_rv, phi_epi); none of them has a degenerate voxel but "all constant"."""
    _, _, L, x, z = ref.slab()
    X = x / L[0]
    y = np.tile(np.repeat(np.arange(5) * 0.25, 9), 5)
    lv, rv, epi = 1.0 - X, 0.5 * X + 0.2 * y, 0.3 * y + 0.1 * X
    return {"plain": (lv, rv, epi), "all constant": (_pin(lv, 0.4), _pin(rv, 0.3), _pin(epi, 0.2)),
            "rv zero in the voxel": (lv, _pin(rv, 0.0), epi), "rv zero": (lv, 0.0 * rv, epi),
            "rv 0.3 in the voxel": (lv, _pin(rv, 0.3), epi), "rv 0.3": (lv, 0.0 * rv + 0.3, epi),
            "no endocardial share": (-X - 0.1, -0.5 * X - 0.1, 0.0 * X),
            "epi above 1": (1.0 - X, 0.0 * X, X + 3.0), "epi below 0": (1.0 - X, 0.0 * X, X - 3.0)}


def _check_degenerates(solve):
    """``solve(phi_lv, phi_rv, phi_epi, angles_deg)`` -> f, s, n, M, count."""
    P = _degenerate_problems()
    assert solve(*P["plain"], ref.ANGLES).count == 0
    out = solve(*P["all constant"], ref.ANGLES)  # all three transmural fields constant over one voxel
    assert out.count == 1
    assert not out.f[VOXEL].any() and not out.s[VOXEL].any() and not out.n[VOXEL].any()
    assert np.array_equal(out.M[VOXEL], ref.S_T * np.eye(3))
    others = np.arange(len(out.f)) != VOXEL
    assert np.abs(np.linalg.norm(out.f[others], axis=1) - 1.0).max() <= 1e-14
    for value in ("zero", "0.3"):  # only phi_rv constant there: Q_rv drops out, as it does everywhere when phi_rv is that constant
        one, everywhere = solve(*P[f"rv {value} in the voxel"], ref.ANGLES), solve(*P[f"rv {value}"], ref.ANGLES)
        assert one.count == 0 and everywhere.count == 0
        for name in ("f", "s", "n", "M"):
            assert np.array_equal(getattr(one, name)[VOXEL], getattr(everywhere, name)[VOXEL]), (value, name)
    flat = (40.0, -50.0, 0.0, 0.0)
    a_endo, a_epi = np.deg2rad(40.0), np.deg2rad(-50.0)
    endo, epi = np.array([[0.0, np.cos(a_endo), np.sin(a_endo)]]), np.array([[0.0, np.cos(a_epi), np.sin(a_epi)]])
    out = solve(*P["no endocardial share"], flat)  # c_lv + c_rv = 0: d = 0, the LV's frame at alpha_endo
    assert out.count == 0 and np.isfinite(out.f).all() and _up_to_sign(out.f, np.broadcast_to(endo, out.f.shape)) <= 1e-14
    out = solve(*P["epi above 1"], flat)  # nodal values past 1 (a solve's overshoot): c_epi = 1, the epicardial frame
    assert out.count == 0 and _up_to_sign(out.f, np.broadcast_to(epi, out.f.shape)) <= 1e-14
    out = solve(*P["epi below 0"], flat)  # ... and below 0: c_epi = 0, the endocardial one
    assert out.count == 0 and _up_to_sign(out.f, np.broadcast_to(endo, out.f.shape)) <= 1e-14


def test_exact_degenerates():
    """(3) all three fields constant over a voxel; only phi_rv constant there; c_lv + c_rv = 0; overshooting nodal values."""
    cells, h, _, _, _ = ref.slab()
    _check_degenerates(lambda lv, rv, epi, angles: ref.rule(cells, h, lv, rv, epi, Z, angles))


def test_inactive_voxels():
    """(3, last) zeros outside the mask, not counted, and the voxels inside are the full box's."""
    cells = (5, 3, 2)
    full, masked = ref.case(cells, False, False, "septum"), ref.case(cells, False, True, "septum")
    act = masked.active
    assert act.any() and not act.all()
    for name in ("f", "s", "n", "M"):
        got, want = getattr(masked.ref, name), getattr(full.ref, name)
        assert not got[~act].any() and np.array_equal(got[act], want[act]), name
    flat = np.full_like(full.phi_lv, 0.5)  # every voxel degenerate: only the active ones count
    assert ref.rule(cells, ref.H, flat, flat, flat, np.array(ref.AXIS), ref.ANGLES, act).count == int(act.sum())


# ---- the header: bislerp and the quaternions on their own ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    out = tmp_path_factory.mktemp("fibres_biv_host_harness")
    return {name: host.build(out, name) for name in host.BUILDS}


def _rotations(count, seed=77):
    rng = np.random.default_rng(seed)
    return [ref.to_matrix(q) for q in rng.standard_normal((count, 4))]


@pytest.mark.parametrize("build", list(host.BUILDS))
def test_bislerp_ends_and_flips(executables, build):
    """(4) t = 0 gives the chosen candidate and t = 1 gives Q_b; bislerp(Q, Q diag(-1, 1, -1), t) is Q diag(-1, 1, -1) for every t."""
    exe = executables[build]
    R = _rotations(12)
    flips = [np.diag(d) for d in ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))]
    for Qa, Qb in zip(R[:6], R[6:]):
        _, k, gap = ref.bislerp(Qa, Qb, 0.0)
        assert gap >= ref.GAP_MIN  # (so that the header's choice is the reference's)
        assert np.abs(host.bislerp(exe, Qa, Qb, 0.0).Q - Qa @ flips[k]).max() <= 1e-14
        assert np.abs(host.bislerp(exe, Qa, Qb, 1.0).Q - Qb).max() <= 1e-14
        half = host.bislerp(exe, Qa, Qb, 0.5)
        assert np.abs(half.Q - ref.bislerp(Qa, Qb, 0.5)[0]).max() <= 1e-14
        assert abs(np.linalg.norm(half.q) - 1.0) <= 1e-14
    for Q in R[:4]:
        for t in (0.0, 0.3, 0.5, 1.0):
            assert np.abs(host.bislerp(exe, Q, Q @ flips[2], t).Q - Q @ flips[2]).max() <= 1e-14


@pytest.mark.parametrize("build", list(host.BUILDS))
def test_quaternion_round_trips(executables, build):
    """(4, last) quaternion -> matrix (here) -> quaternion (Shepperd, the header) -> matrix (the header), on rotations whose largest
    component is w, x, y and z in turn: one for each of Shepperd's branches, a second set with two components nearly as large."""
    exe = executables[build]
    for small in (0.2, 0.95):
        for lead in range(4):
            q = np.array([small, -small * 0.5, small * 0.7, small * 0.3])
            q[lead] = 1.0
            q /= np.linalg.norm(q)
            assert int(np.argmax(np.abs(q))) == lead
            R = ref.to_matrix(q)
            assert int(np.argmax([np.trace(R), R[0, 0], R[1, 1], R[2, 2]])) == lead  # this rotation takes branch `lead`
            got = host.bislerp(exe, R, R, 0.5)
            assert np.abs(got.qa - q).max() <= 1e-15 and np.array_equal(got.qa, got.qb)  # (q[lead] > 0: the sign Shepperd gives)
            assert np.abs(got.Q - R).max() <= 1e-15
            assert np.abs(ref.to_quaternion(R) - q).max() <= 1e-15


# ---- the header against the reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", list(host.BUILDS))
@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_header_against_reference(executables, build, case):
    """(5) f, s, n within TOL per component, the tensor within TOL max(|s_l|, |s_t|), the same degenerate count."""
    c = ref.case(*case)
    ref.assert_conditions(c.ref)
    got = host.run(executables[build], c.cells, c.h, c.phi_lv, c.phi_rv, c.phi_epi, c.psi, c.axis, np.deg2rad(ref.ANGLES), ref.S_L,
                   ref.S_T, c.active)
    worst = max(np.abs(getattr(got, k) - getattr(c.ref, k)).max() for k in ("f", "s", "n"))
    print(f"header ({build}) vs reference on {case}: max |f, s, n difference| = {worst:.3e}, "
          f"tensor {np.abs(got.M - c.ref.M).max() / max(abs(ref.S_L), abs(ref.S_T)):.3e} (relative to max(s_l, s_t))")
    assert got.count == c.ref.count
    assert worst <= ref.TOL
    assert np.abs(got.M - c.ref.M).max() <= ref.TOL * max(abs(ref.S_L), abs(ref.S_T))
    if c.active is not None:
        assert not got.f[~c.active].any() and not got.s[~c.active].any() and not got.n[~c.active].any() and not got.M[~c.active].any()


@pytest.mark.parametrize("build", list(host.BUILDS))
def test_header_degenerates(executables, build):
    """(5, last) the exact cases of (3) through the header, and each of them within TOL of the reference."""
    cells, h, _, _, _ = ref.slab()

    def solve(lv, rv, epi, angles):
        got = host.run(executables[build], cells, h, lv, rv, epi, None, Z, np.deg2rad(angles), ref.S_L, ref.S_T)
        want = ref.rule(cells, h, lv, rv, epi, Z, angles)
        assert got.count == want.count and np.array_equal(got.f.any(axis=1), want.f.any(axis=1))
        assert _up_to_sign(got.f, want.f) <= ref.TOL  # (these inputs have exact ties between candidates: the sign is not pinned)
        return got

    _check_degenerates(solve)
    flat = np.full(9 * 5 * 5, 0.5)
    act = ref.mask(cells)
    got = host.run(executables[build], cells, h, flat, flat, flat, None, Z, np.deg2rad(ref.ANGLES), ref.S_L, ref.S_T, act)
    assert got.count == int(act.sum()) and not got.f.any() and not got.M[~act].any()
    assert np.array_equal(got.M[act], np.broadcast_to(ref.S_T * np.eye(3), (got.count, 3, 3)))


# ---- the binding against the header ------------------------------------------------------------------------------------------------------

def test_binding_matches_header():
    """(6) beat_fibres_biv_rule's argument list in include/beat_hip.h, type by type and name by name, against beat._hip.SIGNATURES."""
    from beat import _hip

    text = (ROOT / "include" / "beat_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+beat_fibres_biv_rule\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "beat_fibres_biv_rule is not declared"
    scalars = {"double": C.c_double, "int64_t": C.c_int64, "int": C.c_int}
    want, names = [], []
    for arg in (a.strip() for a in m.group(1).split(",")):
        am = re.fullmatch(r"(?:const\s+)?(unsigned\s+char|\w+)\s*(\*?)\s*\b(\w+)(\[3\])?", arg)
        assert am, arg
        ctype, star, name, array = am.groups()
        names.append(name)
        if array:  # a host array of three
            want.append(C.POINTER(scalars[ctype]))
        elif star:  # the context or a device address
            assert ctype == "beat_ctx" or name.startswith("dev_"), arg
            want.append(C.c_void_p)
        else:
            want.append(scalars[ctype])
    res, args = _hip.SIGNATURES["beat_fibres_biv_rule"]
    assert res is C.c_int and args == want, list(zip(names, want))
    assert names == ["ctx", "cells", "h", "dev_phi_lv", "dev_phi_rv", "dev_phi_epi", "dev_psi", "axis", "dev_active", "alpha_endo",
                     "alpha_epi", "beta_endo", "beta_epi", "s_l", "s_t", "dev_f", "dev_s", "dev_n", "dev_M", "dev_degenerate"]


# ---- the refusals, before a device is touched ----------------------------------------------------------------------------------------------

def test_refusals_without_a_device(monkeypatch, caplog):
    """(7) what biv_rule and biv_rule_based do not do is refused before anything asks for a device; more than 90 degrees between
    alpha_endo and alpha_epi is logged and is no error."""
    from beat import _device, fibres
    from beat import grid as g

    def no_device(*a, **k):
        raise AssertionError("a device context was asked for")

    monkeypatch.setattr(_device.Context, "default", classmethod(no_device))
    up = (0.0, 0.0, 1.0)
    box = g.create_box(g.COMM_WORLD, [np.zeros(3), np.ones(3)], [4, 3, 2])
    V = g.functionspace(box, ("P", 1))
    square = g.create_unit_square(g.COMM_WORLD, 4, 4)
    with pytest.raises(ValueError, match="3-D"):
        fibres.biv_rule(square, None, None, None, up)
    with pytest.raises(ValueError, match="3-D"):
        fibres.biv_rule_based(g.functionspace(square, ("P", 1)), None, 1, 2, 3, long_axis=up)

    class TwoRanks(g.Comm):
        rank, size = 0, 2

    split = g.Mesh((4, 3, 4), (0.0,) * 3, (1.0,) * 3, comm=TwoRanks())
    with pytest.raises(NotImplementedError, match="ghost plane"):
        fibres.biv_rule(split, None, None, None, up)
    with pytest.raises(NotImplementedError, match="ghost plane"):
        fibres.biv_rule_based(g.functionspace(split, ("P", 1)), None, 1, 2, 3, long_axis=up)
    per_simplex = g.Mesh((2, 2, 2), (0.0,) * 3, (1.0,) * 3, active=np.arange(48) % 2 == 0)
    with pytest.raises(ValueError, match="per simplex"):
        fibres.biv_rule(per_simplex, None, None, None, up)
    with pytest.raises(ValueError, match="per simplex"):
        fibres.biv_rule_based(g.functionspace(per_simplex, ("P", 1)), None, 1, 2, 3, long_axis=up)

    with pytest.raises(ValueError, match="longitudinal"):
        fibres.biv_rule(box, None, None, None, None)
    for kw in ({}, {"base_marker": 4}, {"apex_facets": [0, 1]}):  # neither a base / apex pair nor an axis
        with pytest.raises(ValueError, match="longitudinal"):
            fibres.biv_rule_based(V, None, 1, 2, 3, **kw)
    for bad in ((0.0, 1.0), np.ones((3, 3)), (0.0, 0.0, 0.0), (0.0, np.nan, 1.0), "up"):
        with pytest.raises(ValueError):
            fibres.biv_rule(box, None, None, None, bad)
        with pytest.raises(ValueError):
            fibres.biv_rule_based(V, None, 1, 2, 3, long_axis=bad)
    for name in ("alpha_endo", "alpha_epi", "beta_endo", "beta_epi"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                fibres.biv_rule(box, None, None, None, up, **{name: bad})
    for fields in ((np.zeros(box.num_nodes), None, None), (None, None, None)):
        with pytest.raises(TypeError, match="P1 function"):
            fibres.biv_rule(box, *fields, up)
    with pytest.raises(TypeError, match="unknown"):
        fibres.biv_rule_based(V, None, 1, 2, 3, long_axis=up, gamma=1.0)

    facets = box.exterior_facets()
    ft = g.meshtags(box, 2, facets[:6], [1, 1, 2, 2, 3, 3])
    for markers, missing in (((7, 2, 3), "endo_lv_marker = 7"), ((1, 7, 3), "endo_rv_marker = 7"), ((1, 2, 7), "epi_marker = 7")):
        with pytest.raises(ValueError, match=f"{missing} tags no facet.*lv_rule_based"):
            fibres.biv_rule_based(V, ft, *markers, long_axis=up)

    # past the rule's limit: logged once, and what is raised afterwards is the next check's refusal, not the angles'
    with caplog.at_level(logging.WARNING, logger="beat.fibres"):
        with pytest.raises(TypeError, match="P1 function"):
            fibres.biv_rule(box, None, None, None, up, alpha_endo=60.0, alpha_epi=-60.0)
        assert [r.levelno for r in caplog.records] == [logging.WARNING] and "90 degrees" in caplog.records[0].getMessage()
        caplog.clear()
        with pytest.raises(TypeError, match="P1 function"):
            fibres.biv_rule(box, None, None, None, up)  # the defaults, 40 and -50, are inside it
        assert not caplog.records
