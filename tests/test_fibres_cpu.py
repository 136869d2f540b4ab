"""CPU: the rule-based fibre rule.  tests/_fibres_ref.py (NumPy, written from the rule's text in include/beat_hip.h) is held to the closed
form of a slab, to the frame's properties and to the exact degenerate cases; csrc/beat_fibres_kernel.h -- the text the kernel runs --
is built with g++ into tests/fibres_host_harness.cpp, once plain and once with the address and undefined-behaviour sanitizers, and held
to the reference; the binding's argument list is held to the header; beat.fibres refuses what it does not do before a device is touched."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _fibres_host as host
import _fibres_ref as ref

ROOT = Path(__file__).resolve().parents[1]


# ---- the reference itself ----------------------------------------------------------------------------------------------------------

def _slab(cells=(8, 4, 4), L=(2.0, 1.0, 1.0)):
    cx, cy, cz = cells
    h = tuple(l / c for l, c in zip(L, cells))
    x = np.tile(np.arange(cx + 1) * h[0], (cz + 1) * (cy + 1))
    z = np.repeat(np.arange(cz + 1) * h[2], (cy + 1) * (cx + 1))
    return cells, h, L, x, z


@pytest.mark.parametrize("alpha", [60.0, -60.0, 0.0, 37.5])
def test_slab_closed_form(alpha):
    """(a) phi = x / Lx and a = (0, 0, 1) on the (8, 4, 4) box: e_t = x, e_c = y, f = (0, cos alpha, sin alpha), s = x for beta = 0."""
    cells, h, L, x, _ = _slab()
    out = ref.rule(cells, h, x / L[0], np.array([0.0, 0.0, 1.0]), (alpha, alpha, 0.0, 0.0))
    a = np.deg2rad(alpha)
    assert out.count == 0
    assert np.abs(out.f - np.array([0.0, np.cos(a), np.sin(a)])).max() <= 1e-15
    assert np.abs(out.s - np.array([1.0, 0.0, 0.0])).max() <= 1e-15
    assert np.abs(out.n - np.array([0.0, -np.sin(a), np.cos(a)])).max() <= 1e-15


@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_frame_properties(case):
    """(b) unit length, mutual orthogonality and f x n = s, to 1e-14, on the random inputs; no degenerate voxel among them."""
    r = ref.case(*case).ref
    ref.assert_well_conditioned(r)
    assert r.count == 0
    act = r.active
    f, s, n = r.f[act], r.s[act], r.n[act]
    for v in (f, s, n):
        assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 1e-14
    for a, b in ((f, s), (f, n), (s, n)):
        assert np.abs((a * b).sum(axis=1)).max() <= 1e-14
    assert np.abs(np.cross(f, n) - s).max() <= 1e-14


def test_exact_degenerates():
    """(c) phi constant over a voxel, and grad phi exactly parallel to the axis: zeros, counted; the tensor is the isotropic s_t I."""
    cells, h, L, x, z = _slab()
    phi = x / L[0]
    nodes = phi.reshape(5, 5, 9)
    nodes[1:3, 2:4, 3:5] = 0.4  # the 8 corners of voxel (3, 2, 1)
    out = ref.rule(cells, h, phi, np.array([0.0, 0.0, 1.0]))
    v = 3 + 8 * (2 + 4 * 1)
    assert out.count == 1 and out.degenerate[v]
    assert not out.f[v].any() and not out.s[v].any() and not out.n[v].any()
    assert np.array_equal(out.M[v], ref.S_T * np.eye(3))
    out = ref.rule(cells, h, z / L[2], np.array([0.0, 0.0, 1.0]))
    assert out.count == 8 * 4 * 4 and not out.f.any() and not out.s.any() and not out.n.any()
    psi = z / L[2]  # ... and a longitudinal field that is constant over a voxel
    psi.reshape(5, 5, 9)[1:3, 2:4, 3:5] = 0.3
    out = ref.rule(cells, h, x / L[0], psi)
    assert out.count == 1 and out.degenerate[v]


def test_transmural_coordinate_is_clipped():
    """(d) nodal values outside [0, 1] (a solve's overshoot): the angles stay those of the endo- / epicardium."""
    cells, h, L, x, _ = _slab()
    axis = np.array([0.0, 0.0, 1.0])
    below = ref.rule(cells, h, x / L[0] - 3.0, axis, (60.0, -60.0, 0.0, 0.0))
    above = ref.rule(cells, h, x / L[0] + 3.0, axis, (60.0, -60.0, 0.0, 0.0))
    a = np.deg2rad(60.0)
    assert np.abs(below.f - np.array([0.0, np.cos(a), np.sin(a)])).max() <= 1e-15
    assert np.abs(above.f - np.array([0.0, np.cos(a), -np.sin(a)])).max() <= 1e-15


def test_inactive_voxels():
    """(e) zeros outside the mask, not counted, and the voxels inside are the full box's."""
    cells = (5, 3, 2)
    full, masked = ref.case(cells, False, False), ref.case(cells, False, True)
    act = masked.active
    assert act.any() and not act.all()
    for name in ("f", "s", "n", "M"):
        got, want = getattr(masked.ref, name), getattr(full.ref, name)
        assert not got[~act].any() and np.array_equal(got[act], want[act]), name
    phi = full.phi.copy()
    phi[:] = 0.5  # every voxel degenerate: only the active ones count
    assert ref.rule(cells, ref.H, phi, np.array(ref.AXIS), ref.ANGLES, act).count == int(act.sum())


# ---- the header against the reference --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    out = tmp_path_factory.mktemp("fibres_host_harness")
    return {name: host.build(out, name) for name in host.BUILDS}


def _through_header(exe, c, angles_deg=ref.ANGLES):
    return host.run(exe, c.cells, c.h, c.phi, c.psi, c.axis, np.deg2rad(angles_deg), ref.S_L, ref.S_T, c.active)


@pytest.mark.parametrize("build", list(host.BUILDS))
@pytest.mark.parametrize("case", ref.CASES, ids=str)
def test_header_against_reference(executables, build, case):
    """(f) f, s, n within 1e-12 per component, the tensor within 1e-12 max(|s_l|, |s_t|), the same degenerate count."""
    c = ref.case(*case)
    ref.assert_well_conditioned(c.ref)
    got = _through_header(executables[build], c)
    worst = max(np.abs(getattr(got, k) - getattr(c.ref, k)).max() for k in ("f", "s", "n"))
    print(f"header ({build}) vs reference on {case}: max |f, s, n difference| = {worst:.3e}, "
          f"tensor {np.abs(got.M - c.ref.M).max() / max(abs(ref.S_L), abs(ref.S_T)):.3e} (relative to max(s_l, s_t))")
    assert got.count == c.ref.count
    assert worst <= ref.TOL
    assert np.abs(got.M - c.ref.M).max() <= ref.TOL * max(abs(ref.S_L), abs(ref.S_T))
    if c.active is not None:
        assert not got.f[~c.active].any() and not got.M[~c.active].any()


@pytest.mark.parametrize("build", list(host.BUILDS))
def test_header_degenerates(executables, build):
    """The exact degenerate cases through the header: zeros, the isotropic tensor, the reference's count."""
    cells, h, L, x, z = _slab()
    rad = np.deg2rad(ref.ANGLES)
    phi = x / L[0]
    phi.reshape(5, 5, 9)[1:3, 2:4, 3:5] = 0.4
    for p, psi, axis in ((phi, None, [0.0, 0.0, 1.0]), (z / L[2], None, [0.0, 0.0, 1.0]), (z / L[2], z / L[2], None), (phi, None, [0.0, 0.0, 0.0])):
        want = ref.rule(cells, h, p, np.array(axis) if psi is None else psi)
        got = host.run(executables[build], cells, h, p, psi, axis, rad, ref.S_L, ref.S_T)
        assert got.count == want.count > 0
        assert np.array_equal(got.f == 0.0, want.f == 0.0) and np.abs(got.f - want.f).max() <= ref.TOL
        assert np.array_equal(got.M[want.degenerate], np.broadcast_to(ref.S_T * np.eye(3), (want.count, 3, 3)))


# ---- the binding against the header ------------------------------------------------------------------------------------------------------

def test_binding_matches_header():
    """(g) beat_fibres_rule's argument list in include/beat_hip.h, type by type, against beat._hip.SIGNATURES."""
    from beat import _hip

    text = (ROOT / "include" / "beat_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+beat_fibres_rule\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "beat_fibres_rule is not declared"
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
    res, args = _hip.SIGNATURES["beat_fibres_rule"]
    assert res is C.c_int and args == want, list(zip(names, want))
    assert names == ["ctx", "cells", "h", "dev_phi", "dev_psi", "axis", "dev_active", "alpha_endo", "alpha_epi", "beta_endo", "beta_epi",
                     "s_l", "s_t", "dev_f", "dev_s", "dev_n", "dev_M", "dev_degenerate"]


# ---- the refusals, before a device is touched ----------------------------------------------------------------------------------------------

def test_refusals_without_a_device(monkeypatch):
    """(h) a 2-D mesh, a decomposed mesh, no longitudinal input, wrong shapes: refused before anything asks for a device."""
    import beat
    from beat import _device, fibres
    from beat import grid as g

    def no_device(*a, **k):
        raise AssertionError("a device context was asked for")

    monkeypatch.setattr(_device.Context, "default", classmethod(no_device))
    assert beat.fibres is fibres and "fibres" in beat.__all__
    box = g.create_box(g.COMM_WORLD, [np.zeros(3), np.ones(3)], [4, 3, 2])
    square = g.create_unit_square(g.COMM_WORLD, 4, 4)
    with pytest.raises(ValueError, match="3-D"):
        fibres.rule_based(square, None, (0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="3-D"):
        fibres.lv_rule_based(g.functionspace(square, ("P", 1)), None, 1, 2, long_axis=(0.0, 0.0, 1.0))

    class TwoRanks(g.Comm):
        rank, size = 0, 2

    split = g.Mesh((4, 3, 4), (0.0,) * 3, (1.0,) * 3, comm=TwoRanks())
    with pytest.raises(NotImplementedError, match="ghost plane"):
        fibres.rule_based(split, None, (0.0, 0.0, 1.0))
    with pytest.raises(NotImplementedError, match="ghost plane"):
        fibres.lv_rule_based(g.functionspace(split, ("P", 1)), None, 1, 2, long_axis=(0.0, 0.0, 1.0))

    with pytest.raises(ValueError, match="longitudinal"):
        fibres.rule_based(box, None, None)
    V = g.functionspace(box, ("P", 1))
    for kw in ({}, {"base_marker": 3}, {"apex_facets": [0, 1]}):  # neither a base / apex pair nor an axis
        with pytest.raises(ValueError, match="longitudinal"):
            fibres.lv_rule_based(V, None, 1, 2, **kw)
    for bad in ((0.0, 1.0), np.ones((3, 3)), (0.0, 0.0, 0.0), (0.0, np.nan, 1.0), "up"):
        with pytest.raises(ValueError):
            fibres.rule_based(box, None, bad)
        with pytest.raises(ValueError):
            fibres.lv_rule_based(V, None, 1, 2, long_axis=bad)
    with pytest.raises(ValueError, match="finite"):
        fibres.rule_based(box, None, (0.0, 0.0, 1.0), alpha_endo=float("nan"))
    with pytest.raises(TypeError, match="P1 function"):
        fibres.rule_based(box, np.zeros(box.num_nodes), (0.0, 0.0, 1.0))
    with pytest.raises(TypeError, match="unknown"):
        fibres.lv_rule_based(V, None, 1, 2, long_axis=(0.0, 0.0, 1.0), gamma=1.0)
    with pytest.raises(NotImplementedError, match="bislerp"):  # two endocardia: the bi-ventricular rule
        fibres.lv_rule_based(V, None, (1, 5), 2, long_axis=(0.0, 0.0, 1.0))
    per_simplex = g.Mesh((2, 2, 2), (0.0,) * 3, (1.0,) * 3, active=np.arange(48) % 2 == 0)
    with pytest.raises(ValueError, match="per simplex"):
        fibres.rule_based(per_simplex, None, (0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="one entry per box cell"):
        g.DeviceCellField(box, np.zeros((5, 3)))
