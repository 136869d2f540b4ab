"""Host-side checks of the event maps: the restatement the GPU tests compare the kernel with (tests/_events_ref.py) on courses
worked out by hand, the binding's struct against the header, and what ``beat.EventRecorder`` refuses before it touches a device."""
import ctypes as C
import re
import types
from pathlib import Path

import numpy as np
import pytest

import _events_ref as ref

ROOT = Path(__file__).resolve().parents[1]


def _run(course, mode, strict, thr_up=0.0, thr_down=-50.0):
    V = np.asarray(course, dtype=np.float64).reshape(-1, 1)
    m = ref.new_maps(1)
    for k in range(1, len(V)):
        ref.step(m, V[k - 1], V[k], float(k - 1), float(k), thr_up, thr_down, mode, strict)
    return {k: float(m[k][0]) for k in ref.ALL_MAPS}


def test_restatement_on_hand_made_courses():
    # rest, upstroke between t = 1 and 2, plateau, repolarisation between t = 4 and 5, a second beat between 6 and 7
    course = [-80.0, -80.0, 20.0, 10.0, -40.0, -90.0, -80.0, 30.0]
    m = _run(course, 0, False)
    assert (m["act_first"], m["act_last"], m["repol"], m["apd"]) == (2.0, 7.0, 5.0, 3.0)
    assert (m["dvdt_max"], m["v_max"]) == (110.0, 30.0)
    m = _run(course, 1, False)
    assert m["act_first"] == 1.0 + 80.0 / 100.0 and m["act_last"] == 6.0 + 80.0 / 110.0
    assert m["repol"] == 4.0 + 10.0 / 50.0 and m["apd"] == m["repol"] - m["act_first"]
    # above the threshold when first observed: activated by that step (at its start, in linear mode), not again while it stays
    for mode, t in ((0, 1.0), (1, 0.0)):
        m = _run([5.0, 6.0, 7.0, 8.0], mode, False)
        assert m["act_first"] == t and m["act_last"] == t and np.isnan(m["repol"]) and np.isnan(m["apd"])
    # exactly on the threshold: above for >=, not for >
    assert _run([-1.0, 0.0, 0.0, 1.0], 0, False)["act_first"] == 1.0
    assert _run([-1.0, 0.0, 0.0, 1.0], 0, True)["act_first"] == 3.0
    assert _run([-1.0, 0.0, 0.0, 1.0], 1, True)["act_first"] == 2.0  # vp is not below the threshold: the step's start
    # never activated: no repolarisation either, however often it falls through thr_down
    m = _run([-40.0, -60.0, -40.0, -60.0], 0, False)
    assert all(np.isnan(m[k]) for k in ref.TIME_MAPS) and m["v_max"] == -40.0 and m["dvdt_max"] == 20.0


def test_binding_struct_matches_the_header():
    from beat import _hip

    text = (ROOT / "include" / "beat_hip.h").read_text()
    body = re.search(r"typedef struct beat_event_maps \{(.*?)\} beat_event_maps;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": C.c_double, "int32_t": C.c_int32, "double*": C.c_void_p}
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        typ, names = stmt.split(None, 1)
        if names.startswith("*"):
            typ, names = typ + "*", names[1:]
        declared += [(n.strip(), ctype[typ]) for n in names.split(",")]
    assert declared == list(_hip.EventMaps._fields_)
    assert C.sizeof(_hip.EventMaps) == 2 * 8 + 2 * 4 + 7 * 8


def test_recorder_refuses_before_it_touches_a_device():
    import beat

    def stub(ranks):
        comm = types.SimpleNamespace(size=ranks)
        return types.SimpleNamespace(function_space=types.SimpleNamespace(mesh=types.SimpleNamespace(comm=comm)))

    assert beat.EventRecorder is beat.events.EventRecorder
    with pytest.raises(NotImplementedError):
        beat.EventRecorder(stub(2), 0.0)
    for kw in ({"maps": ("activation", "upstroke")}, {"maps": ("apd",)}, {"maps": ("repolarisation",)}, {"mode": "cubic"},
               {"compare": "<"}, {"maps": ("v_max", "v_max")}):
        with pytest.raises(ValueError):
            beat.EventRecorder(stub(1), 0.0, **kw)


# ---- the kernel's own source on the host (tests/events_host_harness.cpp) ------------------------------------------------------
FAMILIES = {"no_v_prev": ("act_first", "v_max"), "all": ref.ALL_MAPS, "act_first": ("act_first",), "act_last": ("act_last",),
            "repol": ("repol", "act_last"), "apd": ("apd", "act_last"), "dvdt_max": ("dvdt_max",), "v_max": ("v_max",)}
PAD, MARK = 64, 7.25e11


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    import os
    import shutil
    import subprocess

    from beat import _hip

    # the package cannot be built without a host compiler and the HIP headers: their absence is a failure here, not a skip (these
    # are the only checks of the kernel's source that run without a device)
    assert shutil.which("g++") is not None, "g++ not found"
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    assert (rocm / "hip" / "hip_runtime.h").is_file(), f"no HIP headers under {rocm}"
    so = tmp_path_factory.mktemp("events_host") / "libevents_host.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fPIC", "-shared", f"-I{rocm}",
                    "-o", str(so), str(ROOT / "tests" / "events_host_harness.cpp")], check=True)
    lib = C.CDLL(str(so))
    maps_p, vp, dbl, i64 = C.POINTER(_hip.EventMaps), C.c_void_p, C.c_double, C.c_int64
    lib.host_events.argtypes = [i64, C.c_int, vp, maps_p, dbl, dbl, C.c_uint]
    lib.host_flush.argtypes = [i64, vp, vp, vp, i64, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.host_flush_events.argtypes = [i64, C.c_int, vp, maps_p, dbl, dbl, vp, vp, i64, vp, C.c_int, C.c_int, vp, vp, vp, C.c_uint]
    for fn in (lib.host_events, lib.host_flush, lib.host_flush_events):
        fn.restype = None
    return lib


def _padded(n, values):
    a = np.full(n + 2 * PAD, MARK)
    a[PAD:PAD + n] = values
    return a


def _ptr(a, offset=0):
    return a.ctypes.data + 8 * offset


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,shift", [(1, 1), (257, 1), (3150, 54), (3150, 0)])
def test_kernel_source_on_the_host_matches_the_restatement(host_kernel, n, shift, mode, strict):
    """events_kernel as g++ compiles it, over the launch grid lane by lane, on the GPU tests' sequence: every family of maps
    against the restatement -- equal, linear times included (no contraction on either side) --, nothing outside the n nodes
    touched, with the first node 0, 1 and 54 doubles past a 512-byte boundary."""
    from beat import _hip

    V, _ = ref.sequence(n)
    m, _, _ = ref.run(V, mode, bool(strict), t_start=3.0)
    for family, keys in FAMILIES.items():
        arrs = {k: _padded(n, np.nan if k in ref.TIME_MAPS else -np.inf) for k in keys}
        if {"act_last", "dvdt_max"} & set(keys) or (mode == 1 and "act_first" in keys):
            arrs["v_prev"] = _padded(n, V[0])
        v = _padded(n, V[0])
        args = _hip.EventMaps(thr_up=ref.THR_UP, thr_down=ref.THR_DOWN, mode=mode, strict=strict, **{k: _ptr(a, PAD) for k, a in arrs.items()})
        for k in range(1, ref.NSTEPS + 1):
            v[PAD:PAD + n] = V[k]
            t0 = 3.0 + (k - 1) * ref.DT
            host_kernel.host_events(n, shift, _ptr(v, PAD), C.byref(args), t0, t0 + ref.DT, 3)
        for k in keys:
            np.testing.assert_array_equal(arrs[k][PAD:PAD + n], m[k], err_msg=f"{family}: {k}")
        if "v_prev" in arrs:
            np.testing.assert_array_equal(arrs["v_prev"][PAD:PAD + n], V[-1])
        for k, a in list(arrs.items()) + [("v", v)]:
            assert (a[:PAD] == MARK).all() and (a[PAD + n:] == MARK).all(), (family, k)


@pytest.mark.parametrize("case", ["plain", "nothing pending", "order 2", "order 4", "later ring cycle", "guess without directions"])
def test_fused_flush_on_the_host_equals_flush_then_events(host_kernel, case):
    """The kernel's two flush branches against a restatement of x_flush_kernel followed by the plain events pass: x, the guess's d
    and e and every map equal, for the plain update, an update with nothing to apply, the guess's bookkeeping of orders 2 and 4,
    a later ring cycle of the same solve (accumulate) and a guess that rides without any search direction."""
    from beat import _hip

    rng = np.random.default_rng(3)
    n, fld, R, ring_base = 3150, 3150 + 1260, 6, 6
    st = np.zeros(32)
    st[14] = ring_base + (0 if case in ("nothing pending", "guess without directions") else 3)
    alphas, ring = rng.standard_normal(12), rng.standard_normal(6 * fld)
    x0 = -85.0 + 100.0 * rng.random(n)
    g0 = {k: rng.standard_normal(n) for k in ("d", "dp0", "dp1", "e")}
    coef = {"plain": None, "nothing pending": None, "order 2": (2.0, -1.0, 0.0, 0.0), "order 4": (4.0, -1.0, -6.0, 4.0),
            "later ring cycle": (2.0, 0.0, 0.0, 0.0), "guess without directions": (2.0, -1.0, 0.0, 0.0)}[case]
    flags = np.array([1, 1 if case == "later ring cycle" else 0], dtype=np.int32)
    results = []
    for fused in (False, True):
        x, g = x0.copy(), {k: a.copy() for k, a in g0.items()}
        gt = (C.c_void_p * 4)(*([None] * 4 if coef is None else [_ptr(g[k]) for k in ("d", "dp0", "dp1", "e")]))
        cf = np.array(coef or (1.0, 0.0, 0.0, 0.0))
        maps = {k: np.full(n, np.nan if k in ref.TIME_MAPS else -np.inf) for k in ref.ALL_MAPS}
        maps["act_last"][::3] = maps["act_first"][::3] = 0.01
        maps["v_prev"] = -85.0 + 100.0 * np.random.default_rng(5).random(n)
        args = _hip.EventMaps(thr_up=-40.0, thr_down=-50.0, mode=1, strict=0, **{k: _ptr(a) for k, a in maps.items()})
        if fused:
            host_kernel.host_flush_events(n, 54, _ptr(x), C.byref(args), 0.05, 0.1, _ptr(st), _ptr(ring), fld, _ptr(alphas), ring_base, R,
                                          gt, _ptr(cf), _ptr(flags), 3)
        else:
            host_kernel.host_flush(n, _ptr(st), _ptr(x), _ptr(ring), fld, _ptr(alphas), ring_base, R, gt, _ptr(cf), _ptr(flags))
            host_kernel.host_events(n, 54, _ptr(x), C.byref(args), 0.05, 0.1, 3)
        results.append((x, g, maps))
    (xa, ga, ma), (xb, gb, mb) = results
    np.testing.assert_array_equal(xa, xb)
    assert np.array_equal(xa, x0) == (case == "nothing pending")
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k], err_msg=k)
    assert np.array_equal(ga["d"], g0["d"]) == (coef is None)
    for k in ma:
        np.testing.assert_array_equal(ma[k], mb[k], err_msg=k)
    assert np.isfinite(mb["repol"]).any() and (mb["act_last"] >= 0.05).any()  # the step had events of both kinds
    np.testing.assert_array_equal(mb["v_prev"], xb)
