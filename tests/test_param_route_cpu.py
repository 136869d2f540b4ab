"""beat._param_route: how a solver's cell-model parameters reach the ionic kernel, driven with CPU tensors and a
recording stub in place of the device and the library: for every input the route's kind and data, the exact list of calls, and
that resolving unchanged input again makes none."""

import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from beat import _hip
from beat._param_route import ParameterRoutes, Route
from beat.models._base import DeviceParameters

P, N, MODEL, STRIDE = 20, 40, 3, 24  # parameters, nodes, a shipped model's id, doubles per class in the stub's table


def _tensor(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))  # (a copy, as a device array is)


class Stub:
    """Records the calls ``ParameterRoutes`` makes on the device or in the library; ``jit``: what jit_available answers."""

    torch = torch

    def __init__(self, jit=True):
        self.calls, self.jit = [], jit

    def from_numpy(self, a):
        self.calls.append(("from_numpy", a.shape))
        return _tensor(a)

    def zeros(self, n):
        self.calls.append(("zeros", n))
        return torch.zeros(n, dtype=torch.float64)

    def class_table_doubles(self, model_id):
        self.calls.append(("class_table_doubles", model_id))
        return STRIDE

    def class_table_fill(self, model_id, sets, table):
        assert table.numel() == STRIDE * len(sets)
        self.calls.append(("class_table_fill", model_id, sets.tolist()))

    def jit_available(self):
        self.calls.append(("jit_available",))
        return self.jit

    def take(self):
        calls, self.calls = self.calls, []
        return calls


HOST = SimpleNamespace(torch=torch, from_numpy=_tensor)  # the context a DeviceParameters handle lives in: not recorded


def make(n=N, model_id=MODEL, jit=True, num_parameters=P):
    stub = Stub(jit)
    return ParameterRoutes("model", num_parameters, model_id, n, stub), stub


def uniform(n=N):
    return np.repeat(np.arange(1.0, P + 1.0)[:, None], n, axis=1)


def two_columns(n=N):
    """Rows 1 and 3 differ on the nodes from 17 on: two distinct columns."""
    a = uniform(n)
    a[1, 17:] = 0.5
    a[3, 17:] = 0.0
    return a


def smooth(rows, n=N):
    """``rows`` vary smoothly over the nodes: n distinct columns (more than MAX_CLASSES)."""
    a = uniform(n)
    for r in rows:
        a[r] += np.linspace(0.0, 1.0, n)
    return a


def table_calls(sets):
    return [("class_table_doubles", MODEL), ("zeros", STRIDE * len(sets)), ("class_table_fill", MODEL, np.asarray(sets).tolist())]


def check_classes(route, array, count):
    """The invariant of a classified route: every node's column is the set of the class its byte names, the sets in the order
    torch.unique(dim=1) gives the columns; returns the sets."""
    assert route.kind == "classes" and route.classes[2] == count and route.vector is None and route.rows is None and route.per_node is None
    markers, table, _ = route.classes
    assert markers.dtype == torch.uint8 and markers.shape == (array.shape[1],) and table.numel() == STRIDE * count
    sets = torch.unique(_tensor(array), dim=1).T.numpy()
    assert sets.shape == (count, array.shape[0])
    np.testing.assert_array_equal(sets[markers.numpy()].T, array)
    return sets


def unchanged(routes, stub, p, route):
    assert routes.resolve(p) is route and routes.current is route and stub.calls == []


# ---- None, a vector, errors ---------------------------------------------------------------------------------------------------
def test_none_and_vector_make_no_calls():
    routes, stub = make()
    assert routes.current.kind == "none"
    r = routes.resolve(None)
    assert r == Route("none") and stub.calls == []
    v = np.arange(1.0, P + 1.0)
    r = routes.resolve(v[::1])
    assert r.kind == "uniform" and r.classes is None and r.rows is None and r.per_node is None and r.fallback is None
    assert r.vector.dtype == np.float64 and r.vector.flags.c_contiguous
    np.testing.assert_array_equal(r.vector, v)
    assert stub.calls == []
    r2 = routes.resolve(list(v))  # (a vector is taken as it is at every step: no cache to go stale)
    np.testing.assert_array_equal(r2.vector, v)
    assert stub.calls == [] and routes.current is r2
    strided = np.arange(1.0, 2 * P + 1.0)[::2]
    r3 = routes.resolve(strided)
    assert r3.vector.flags.c_contiguous
    np.testing.assert_array_equal(r3.vector, strided)


def test_wrong_length_or_shape_raises():
    routes, stub = make()
    with pytest.raises(ValueError, match=rf"expected {P} parameters, got {P - 1}"):
        routes.resolve(np.ones(P - 1))
    for shape in ((P, N + 1), (P - 1, N), (P, N, 1), ()):
        with pytest.raises(ValueError, match=re.escape(f"per-node parameters must have shape ({P}, {N}), got {shape}")):
            routes.resolve(np.ones(shape))
    with pytest.raises(ValueError, match=rf"per-node parameters must have shape \({P}, {N}\), got \({P}, {N + 1}\)"):
        routes.resolve(DeviceParameters(np.ones((P, N + 1)), ctx=HOST))
    assert stub.calls == [] and routes.current.kind == "none"


# ---- classes and the class table ----------------------------------------------------------------------------------------------
def test_two_columns_become_two_classes_and_edits_in_place_are_seen():
    routes, stub = make()
    a = two_columns()
    r = routes.resolve(a)
    sets = check_classes(r, a, 2)
    np.testing.assert_array_equal(r.classes[0].numpy(), (np.arange(N) < 17).astype(np.uint8))  # (0.5 sorts before 2.0: the tail is class 0)
    assert stub.take() == [("from_numpy", (P, N))] + table_calls(sets)
    unchanged(routes, stub, a, r)
    # a third column: a new table
    a[7, 30:] = -1.0
    r3 = routes.resolve(a)
    sets3 = check_classes(r3, a, 3)
    assert stub.take() == [("from_numpy", (P, N))] + table_calls(sets3)
    assert r3.classes[1] is not r.classes[1]
    unchanged(routes, stub, a, r3)
    # a value changed, the count did not: the same table, filled once
    a[7, 30:] = -2.0
    r4 = routes.resolve(a)
    sets4 = check_classes(r4, a, 3)
    assert stub.take() == [("from_numpy", (P, N)), ("class_table_fill", MODEL, sets4.tolist())]
    assert r4.classes[1] is r3.classes[1]
    unchanged(routes, stub, a, r4)
    # other nodes, the same sets: the table is neither replaced nor filled
    a[:, 29] = a[:, 30]
    r5 = routes.resolve(a)
    np.testing.assert_array_equal(check_classes(r5, a, 3), sets4)
    assert stub.take() == [("from_numpy", (P, N))] and r5.classes[1] is r3.classes[1]


def test_uniform_columns_are_one_class():
    routes, stub = make()
    a = uniform()
    r = routes.resolve(a)
    check_classes(r, a, 1)
    assert not r.classes[0].any()
    assert stub.take() == [("from_numpy", (P, N))] + table_calls(a[:, :1].T)


# ---- the class limit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_class_limit(extra):
    count = _hip.MAX_CLASSES + extra
    routes, stub = make()
    a = uniform()
    assert N >= count
    a[2, :count - 1] = 100.0 + np.arange(count - 1)[::-1]  # (count - 1 values and the 3.0 of the other nodes)
    assert len(np.unique(a[2])) == count
    r = routes.resolve(a)
    if extra == 0:
        sets = check_classes(r, a, count)
        assert stub.calls == [("from_numpy", (P, N))] + table_calls(sets)
    else:  # one varying row: the sparse-row route
        assert r.kind == "rows" and r.rows[1].tolist() == [2] and r.classes is None
        assert stub.calls == [("from_numpy", (P, N)), ("jit_available",)]


def test_the_full_pass_rejects_what_the_strided_sample_did_not_see():
    n = 200000
    stride = n // 65536
    assert stride == 3
    routes, stub = make(n=n, num_parameters=2)
    a = np.ones((2, n))
    a[1, 1::3] = 1000.0 + np.arange(len(a[1, 1::3]))
    assert len(np.unique(a[1, ::stride])) == 1  # the sample meets one column ...
    r = routes.resolve(a)  # ... the full pass 66668
    assert r.kind == "rows" and r.classes is None and r.rows[1].tolist() == [1]
    assert stub.calls == [("from_numpy", (2, n)), ("jit_available",)]


# ---- varying rows -------------------------------------------------------------------------------------------------------------
ROWS = [0, 2, 3, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19]  # (17 of the 20)


def check_rows(route, array, rows):
    assert route.kind == "rows" and route.classes is None and route.vector is None and route.per_node is None
    uni, idx, dev = route.rows
    assert idx.dtype == np.int32 and idx.flags.c_contiguous and idx.tolist() == rows
    assert tuple(dev.shape) == (len(rows), array.shape[1]) and dev.is_contiguous() and dev.dtype == torch.float64
    np.testing.assert_array_equal(dev.numpy(), array[rows])
    assert uni.dtype == np.float64 and uni.flags.c_contiguous
    np.testing.assert_array_equal(uni, array[:, 0])
    check_per_node(route.fallback, array)


def check_per_node(route, array):
    assert route.kind == "per_node" and route.classes is None and route.rows is None and route.vector is None and route.fallback is None
    tensor, num, ld = route.per_node
    assert (num, ld) == array.shape and tensor.is_contiguous()
    np.testing.assert_array_equal(tensor.numpy(), array)


@pytest.mark.parametrize("k", [1, 4, 5, 16, 17])
def test_varying_rows_with_run_time_compilation(k):
    routes, stub = make(jit=True)
    a = smooth(ROWS[:k])
    r = routes.resolve(a)
    if k <= _hip.MAX_SPARSE_ROWS:
        check_rows(r, a, ROWS[:k])
    else:
        check_per_node(r, a)
    assert stub.take() == [("from_numpy", (P, N)), ("jit_available",)]
    unchanged(routes, stub, a, r)


@pytest.mark.parametrize("k", [4, 5])
@pytest.mark.parametrize("how", ["unavailable", "BEAT_JIT=0"])
def test_varying_rows_without_run_time_compilation(k, how, monkeypatch):
    if how == "BEAT_JIT=0":
        monkeypatch.setenv("BEAT_JIT", "0")
    routes, stub = make(jit=how != "unavailable")
    a = smooth(ROWS[:k])
    r = routes.resolve(a)
    if k <= _hip.MAX_SPARSE_ROWS_RT:
        check_rows(r, a, ROWS[:k])
    else:
        check_per_node(r, a)
    assert stub.take() == [("from_numpy", (P, N))] + ([("jit_available",)] if how == "unavailable" else [])
    unchanged(routes, stub, a, r)


def test_switches_of_the_environment_are_read_at_each_derivation(monkeypatch):
    routes, stub = make()
    monkeypatch.setenv("BEAT_PARAM_SPARSE", "0")
    a = smooth([4])
    r = routes.resolve(a)
    check_per_node(r, a)
    assert stub.take() == [("from_numpy", (P, N))]
    monkeypatch.delenv("BEAT_PARAM_SPARSE")
    a[4, 0] += 1.0
    check_rows(routes.resolve(a), a, [4])
    assert stub.take() == [("from_numpy", (P, N)), ("jit_available",)]
    # few columns, the class analysis off: by the row count
    monkeypatch.setenv("BEAT_PARAM_CLASSES", "0")
    b = two_columns()
    check_rows(routes.resolve(b), b, [1, 3])
    assert stub.take() == [("from_numpy", (P, N)), ("jit_available",)]
    routes, stub = make(jit=False)
    c = two_columns()
    c[[6, 8, 9], 17:] = 0.25  # five varying rows, two columns
    check_per_node(routes.resolve(c), c)
    assert stub.take() == [("from_numpy", (P, N)), ("jit_available",)]
    monkeypatch.delenv("BEAT_PARAM_CLASSES")
    c[6, 17:] = 0.125
    check_classes(routes.resolve(c), c, 2)


def test_a_model_registered_as_source_never_gets_the_sparse_rows():
    for model_id in (_hip.CUSTOM_MODEL_BASE, _hip.CUSTOM_MODEL_BASE + 5):
        routes, stub = make(model_id=model_id)
        a = smooth([4])
        check_per_node(routes.resolve(a), a)
        assert stub.calls == [("from_numpy", (P, N))]
    routes, stub = make(model_id=_hip.CUSTOM_MODEL_BASE - 1)
    check_rows(routes.resolve(a), a, [4])


# ---- switching between inputs -------------------------------------------------------------------------------------------------
def test_array_then_vector_then_the_same_array_classifies_again():
    routes, stub = make()
    a = two_columns()
    r = routes.resolve(a)
    sets = check_classes(r, a, 2)
    stub.take()
    assert routes.resolve(a[:, 0].copy()).kind == "uniform" and stub.calls == []
    r2 = routes.resolve(a)
    check_classes(r2, a, 2)
    assert stub.take() == [("from_numpy", (P, N))] + table_calls(sets)  # (the vector dropped the classes: a table of its own, filled)
    assert routes.resolve(None).kind == "none" and stub.calls == []
    check_classes(routes.resolve(a), a, 2)
    assert stub.take() == [("from_numpy", (P, N))] + table_calls(sets)


def test_array_then_handle_then_the_same_array_derives_each_time():
    routes, stub = make()
    a = two_columns()
    r = routes.resolve(a)
    check_classes(r, a, 2)
    stub.take()
    h = DeviceParameters(a, ctx=HOST)
    rh = routes.resolve(h)
    check_classes(rh, a, 2)
    assert rh is not r and rh.classes[0] is not r.classes[0] and rh.fallback.per_node[0] is h.tensor
    assert stub.take() == [] and rh.classes[1] is r.classes[1]  # (resident values, the same sets: nothing moves, the table stays)
    ra = routes.resolve(a)
    check_classes(ra, a, 2)
    assert ra is not rh and ra.fallback.per_node[0] is not h.tensor
    assert stub.take() == [("from_numpy", (P, N))]
    unchanged(routes, stub, a, ra)


def test_a_handle_is_current_while_it_is_the_same_object_at_the_same_version():
    routes, stub = make()
    a = two_columns()
    h = DeviceParameters(a, ctx=HOST)
    r = routes.resolve(h)
    sets = check_classes(r, a, 2)
    assert stub.take() == table_calls(sets)
    unchanged(routes, stub, h, r)
    h.set_row(9, np.where(np.arange(N) < 30, 10.0, 7.0))
    a[9, 30:] = 7.0
    r2 = routes.resolve(h)
    sets2 = check_classes(r2, a, 3)
    assert stub.take() == table_calls(sets2)
    unchanged(routes, stub, h, r2)
    # another handle with the same version count and other values: not taken for the first
    b = smooth([4, 6])
    h2 = DeviceParameters(b, ctx=HOST)
    h2.set_row(0, b[0])
    assert h2 is not h and h2.version == h.version
    r3 = routes.resolve(h2)
    check_rows(r3, b, [4, 6])
    assert r3.fallback.per_node[0] is h2.tensor and stub.take() == [("jit_available",)]
    unchanged(routes, stub, h2, r3)
    check_classes(routes.resolve(h), a, 3)  # (and back: derived again)
    assert stub.take() == table_calls(sets2)


# ---- classified routes and explicit classes -----------------------------------------------------------------------------------
def test_a_classified_route_carries_its_per_node_fallback():
    routes, stub = make()
    a = two_columns()
    r = routes.resolve(a)
    check_classes(r, a, 2)
    check_per_node(r.fallback, a)
    stub.take()
    hp, num, rows, ld = r.fallback.args()  # (what a step that mirrors another row than the potential launches with)
    assert hp is None and (num, ld) == (P, N) and rows.value == r.fallback.per_node[0].data_ptr()
    unchanged(routes, stub, a, r)


def test_explicit_classes_are_not_resolved():
    routes, stub = make()
    markers = torch.from_numpy((np.arange(N) % 2).astype(np.uint8))
    sets = [np.arange(1.0, P + 1.0), np.arange(2.0, P + 2.0)]
    assert not routes.explicit
    r = routes.set_classes(markers, sets)
    assert routes.explicit and r.kind == "classes" and r.fallback is None and r.classes[0] is markers and r.classes[2] == 2
    assert stub.take() == table_calls(sets)
    for p in (None, sets[0], two_columns(), DeviceParameters(smooth([1]), ctx=HOST), np.ones(3)):
        unchanged(routes, stub, p, r)
    r2 = routes.set_classes(markers, [s.copy() for s in sets])
    assert stub.calls == [] and r2.classes[1] is r.classes[1]
    sets[1][4] = -3.0
    r3 = routes.set_classes(markers, sets)
    assert stub.take() == [("class_table_fill", MODEL, np.asarray(sets).tolist())] and r3.classes[1] is r.classes[1]
    unchanged(routes, stub, None, r3)
    with pytest.raises(ValueError):
        routes.set_classes(markers, [])
    with pytest.raises(ValueError, match=rf"model: {_hip.MAX_CLASSES + 1} parameter sets of \({P},\) values \(expected 1\.\.{_hip.MAX_CLASSES} sets of {P}\)"):
        routes.set_classes(markers, [sets[0]] * (_hip.MAX_CLASSES + 1))
    with pytest.raises(ValueError, match=rf"model: 2 parameter sets of \({P - 1},\) values \(expected 1\.\.{_hip.MAX_CLASSES} sets of {P}\)"):
        routes.set_classes(markers, [s[:-1] for s in sets])
    unchanged(routes, stub, None, r3)


# ---- argument forms -----------------------------------------------------------------------------------------------------------
def _fits(args, argtypes):
    """``args`` as ctypes would take them for ``argtypes``: a pointer is None or a c_void_p, an integer a Python int."""
    assert len(args) == len(argtypes)
    for a, t in zip(args, argtypes):
        if t is C.c_void_p:
            assert a is None or isinstance(a, C.c_void_p)
        else:
            assert t in (C.c_int, C.c_int64) and type(a) is int
    return tuple(a is not None if t is C.c_void_p else a for a, t in zip(args, argtypes))


def test_argument_forms_match_the_prototypes():
    """Every entry point takes (context, model, states, n, ld), the route's parameter arguments, (t, dt, v_index, v_copy) and
    what is its own behind them (_hip.SIGNATURES)."""
    sig = {k: _hip.SIGNATURES[k][1] for k in ("beat_ode_step", "beat_ode_step_pending", "beat_ode_step_rows", "beat_ode_step_classes")}
    assert [len(sig[k]) for k in sig] == [13, 17, 19, 18]
    routes, stub = make()
    a = two_columns()
    v = a[:, 0].copy()
    for route, want in ((routes.resolve(None), (False, 0, False, 0)), (routes.resolve(v), (True, P, False, 0)),
                        (routes.resolve(a).fallback, (False, P, True, N))):
        for name, own in (("beat_ode_step", 0), ("beat_ode_step_pending", 4)):
            assert len(sig[name]) == 5 + 4 + 4 + own
            assert _fits(route.args(), sig[name][5:9]) == want, (route.kind, name)
    u = routes.resolve(v)
    assert u.args()[0].value == u.vector.ctypes.data
    assert u.monitor_kwargs() == dict(host_params=u.vector, per_node=None, classes=None) and u.monitor_kwargs()["host_params"] is u.vector
    c = routes.resolve(a)
    assert _fits(c.args(), sig["beat_ode_step_classes"][5:8]) == (True, 2, True) and len(sig["beat_ode_step_classes"]) == 5 + 3 + 4 + 2 + 4
    assert [p.value for p in c.args()[::2]] == [c.classes[1].data_ptr(), c.classes[0].data_ptr()]
    assert c.monitor_kwargs() == dict(host_params=None, per_node=None, classes=c.classes)
    f = c.fallback
    assert f.args()[2].value == f.per_node[0].data_ptr()
    assert f.monitor_kwargs() == dict(host_params=None, per_node=(f.per_node[0], N), classes=None)
    b = smooth([4, 6])
    s = routes.resolve(b)
    assert _fits(s.args(), sig["beat_ode_step_rows"][5:11]) == (True, P, True, 2, True, N) and len(sig["beat_ode_step_rows"]) == 5 + 6 + 4 + 4
    assert [p.value for p in s.args()[::2]] == [s.rows[0].ctypes.data, s.rows[1].ctypes.data, s.rows[2].data_ptr()]
    assert s.monitor_kwargs() == dict(host_params=None, per_node=(s.fallback.per_node[0], N), classes=None)
    assert Route("none").monitor_kwargs() == dict(host_params=None, per_node=None, classes=None)
