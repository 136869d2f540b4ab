"""CPU: missing variables of split cell models in ``beat.models.from_ode(path, missing=...)``: the parser's rules; models
WITHOUT missing variables, which get no input rows (their sources are pinned in tests/test_ode_sources_cpu.py); the NumPy twin of the membrane half of
tests/data/small_cell.ode against mpmath (on the as-parameters form of the same file, tests/_missing_ref.py); one step of the two
halves against one step of the whole model; and the twin's argument checks."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _missing_ref as X
import _ode_mp as M

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
GRL1, FE, GRL2 = X.GRL1, X.FE, X.GRL2
# the twin's bounds of tests/test_ode_language_cpu.py and tests/test_grl2_cpu.py (ulp of the budget's magnitude)
TWIN_CR, TWIN_TR = 1.0, 4.0


# ---------------------------------------------------------------------------------------------------- 1. the parser
def test_explicit_order_is_kept_and_auto_is_sorted():
    from beat.models import from_ode

    a = from_ode(X.CALCIUM, missing=("m", "V", "h"))
    assert a.missing_names == ("m", "V", "h") and a.num_missing_variables == 3
    assert [a.missing_index(nm) for nm in ("m", "V", "h")] == [0, 1, 2]
    with pytest.raises(KeyError):
        a.missing_index("ca")
    b = from_ode(X.CALCIUM, missing="auto")
    assert b.missing_names == ("V", "h", "m")
    assert a.cxx_name != b.cxx_name and a.source != b.source  # (the order decides the rows: another kernel, another cache key)
    assert from_ode(X.MEMBRANE, missing="auto").missing_names == ("ca",)
    assert from_ode(X.SMALL, missing="auto").missing_names == () and from_ode(X.SMALL, missing=()).source == from_ode(X.SMALL).source
    # the states are the file's alone
    assert a.num_states == 1 and a.state_names == ("ca",) and a.state_index("ca") == 0 and a.init_state_values().shape == (1,)
    np.testing.assert_array_equal(a.init_missing_values(), np.zeros(3))
    np.testing.assert_array_equal(a.init_missing_values(V=-84.0, h=0.5), [0.0, -84.0, 0.5])
    with pytest.raises(KeyError):
        a.init_missing_values(ca=1.0)


@pytest.mark.parametrize("missing, offender", [
    (("ca", "V"), "V"),          # a state of the file
    (("ca", "g_out"), "g_out"),  # a parameter
    (("ca", "i_in"), "i_in"),    # an assignment
    (("ca", "lmbda"), "lmbda"),  # used by nothing
    (("ca", "ca"), "ca"),        # twice
    (("ca", "time"), "time"),    # reserved
])
def test_refusals_name_the_file_and_the_name(missing, offender):
    from beat.models import from_ode

    with pytest.raises(ValueError) as err:
        from_ode(X.MEMBRANE, missing=missing)
    assert "split_membrane.ode" in str(err.value) and repr(offender) in str(err.value)


def test_a_split_file_without_missing_still_raises():
    from beat.models import from_ode

    with pytest.raises(ValueError) as err:
        from_ode(X.MEMBRANE)
    assert "split_membrane.ode" in str(err.value) and "ca" in str(err.value)
    with pytest.raises(ValueError):  # (a declared subset leaves the rest undefined)
        from_ode(X.CALCIUM, missing=("V", "m"))
    with pytest.raises(ValueError):
        from_ode(X.MEMBRANE, missing=["ca"], missing_ranges={"V": (0.0, 1.0)})


def test_generated_source_reads_input_rows_and_never_stores_them():
    for scheme in (GRL1, FE, GRL2):
        m = X.membrane(scheme)
        assert "NS = 5," in m.source and "static constexpr int NIN = 1;" in m.source
        assert m.source.count("io.load(4);") == 1 and "io.store(4," not in m.source
        for k in range(4):
            assert m.source.count(f"io.load({k});") == 1 and m.source.count(f"io.store({k},") == 1
        c = X.calcium(scheme)
        assert "NS = 4," in c.source and "NIN = 3;" in c.source and "io.store(0," in c.source
        assert all(f"io.store({k}," not in c.source for k in (1, 2, 3))
    # a monitor selection loads only the rows it uses: i_leak needs no input row, i_out does
    m = X.membrane()
    assert "io.load(4)" not in m._monitor_cxx(["i_leak"])[1] and "io.load(4)" in m._monitor_cxx(["i_out"])[1]
    assert "NIN" not in X.whole().source


# ---------------------------------------------------------------------------------------------------- 2. no drift
def test_models_without_missing_variables_have_no_input_rows():
    """(That their sources are byte for byte what they were is tests/test_ode_sources_cpu.py's.)"""
    from beat.models import from_ode

    for stem in ("small_cell", "language_cell", "big_cell"):
        for scheme in (GRL1, FE, GRL2):
            model = from_ode(X.DATA / f"{stem}.ode", scheme=scheme)
            assert model.num_missing_variables == 0 and model.missing_names == () and model.num_rows == model.num_states


# ---------------------------------------------------------------------------------------------------- 3. the twin against mpmath
@pytest.mark.parametrize("route", ["uniform", "per_node"])
def test_twin_of_the_membrane_half_against_mpmath(route):
    """One step of dt = 0.05 of the membrane half's twin, ``ca`` handed in as a missing variable, against mpmath on the
    as-parameters form: every state within the twin's bound (4 ulp of the running-error magnitude; GRL2: of the two-stage budget
    of tests/_grl2_ref.py) under each scheme."""
    Y, C, P, t, _ = X.membrane_case(route)
    ref = X.membrane_reference(route)
    for scheme in (GRL1, FE, GRL2):
        got = X.membrane(scheme).numpy_step(Y, t, P, X.DT, missing_variables=C)
        assert got.shape == Y.shape
        worst, leak = M.compare(got, X.budget(ref, scheme, TWIN_CR, TWIN_TR), X.MEMBRANE_STATES)
        print(route, scheme, worst)
        assert not leak and max(worst.values()) <= TWIN_TR, (scheme, worst, leak)
    # (M,) is broadcast: node 0 alone with its own value
    one = X.membrane().numpy_step(Y[:, 0], t, P if P.ndim == 1 else P[:, 0], X.DT, missing_variables=C[:, 0])
    np.testing.assert_array_equal(one, X.membrane().numpy_step(Y, t, P, X.DT, missing_variables=C)[:, 0])


def test_monitor_twin_reads_missing_variables():
    from beat.models import from_ode

    m, a = X.membrane(), from_ode(X.AS_PARAMETERS)
    Y, C, P, t, _ = X.membrane_case("uniform")
    got = m.numpy_monitor(Y, t, P, ["i_out", "dV_dt"], missing_variables=C)
    np.testing.assert_array_equal(got, a.numpy_monitor(Y, t, X.as_parameters(P, C), ["i_out", "dV_dt"]))
    assert not np.array_equal(got[0], m.numpy_monitor(Y, t, P, ["i_out"], missing_variables=2.0 * C)[0])


# ---------------------------------------------------------------------------------------------------- 4. the split equals the whole
@pytest.mark.parametrize("scheme", [GRL1, FE])
def test_one_step_of_the_halves_is_one_step_of_the_whole(scheme):
    """Both halves miss only STATES of the other, so a forward-Euler or GRL1 step of the two, each fed the other's step-start
    rows, is mathematically one step of small_cell.ode (no J_kk crosses a missing variable): the five rows against mpmath on
    small_cell.ode, under the twin's bound."""
    import _grl2_ref as R

    w = X.whole(scheme)
    mem, cal = X.membrane(scheme), X.calcium(scheme)
    _, _, Y5 = X.points()
    p = R.small_parameters(w)
    got = X.split_step(mem, cal, Y5, 0.9, X.DT, X.half_parameters(mem, p), X.half_parameters(cal, p))
    ref = M.reference(X.SMALL, Y5, p, 0.9, X.DT)[scheme]
    worst, leak = M.compare(got, ref, w.state_names)
    print(scheme, worst)
    assert not leak and max(worst.values()) <= TWIN_TR, (worst, leak)


def test_grl2_split_differs_from_the_whole_at_second_order():
    """Under GRL2 both stages of a half see the step-start value of a missing variable, where the whole model's second stage
    sees the midpoint value: the one-step difference in V (through ca) and in ca (through V, m, h) is O(dt^2) -- halving dt
    quarters it, within a factor 2.  The steps are dt = 0.001 and 0.0005, not the one-step tests' 0.05: at the random nodes with
    every gate open ca moves by many times its own size over 0.05 ms (|dca/dt| up to 7 per ms against ca >= 3e-5), and the
    expansion in dt this test is about has no leading term there; the ratio tends to 4 as dt falls (measured: 2.4 / 2.2 for V /
    ca at 0.05, 3.1 / 3.9 at 0.001, 3.9 / 4.0 at 1e-5)."""
    import _grl2_ref as R

    w, mem, cal = X.whole(GRL2), X.membrane(GRL2), X.calcium(GRL2)
    _, _, Y5 = X.points()
    p = R.small_parameters(w)
    pm, pc = X.half_parameters(mem, p), X.half_parameters(cal, p)

    def difference(dt):
        d = np.abs(X.split_step(mem, cal, Y5, 0.9, dt, pm, pc) - w.numpy_step(Y5, 0.9, p, dt))
        return {s: float(d[w.state_index(s)].max()) for s in ("V", "ca")}

    d1, d2 = difference(1.0e-3), difference(0.5e-3)
    print("one-step difference", d1, d2)
    for s in ("V", "ca"):
        assert d1[s] > 0.0 and 2.0 <= d1[s] / d2[s] <= 8.0, (s, d1, d2)


# ---------------------------------------------------------------------------------------------------- 5. argument checks
def test_twin_argument_checks():
    m, w = X.membrane(), X.whole()
    y, p = m.init_state_values(), m.init_parameter_values()
    for call in (lambda: m.numpy_step(y, 0.0, p, 0.01), lambda: m.numpy_monitor(y, 0.0, p, ["i_out"]),
                 lambda: m(states=y, t=0.0, parameters=p, dt=0.01)):
        with pytest.raises(TypeError):
            call()
    yw, pw = w.init_state_values(), w.init_parameter_values()
    for call in (lambda: w.numpy_step(yw, 0.0, pw, 0.01, missing_variables=np.zeros(1)),
                 lambda: w.numpy_monitor(yw, 0.0, pw, ["i_out"], missing_variables=np.zeros(1)),
                 lambda: w(states=yw, t=0.0, parameters=pw, dt=0.01, missing_variables=np.zeros(1))):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):  # (M, N) must match the nodes
        m.numpy_step(np.repeat(y[:, None], 3, axis=1), 0.0, p, 0.01, missing_variables=np.zeros((1, 2)))
    assert m.numpy_step(y, 0.0, p, 0.01, missing_variables=np.array([1e-4])).shape == (4,)


def test_sample_states_carry_finite_input_rows():
    c = X.calcium()
    y = c._sample_states(64)
    assert y.shape == (4, 64) and np.isfinite(y).all()
    v = y[1 + c.missing_index("V")]
    assert v.min() >= -100.0 and v.max() <= 60.0 and v.min() < 0.0
    assert (y[2:] >= 0.0).all() and (y[2:] <= 1.0).all()
    out = c._numpy_step_rows(y, 0.0, c.init_parameter_values(), 0.01)
    np.testing.assert_array_equal(out[1:], y[1:])  # (what the self check compares the kernel's untouched input rows with)


# ---------------------------------------------------------------------------------------------------- the cross-compile
HIPCC = os.environ.get("BEAT_HIPCC") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else shutil.which("hipcc"))


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_model_with_input_rows_compiles_for_gfx950(tmp_path):
    """The instantiations tests/test_grl2_cpu.py::test_generated_grl2_model_compiles_for_gfx950 lists, with its flags, for the
    membrane half under GRL2 (NS = 5: four states and an input row): the kernels need no change for a model whose last rows are
    inputs."""
    model = X.membrane(GRL2)
    name, csrc = model.cxx_name, ROOT / "fenicsx-beat_amd" / "csrc"
    flags = [HIPCC, "--genco", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DBEAT_ODE_WAVES=3",
             "-mllvm", "-disable-machine-licm", "-w", f"-I{csrc}"]
    units = {tag: (f"\ntemplate __global__ void ode_step_kernel<{name}, {inst}>(\n    double*, int64_t, int64_t, ParamPack<{name}::NP>, "
                   f"typename {name}::Derived, const double*, int64_t, double, double, int, double*, PendingV, MarkedArgs, SparseRows);\n",
                   b"ode_step_kernel")
             for tag, inst in (("plain", "false, false"), ("pending", "false, true"), ("per_node", "true, true"), ("classes", "false, true, true"))}
    units["run"] = (f"\ntemplate __global__ void ode_run_kernel<{name}, true>(\n    double*, int64_t, int64_t, ParamPack<{name}::NP>, "
                    f"typename {name}::Derived, const double*, int64_t, double, double, int64_t, int, int, TrackSpec, double*);\n", b"ode_run_kernel")
    for tag, (inst, kernel) in units.items():
        unit, out = tmp_path / f"unit_{tag}.hip", tmp_path / f"unit_{tag}.hsaco"
        unit.write_text('#include "beat_ode_kernel.h"\n' + model.source + inst)
        run = subprocess.run(flags + [str(unit), "-o", str(out)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (tag, run.stderr[-3000:])
        names = {s for s in out.read_bytes().split(b"\0") if s.startswith(b"_Z") and kernel in s and b"." not in s}
        assert len(names) == 1, (tag, names)
