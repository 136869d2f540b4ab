"""CPU: the second-order generalised Rush-Larsen step of ``beat.models.from_ode`` (``scheme="generalized_rush_larsen_2"``).

The two stages in mpmath (tests/_grl2_ref.py, on the independent evaluation of the file in tests/_ode_mp.py) against the NumPy
twin (``numpy_step``) and against the generated C++ struct built for the host; closed forms; the cross-compile for gfx950; the
observed order of the twin on a paced single cell and in a Strang-split cable.  (The sources of every scheme are pinned in
tests/test_ode_sources_cpu.py.)"""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _grl2_ref as R
import _ode_mp as M

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
sys.path.insert(0, str(ROOT))
CSRC = ROOT / "fenicsx-beat_amd" / "csrc"
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
HIPCC = os.environ.get("BEAT_HIPCC") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else shutil.which("hipcc"))
GRL1, GRL2 = "generalized_rush_larsen", "generalized_rush_larsen_2"
DT = 0.5          # tests/test_ode_language_cpu.py's: the language file's probes decay at k_dec = 2
N_RANDOM = 150
SMALL_DT = R.SMALL_DT


@pytest.fixture(scope="module")
def language():
    """The nodes and parameter cases of tests/test_ode_language_cpu.py with the GRL2 reference, computed once."""
    from beat.models import from_ode

    model = from_ode(M.LANGUAGE_CELL, scheme=GRL2)
    Y = M.language_points(model.state_names, N_RANDOM, seed=1)
    cases = [(M.language_parameters(model), 0.0), (M.language_parameters(model, Y.shape[1], seed=2), 13.7)]
    return M.LANGUAGE_CELL, M.CORRECTLY_ROUNDED, DT, Y, [(P, t, R.reference(M.LANGUAGE_CELL, Y, P, t, DT, M.CORRECTLY_ROUNDED)) for P, t in cases]


@pytest.fixture(scope="module")
def small():
    """tests/data/small_cell.ode: uniform parameters inside the stimulus window, per-node parameters outside it.  Every
    equation of the file goes through exp: no state is in the correctly rounded group."""
    from beat.models import from_ode

    model = from_ode(SMALL, scheme=GRL2)
    Y = R.small_points(model)
    cases = [(R.small_parameters(model), 0.9), (R.small_parameters(model, Y.shape[1]), 0.2)]
    return SMALL, (), SMALL_DT, Y, [(P, t, R.reference(SMALL, Y, P, t, SMALL_DT)) for P, t in cases]


def _check(got, Y, ref, names, correctly_rounded, bound_cr, bound_tr, what):
    """tests/test_ode_language_cpu.py's check with the two-stage budget: drivers unchanged; where the reference is not finite the
    tested side is not finite; elsewhere every state within its bound, in ulp of ``_grl2_ref.budgeted``'s magnitude."""
    worst, leak = M.compare(got, R.budgeted(ref, names, correctly_rounded, bound_cr, bound_tr), names)
    print(what, {s: round(v, 3) for s, v in worst.items() if v > 0})
    assert not leak, (what, "finite where the reference is not", leak[:10])
    for k, s in enumerate(names):
        if s in M.DRIVERS:
            np.testing.assert_array_equal(got[k], Y[k], err_msg=f"{what}: driver {s}")
    bad = {s: v for s, v in worst.items() if v > (bound_cr if s in correctly_rounded else bound_tr)}
    assert not bad, (what, bad)


def test_scheme_names():
    from beat.models import from_ode
    from beat.models.ode_file import _SCHEMES

    assert GRL2 in _SCHEMES
    a, b = from_ode(SMALL, scheme=GRL2), from_ode(SMALL, scheme="grl2")
    assert a.scheme == b.scheme == GRL2 and a.source == b.source and a.cxx_name == b.cxx_name
    assert a.cxx_name != from_ode(SMALL).cxx_name and a.name == "small_cell_generalized_rush_larsen_2"
    for bad in ("grl3", "generalized_rush_larsen_3", "rk2"):
        with pytest.raises(ValueError):
            from_ode(SMALL, scheme=bad)


@pytest.mark.parametrize("which", ["language", "small"])
def test_numpy_step_against_mpmath(which, request):
    """``numpy_step`` under GRL2 against the two stages in mpmath.  The budget of state i, derived in tests/_grl2_ref.py:

        eps (K_i m2_i + sum_j |d y'_i / d yh_j| (K_j + 1/2) m1_j)

    K = 1 ulp for the correctly rounded constructs and 4 for the transcendental ones and pow -- the per-step bounds of
    tests/test_ode_language_cpu.py -- m2 the running-error magnitude of stage 2 at the reference's midpoint values, m1 that of
    stage 1, the partial derivatives by central differences in mpmath, the 1/2 for the reference's midpoint values being
    rounded to double."""
    from beat.models import from_ode

    path, cr, dt, Y, cases = request.getfixturevalue(which)
    model = from_ode(path, scheme=GRL2)
    for P, t, ref in cases:
        _check(model.numpy_step(Y, t, P, dt), Y, ref, model.state_names, cr, 1.0, 4.0, (which, t))


def test_first_stage_of_the_twin_is_the_grl1_twin_over_half_a_step(monkeypatch):
    """What the twin's second stage is handed as midpoint values is, bit for bit, ``numpy_step`` of the GRL1 model over dt / 2."""
    from beat.models import from_ode

    two, one = from_ode(M.LANGUAGE_CELL, scheme=GRL2), from_ode(M.LANGUAGE_CELL, scheme=GRL1)
    Y = M.language_points(two.state_names, 30, seed=5)
    P = M.language_parameters(two, Y.shape[1], seed=6)
    seen = []
    real = type(two._twin).update

    def spy(self, y2, args, dt, about=None):
        seen.append(about)
        return real(self, y2, args, dt, about=about)

    monkeypatch.setattr(type(two._twin), "update", spy)
    with np.errstate(all="ignore"):
        two.numpy_step(Y, 13.7, P, DT)
    assert len(seen) == 2 and seen[0] is None
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(seen[1], one.numpy_step(Y, 13.7, P, DT / 2))


@pytest.mark.parametrize("a", [-2.0, 0.7, 2e-8, -2e-8, 1.0000001e-8, 1e-8, 5e-9, -5e-9, 0.0])
def test_linear_equation_is_integrated_exactly(tmp_path, a):
    """x' = a x + c.  Above the switch (|a| > 1e-8) both stages integrate exactly: b = f(xh) + a (x - xh) = a x + c whatever xh
    is, and x' = x + (a x + c) (exp(a dt) - 1) / a is the exponential solution.  Rounding, to first order: exp is within 1 ulp
    and its argument within half an ulp, so exp(a dt) - 1 is off by at most 2 eps max(1, E), E = exp(a dt); b / a has the
    rounding of b's three terms (each at most (|a| |x| + |c|) in size, |xh| < 2 |x| + |c| dt here) and a division; the last sum
    half an ulp of x'.  Budget: 8 eps (|x'| + (|x| + |c / a|) max(1, E)) -- about twice the count.  At and below the switch
    phi is dt: the step is x + (a x + c) dt, which differs from the exponential solution by (a x + c) (phi(a, dt) - dt), at
    most |a x + c| |a| dt^2 (for |a| dt < 1), on top of 8 eps (|x'| + (|a x| + |c|) dt)."""
    import mpmath

    from beat.models import from_ode

    f = tmp_path / "linear.ode"
    f.write_text('parameters("P", a = 1.0, c = 0.3)\nstates("S", x = 0.5)\nexpressions("S")\ndx_dt = a*x + c\n')
    model = from_ode(f, scheme=GRL2)
    assert model._grl == [True]
    x = np.array([0.5, -1.25, 3.0, 1e-3, -0.429])
    eps = 2.0 ** -52
    for c in (0.3, -1.7):
        for dt in (0.5, 0.05):
            got = model.numpy_step(x[None, :], 0.0, model.init_parameter_values(a=a, c=c), dt)[0]
            for xj, gj in zip(x, got):
                with mpmath.workdps(60):
                    am, cm, xm, h = (mpmath.mpf(float(v)) for v in (a, c, xj, dt))
                    E = mpmath.exp(am * h)
                    exact = xm + cm * h if a == 0 else (xm + cm / am) * E - cm / am
                    if abs(a) > 1e-8:
                        budget = 8 * eps * (abs(exact) + (abs(xm) + abs(cm / am)) * max(1, E))
                    else:
                        budget = abs(am * xm + cm) * abs(am) * h * h + 8 * eps * (abs(exact) + (abs(am * xm) + abs(cm)) * h)
                    assert abs(mpmath.mpf(float(gj)) - exact) <= budget, (a, c, dt, xj, gj, float(exact), float(budget))


def test_state_without_self_dependence_follows_the_midpoint_rule(tmp_path):
    """z' = x^2 + time has a self-derivative that is identically zero: z + dt (xh^2 + t + dt / 2) with xh the first stage's value
    of x -- bit for bit, with x's midpoint value taken from the GRL1 twin over dt / 2."""
    from beat.models import from_ode

    f = tmp_path / "midpoint.ode"
    f.write_text('parameters("P", k = 1.5)\nstates("S", x = 0.5, z = 0.25)\nexpressions("S")\ndx_dt = -k*x*x\ndz_dt = x*x + time\n')
    two, one = from_ode(f, scheme=GRL2), from_ode(f, scheme=GRL1)
    assert two._grl == [True, False]
    assert "yh_1 = y_1 + hdt * (" in two.source and "io.store(1, y_1 + dt * (" in two.source
    y = np.array([[0.5, 1.2, -0.3, 2.0], [0.25, -1.0, 0.0, 3.5]])
    p, t, dt = two.init_parameter_values(), 0.3, 0.1
    got = two.numpy_step(y, t, p, dt)
    xh = one.numpy_step(y, t, p, 0.5 * dt)[0]
    np.testing.assert_array_equal(got[1], y[1] + dt * (xh * xh + (t + 0.5 * dt)))
    assert not np.array_equal(got[1], y[1] + dt * (y[0] * y[0] + t))  # (not forward Euler)


@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("which", ["language", "small"])
def test_generated_cxx_on_the_host_against_mpmath(which, fast_exp, request, tmp_path):
    """The generated GRL2 struct -- the source the device compiles -- built with g++ (tests/ode_host_harness.cpp), held to the
    same reference and budget formula with the host build's bounds of tests/test_ode_language_cpu.py: 1 ulp for the correctly
    rounded constructs, 2 for the transcendental ones and pow."""
    from beat.models import from_ode

    path, cr, dt, Y, cases = request.getfixturevalue(which)
    model = from_ode(path, scheme=GRL2, fast_exp=fast_exp)
    run = M.build_host(tmp_path, model)
    if run is None:
        pytest.skip("no g++ on this machine")
    assert ("fexp(" in model.source) == fast_exp and "yh_0" in model.source and "io.load(0)" in model.source
    for P, t, ref in cases:
        _check(run(Y, P, t, dt), Y, ref, model.state_names, cr, 1.0, 2.0, (which, fast_exp, t))


def test_generated_step_loads_each_state_once_and_stores_it_once():
    """y_n comes from the registers loaded at the top of the step (on the fused route the potential's load applies the pending
    update, and the row is overwritten in place): one ``io.load`` and one ``io.store`` per state, every load ahead of the first
    store, and each midpoint value defined once."""
    from beat.models import from_ode

    for path in (SMALL, M.LANGUAGE_CELL, ROOT / "tests" / "data" / "big_cell.ode"):
        model = from_ode(path, scheme=GRL2)
        src = model.source
        for k in range(model.num_states):
            assert src.count(f"io.load({k});") == 1 and src.count(f"io.store({k},") == 1, (path.name, k)
            assert src.count(f"double yh_{k};") + src.count(f"const double yh_{k} =") == 1, (path.name, k)
        assert src.rfind("io.load(") < src.find("io.store(")
        assert src.find("// stage 2") < src.find("io.store(")  # (nothing is stored before every midpoint value exists)


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_generated_grl2_model_compiles_for_gfx950(tmp_path):
    """Every instantiation tests/test_ode_file_cpu.py::test_generated_model_compiles_for_gfx950 lists (uniform parameters without
    and with a pending update, per-node rows, parameter classes, the in-kernel time loop), with its flags, for small_cell
    under GRL2."""
    from beat.models import from_ode

    model = from_ode(SMALL, scheme=GRL2)
    name = model.cxx_name
    flags = [HIPCC, "--genco", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DBEAT_ODE_WAVES=3",
             "-mllvm", "-disable-machine-licm", "-w", f"-I{CSRC}"]
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


def test_order_of_the_twin_on_a_paced_single_cell():
    """small_cell from t = 0 through its own stimulus window (edges at 0.5 and 1.5 ms, on step boundaries) to 3 ms at dt = 0.05,
    0.025, 0.0125 against GRL2 at dt = 0.05 / 128; error: max over states of |difference| / max(|reference|, 1e-3).  Measured:
    GRL1 3.0e-1 / 1.3e-1 / 6.4e-2 (orders 1.16, 1.08), GRL2 2.9e-4 / 9.4e-5 / 2.6e-5 (orders 1.61, 1.83)."""
    from beat.models import from_ode

    def run(scheme, dt):
        model = from_ode(SMALL, scheme=scheme)
        y, p = model.init_state_values(), model.init_parameter_values()
        for j in range(int(round(3.0 / dt))):
            y = model.numpy_step(y, j * dt, p, dt)
        return y

    ref = run(GRL2, 0.05 / 128)
    errors = {s: [float(np.max(np.abs(run(s, dt) - ref) / np.maximum(np.abs(ref), 1e-3))) for dt in (0.05, 0.025, 0.0125)] for s in (GRL1, GRL2)}
    R.assert_second_against_first_order(errors[GRL1], errors[GRL2], "single cell")


def test_order_of_the_twin_in_a_strang_cable():
    """``_grl2_ref.strang_cable``: a 64-cell P1 interval (h = 0.25, conductivity 0.1), theta_pde = theta_split = 0.5, no stimulus,
    V raised to -20 on the first six nodes, 2 ms at the three steps against GRL2 at dt = 0.05 / 64; error: max |difference of V|
    in mV.  Measured: GRL1 6.2 / 3.4 / 1.8 (orders 0.85, 0.91), GRL2 0.99 / 0.29 / 0.068 (orders 1.75, 2.11)."""
    from beat.models import from_ode

    def run(scheme, dt):
        model = from_ode(SMALL, scheme=scheme)
        return R.strang_cable(model, dt, int(round(2.0 / dt)))[model.state_index("V")]

    ref = run(GRL2, 0.05 / 64)
    errors = {s: [float(np.max(np.abs(run(s, dt) - ref))) for dt in (0.05, 0.025, 0.0125)] for s in (GRL1, GRL2)}
    R.assert_second_against_first_order(errors[GRL1], errors[GRL2], "Strang cable")
