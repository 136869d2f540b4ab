"""CPU: the ``.ode`` expression language of ``beat.models.from_ode`` against an independent evaluation of the same file in mpmath.

tests/data/language_cell.ode holds every construct the generator admits, one per equation (driver states held fixed, probe
states whose increment shows an error in their construct at full size, self-dependent probes whose construct's derivative is
GRL1's J, and states on both sides of GRL1's |J| > 1e-8 switch).  tests/_ode_mp.py interprets the file's syntax with mpmath
numbers -- Python's %, comparisons and and / or on numbers, forward-mode self-derivatives, no SymPy -- and gives each step's
exact value and a running-error magnitude.  Held against it: the generated NumPy evaluation (``numpy_step``) and the generated
C++ struct built for the host with g++ (tests/ode_host_harness.cpp), which is how this suite sees the kernel's C semantics
(fmod, M_PI, the int-valued sign form, the pow overloads, the table-driven exp) without a GPU."""
import ast
import sys
from pathlib import Path

import numpy as np
import pytest

import _ode_mp as M

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
BIG = ROOT / "tests" / "data" / "big_cell.ode"
SCHEMES = ("generalized_rush_larsen", "forward_euler")
DT = 0.5  # (the file's probes decay at k_dec = 2: J dt = -1)
N_RANDOM = 150


@pytest.fixture(scope="module")
def points():
    """The nodes and the mpmath reference, computed once: uniform parameters at t = 0 (the pacing forms' negative dividends) and
    per-node parameters -- period, start, exponent and the five threshold coefficients varied -- at t = 13.7."""
    from beat.models import from_ode

    model = from_ode(M.LANGUAGE_CELL)
    Y = M.language_points(model.state_names, N_RANDOM, seed=1)
    cases = [(M.language_parameters(model), 0.0), (M.language_parameters(model, Y.shape[1], seed=2), 13.7)]
    return model, Y, [(P, t, M.reference(M.LANGUAGE_CELL, Y, P, t, DT, SCHEMES)) for P, t in cases]


def _check(got, Y, ref, names, bound_cr, bound_tr, what):
    """Drivers unchanged; where the reference is not finite the tested side is not finite; elsewhere every probe within its
    bound (in ulp of its running-error magnitude).  Returns the maxima of the two groups."""
    worst, leak = M.compare(got, ref, names)
    assert not leak, (what, "finite where the reference is not", leak[:10])
    for k, s in enumerate(names):
        if s in M.DRIVERS:
            np.testing.assert_array_equal(got[k], Y[k], err_msg=f"{what}: driver {s}")
    bad = {s: v for s, v in worst.items() if v > (bound_cr if s in M.CORRECTLY_ROUNDED else bound_tr)}
    assert not bad, (what, bad)
    return (max(v for s, v in worst.items() if s in M.CORRECTLY_ROUNDED),
            max(v for s, v in worst.items() if s not in M.CORRECTLY_ROUNDED and s not in M.DRIVERS))


def test_language_cell_uses_every_construct_the_generator_admits():
    """The coverage guard: every callable and constant of the generator's name table and every node type its expression check
    admits is used in tests/data/language_cell.ode -- a construct added to the generator without a probe fails here."""
    from beat.models import _ode_parse, from_ode

    tree = ast.parse(M.LANGUAGE_CELL.read_text())
    values = [node.value for node in tree.body if isinstance(node, ast.Assign)]
    used_types = {type(n) for v in values for n in ast.walk(v)}
    used_names = {n.id for v in values for n in ast.walk(v) if isinstance(n, ast.Name)}
    assert set(_ode_parse._EXPR_NODES) - used_types == set()
    assert set(_ode_parse._FUNCTIONS) - used_names == set()
    assert set(_ode_parse._CONSTANTS) - used_names == set()
    assert set(M.FUNCTIONS) == set(_ode_parse._FUNCTIONS)  # (the reference knows each of them, and no more)
    # the parameter given as ScalarParam(value, unit=...) is read as its value
    model = from_ode(M.LANGUAGE_CELL)
    assert model.parameter_defaults["k_dec"] == 2.0 and model.parameter_defaults["period"] == 5.0


@pytest.mark.parametrize("scheme", SCHEMES)
def test_numpy_step_against_mpmath(points, scheme):
    """``numpy_step``, probe by probe (the threshold states included: at J = -1e-8 exactly GRL1's increment differs from Euler's by
    |J| dt / 2 of itself, millions of ulp, so the bounds tell the two updates apart).  Bounds (ulp of the running-error magnitude): 1 for the correctly rounded constructs,
    4 for the transcendental ones and pow (NumPy may take SIMD versions of them).  Measured: 0.57 and 0.41."""
    from beat.models import from_ode

    model, Y, cases = points
    handle = from_ode(M.LANGUAGE_CELL, scheme=scheme)
    for P, t, ref in cases:
        _check(handle.numpy_step(Y, t, P, DT), Y, ref[scheme], model.state_names, 1.0, 4.0, (scheme, t))


@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_generated_cxx_on_the_host_against_mpmath(points, scheme, fast_exp, tmp_path):
    """The generated struct -- the source the device compiles -- built with g++, probe by probe.  Bounds: 1 ulp for the correctly
    rounded constructs, 2 for the transcendental ones and pow (glibc's libm; the table-driven exp is <= 1 ulp).  Measured: 0.41
    and 0.41 with either exp."""
    from beat.models import from_ode

    model, Y, cases = points
    handle = from_ode(M.LANGUAGE_CELL, scheme=scheme, fast_exp=fast_exp)
    run = M.build_host(tmp_path, handle)
    if run is None:
        pytest.skip("no g++ on this machine")
    assert ("beat_mod(" in handle.source) and ("fmod(" in handle.source) and ("M_PI" in handle.source)
    for P, t, ref in cases:
        _check(run(Y, P, t, DT), Y, ref[scheme], model.state_names, 1.0, 2.0, (scheme, fast_exp, t))


def test_mod_is_python_and_numpy_mod_bit_for_bit(tmp_path):
    """``%`` is printed as a helper with Python's meaning (the result takes the divisor's sign; a zero result the divisor's
    sign too): the generated C++ on the host against ``numpy.mod`` bit for bit on finite inputs, and the sign of a zero result
    through 1 / (a % b).  (C's fmod gives the dividend's sign: -1 % 3 is 2 in the model's own language and -1 in fmod.)"""
    from beat.models import from_ode

    f = tmp_path / "mod.ode"
    f.write_text('states("S", a = 1.0, b = 3.0, r = 0.0, w = 0.0)\nexpressions("S")\nda_dt = 0\ndb_dt = 0\n'
                 'dr_dt = a % b\ndw_dt = 1.0/(a % b)\n')
    model = from_ode(f, scheme="forward_euler")
    assert "beat_mod(" in model.source
    assert "beat_mod" not in from_ode(SMALL).source  # (only a model that uses % gets the helper)
    rng = np.random.default_rng(4)
    a = np.concatenate([[-1.0, 1.0, -0.0, 0.0, -6.0, 6.0, -7.5, 7.5, 1e-300, -1e-300, 1e300, -1e300, 5e-324, -5e-324, 3.0, -3.0],
                        rng.uniform(-50, 50, 300), rng.integers(-20, 20, 100).astype(float)])
    b = np.concatenate([[3.0, -3.0, 2.0, -2.0, 3.0, -3.0, 2.5, -2.5, 1.0, -1.0, 7.0, 7.0, 1.0, -1.0, -3.0, 3.0],
                        rng.choice([-1.0, 1.0], 300) * rng.uniform(0.1, 10, 300), rng.choice([-4.0, -2.0, 2.0, 4.0], 100)])
    Y = np.vstack([a, b, np.zeros_like(a), np.zeros_like(a)])
    want = np.mod(a, b)
    with np.errstate(divide="ignore", over="ignore"):
        want_inv = 1.0 / want
    np.testing.assert_array_equal(model.numpy_step(Y, 0.0, model.init_parameter_values(), 1.0)[2], want)
    run = M.build_host(tmp_path, model)
    if run is None:
        pytest.skip("no g++ on this machine")
    got = run(Y, model.init_parameter_values(), 0.0, 1.0)
    np.testing.assert_array_equal(got[2], want)
    np.testing.assert_array_equal(got[3], want_inv)  # +-inf: the zero's sign
    assert got[2][0] == 2.0 and got[2][1] == -2.0


def test_models_without_percent_get_no_mod_helper():
    """The small and the big cell use no ``%``: neither scheme's source, with either exp, names the helper.  (That their sources
    are byte for byte what they were is tests/test_ode_sources_cpu.py's.)"""
    from beat.models import from_ode

    for path in (SMALL, BIG):
        for scheme in SCHEMES:
            for fast in (True, False):
                assert "beat_mod" not in from_ode(path, scheme=scheme, fast_exp=fast).source, (path.name, scheme, fast)


@pytest.mark.parametrize("line, match", [
    ("dV_dt = -floor(V)*0.1", r"bad\.ode:3: dV_dt.*state V"),
    ("dV_dt = -(V % 2.0)", r"bad\.ode:3: dV_dt.*state V"),
    ("dV_dt = -(1.0 % V)", r"bad\.ode:3: dV_dt.*state V"),
    ("dV_dt = -V*((V and 1.0)*1.0)", r"bad\.ode:3: .*`and`"),
    ("dV_dt = -V*((V > 0 or w)*1.0)", r"bad\.ode:3: .*`or`"),
    ("dV_dt = -V*((not w)*1.0)", r"bad\.ode:3: .*`not`"),
    ("dV_dt = -V if V > 0 else V", r"bad\.ode:3: .*IfExp"),
])
def test_constructs_the_generator_cannot_take_are_refused_with_their_line(tmp_path, line, match):
    """What the generator cannot differentiate (floor or % of the state itself: GRL1's J would hold a Derivative no printer
    knows) or does not accept (``and`` / ``or`` / ``not`` of anything but comparisons; Python's conditional expression) is a
    ValueError naming the file and line -- and the state, for a J -- not an error of SymPy's."""
    from beat.models import from_ode

    f = tmp_path / "bad.ode"
    f.write_text(f'states("S", V = 0.5, w = 0.0)\nexpressions("S")\n{line}\ndw_dt = 0\n')
    with pytest.raises(ValueError, match=match):
        from_ode(f)
    if "floor" in line or "%" in line:
        from_ode(f, scheme="forward_euler")  # (forward Euler needs no J: the same file is fine there)
