"""GPU: the kernel ``beat.models.from_ode`` compiles for tests/data/language_cell.ode -- every construct of the ``.ode``
expression language, one per equation -- against the independent mpmath evaluation of the same file (tests/_ode_mp.py), not
against the generated NumPy evaluation (both of those come from one SymPy tree: a wrong parse would be wrong on both sides).
GRL1 and forward Euler, the table-driven exp and libm's, over random and edge values of the drivers; the threshold states
through per-node parameter rows.  Four models, five run-time compiles (the plain instance of each, the per-node rows of one).

Measured on an MI355X (ulp of each probe's running-error magnitude, largest over the nodes, uniform parameters at t = 0):
correctly rounded constructs 0.39 (GRL1) / 0.41 (Euler), the threshold states the largest; transcendental constructs and pow
0.31 / 0.41, log the largest (r_log), then s_f2 0.22, s_log 0.21, s_f024 / s_atan 0.20 under GRL1 and s_f8 0.33, s_exp 0.33,
s_f15 0.32 under Euler -- the same with the table-driven exp and libm's.  The host build measures 0.41 / 0.41."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

import _ode_mp as M

pytestmark = pytest.mark.gpu
SCHEMES = ("generalized_rush_larsen", "forward_euler")
DT = 0.5
N_RANDOM = 150
# Bounds (ulp of the running-error magnitude), what the host build is held to: the device's divide and sqrt are correctly
# rounded and the table-driven exp is <= 1 ulp (1 for the correctly rounded constructs, measured 0.41); ocml's transcendental
# functions and pow on gfx950 measure as glibc's do here (2, measured 0.41)
BOUND_CR = 1.0
BOUND_TR = 2.0


@pytest.fixture(scope="module")
def points():
    from beat.models import from_ode

    model = from_ode(M.LANGUAGE_CELL)
    Y = M.language_points(model.state_names, N_RANDOM, seed=1)
    cases = [(M.language_parameters(model), 0.0), (M.language_parameters(model, Y.shape[1], seed=2), 13.7)]
    return model, Y, [(P, t, M.reference(M.LANGUAGE_CELL, Y, P, t, DT, SCHEMES)) for P, t in cases]


def _check(got, Y, ref, names, what):
    worst, leak = M.compare(got, ref, names)
    out = os.environ.get("BEAT_ODE_LANGUAGE_REPORT")  # (a file the measured maxima are appended to, for the record above)
    if out:
        with open(out, "a") as fh:
            fh.write(json.dumps({"case": [str(w) for w in what], "worst": worst}) + "\n")
    assert not leak, (what, "finite where the reference is not", leak[:10])
    for k, s in enumerate(names):
        if s in M.DRIVERS:
            np.testing.assert_array_equal(got[k], Y[k], err_msg=f"{what}: driver {s}")
    bad = {s: v for s, v in worst.items() if v > (BOUND_CR if s in M.CORRECTLY_ROUNDED else BOUND_TR)}
    assert not bad, (what, bad)


@pytest.mark.parametrize("fast_exp", [True, False])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_generated_kernel_against_mpmath(hip_ctx, points, scheme, fast_exp):
    """One step of every node, uniform parameters at t = 0, probe by probe; for GRL1 with the table-driven exp also per-node
    parameter rows at t = 13.7 (the threshold coefficients e_k take 0, 5e-9, 1e-8, 1.0000001e-8 and 2e-8 across the nodes:
    at 1e-8 exactly the update must be Euler's -- GRL1's differs from it by millions of ulp there).  Edge nodes: exp overflows to
    inf, a NaN or inf in an unselected Conditional arm stays out of the result, and what is undefined stays non-finite."""
    from beat.models import from_ode

    model, Y, cases = points
    handle = from_ode(M.LANGUAGE_CELL, scheme=scheme, fast_exp=fast_exp, name=f"language_{int(fast_exp)}")
    runs = cases if (scheme == "generalized_rush_larsen" and fast_exp) else cases[:1]
    for P, t, ref in runs:
        if P.ndim == 2:
            # The library holds a variant instance against the plain one at its first launch (csrc/beat_ode_jit.hip), and that
            # check takes two equal infinities for a difference (|inf - inf| is NaN): the rows' first launch is on the random
            # nodes, all finite; the edge nodes follow in the launch checked below.
            handle(states=Y[:, :N_RANDOM], t=t, parameters=P[:, :N_RANDOM], dt=DT)
        got = handle(states=Y, t=t, parameters=P, dt=DT)
        assert got.shape == Y.shape
        _check(got, Y, ref[scheme], model.state_names, (scheme, fast_exp, t, P.ndim))
        k = model.state_index
        a, z, u = Y[k("a")], Y[k("z")], Y[k("u")]
        assert np.isposinf(got[k("s_exp"), a == 800.0]).all() and np.isfinite(got[k("s_exp"), a == -800.0]).all()
        assert np.isfinite(got[k("s_nan")]).all()  # (log / sqrt / asin / exp of the edges sit in arms that are not selected)
        assert np.isnan(got[k("s_log"), z < 0]).all() and np.isnan(got[k("s_asin"), np.abs(u) > 1]).all()
        assert np.isneginf(got[k("s_log"), z == 0]).all()
