"""CPU: the monitored values of a model generated from an ``.ode`` file (``beat.models.from_ode``): names and their order, the
NumPy evaluation ``numpy_monitor`` -- the reference the monitor kernel is held to in tests/test_monitor_gpu.py -- against the
file's formulas written out by hand and against the forward-Euler step, and the emitted monitor translation units compiled for
gfx950.  (The generated texts themselves are pinned in tests/test_ode_sources_cpu.py.)"""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
CSRC = ROOT / "fenicsx-beat_amd" / "csrc"
DATA = ROOT / "tests" / "data"
SMALL = DATA / "small_cell.ode"
HIPCC = os.environ.get("BEAT_HIPCC") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else shutil.which("hipcc"))

# the assignments of small_cell.ode in the order _dependency_order gives them: those that need states and parameters only,
# then those that need the first group, then dca_dt (which needs j_in)
SMALL_NAMES = ("alpha_m", "beta_m", "alpha_h", "beta_h", "n_inf", "tau_n", "i_in", "i_out", "i_leak", "i_stim", "j_pump",
               "dm_dt", "dh_dt", "dn_dt", "dV_dt", "j_in", "dca_dt")
# eight names of big_cell.ode spread over its components (tests/test_monitor_gpu.py monitors the same ones)
BIG_EIGHT = ["I_0", "E_3", "tau_x1_1", "dV_dt", "x5_2_inf", "dc_6_dt", "I_9", "dx11_0_dt"]


def _states(model, n, seed):
    """States on both sides of V = -40 (the branch of alpha_h / beta_h)."""
    rng = np.random.default_rng(seed)
    y = np.repeat(model.init_state_values()[:, None], n, axis=1)
    y[model.state_index("V")] = np.concatenate([rng.uniform(-95.0, -40.5, n // 2), rng.uniform(-39.5, 45.0, n - n // 2)])
    for g in ("m", "h", "n"):
        y[model.state_index(g)] = rng.uniform(0.0, 1.0, n)
    y[model.state_index("ca")] = 10.0 ** rng.uniform(-4.5, -2.5, n)
    return y


def test_monitor_names_are_the_assignments_in_dependency_order():
    from beat.models import from_ode

    model = from_ode(SMALL)
    assert model.monitor_names == SMALL_NAMES
    assert {f"d{s}_dt" for s in model.state_names} <= set(model.monitor_names)
    for k, name in enumerate(model.monitor_names):
        assert model.monitor_index(name) == k
    with pytest.raises(KeyError, match="Unknown monitor"):
        model.monitor_index("i_nope")
    with pytest.raises(KeyError, match="Unknown monitor"):
        model.numpy_monitor(model.init_state_values(), 0.0, model.init_parameter_values(), ["i_in", "V"])  # a state is no assignment


def test_numpy_monitor_equals_the_formulas_of_the_file():
    """i_in, i_out, i_stim, alpha_h, beta_h and j_pump as tests/data/small_cell.ode writes them, to 1e-14 relative, on both
    sides of V = -40 and with t outside (0.2, 1.6) and inside (0.5, 1.0, 1.5: both ends belong to it) the stimulus window."""
    from beat.models import from_ode

    model = from_ode(SMALL)
    y = _states(model, 200, 7)
    V, m, h, n, ca = y
    assert (V < -40).any() and (V > -40).any()
    p = model.init_parameter_values(stim_amplitude=30.0)
    P = dict(zip(model.parameter_names, p))
    names = ["i_in", "i_out", "i_stim", "alpha_h", "beta_h", "j_pump"]
    for t in (0.2, 0.5, 1.0, 1.5, 1.6):
        got = dict(zip(names, model.numpy_monitor(y, t, p, names)))
        want = {
            "i_in": P["g_in"] * m**3 * h * (V - P["E_in"]),
            "i_out": P["g_out"] * n * np.sqrt(np.abs(ca) / P["ca_rest"]) * (V - P["E_out"]),
            "i_stim": np.full_like(V, P["stim_amplitude"] if P["stim_start"] <= t <= P["stim_start"] + P["stim_duration"] else 0.0),
            "alpha_h": np.where(V < -40, 0.135 * np.exp(-(V + 80) / 6.8), 0.0),
            "beta_h": np.where(V < -40, 3.56 * np.exp(0.079 * V) + 310000 * np.exp(0.35 * V), 1 / (0.13 * (1 + np.exp(-(V + 10.66) / 11.1)))),
            "j_pump": P["v_pump"] * ca**2 / (ca**2 + P["K_pump"] ** 2),
        }
        for nm in names:
            err = np.abs(got[nm] - want[nm]) / np.maximum(np.abs(want[nm]), 1e-300)
            assert err.max() <= 1e-14, (nm, t, err.max())
    assert model.numpy_monitor(y, 1.0, p, ["i_stim"]).max() == 30.0 and model.numpy_monitor(y, 0.2, p, ["i_stim"]).max() == 0.0
    # (S,) states give (M,)
    one = model.numpy_monitor(y[:, 3], 1.0, p, names)
    np.testing.assert_array_equal(one, model.numpy_monitor(y, 1.0, p, names)[:, 3])


def test_numpy_monitor_rates_are_what_the_forward_euler_step_integrates():
    """y + dt * d<state>_dt == numpy_step(y, t, p, dt) of the forward-Euler model to 1e-15 max(|y|, |dt row|), with (P,) and
    with (P, N) parameters."""
    from beat.models import from_ode

    model = from_ode(SMALL, scheme="forward_explicit_euler")
    n, dt = 300, 0.02
    y = _states(model, n, 11)
    rates = [f"d{s}_dt" for s in model.state_names]
    p1 = model.init_parameter_values(stim_amplitude=30.0)
    pn = np.repeat(p1[:, None], n, axis=1)
    pn[model.parameter_index("g_in")] *= np.linspace(0.5, 1.5, n)
    pn[model.parameter_index("E_out")] += np.linspace(-5.0, 5.0, n)
    for p in (p1, pn):
        for t in (0.2, 1.0):
            rows = model.numpy_monitor(y, t, p, rates)
            assert rows.shape == (model.num_states, n)
            new = model.numpy_step(y, t, p, dt)
            assert (np.abs(y + dt * rows - new) <= 1e-15 * np.maximum(np.abs(y), np.abs(dt * rows))).all(), t
    # the per-node evaluation is the (P,) one column by column
    whole = model.numpy_monitor(y, 1.0, pn)
    for j in (0, 17, n - 1):
        np.testing.assert_allclose(whole[:, j], model.numpy_monitor(y[:, j], 1.0, pn[:, j]), rtol=1e-14, atol=0.0)
    with pytest.raises(ValueError):
        model.numpy_monitor(y, 1.0, pn[:, :5])


def test_a_selection_gives_the_rows_of_all_names():
    from beat.models import from_ode

    model = from_ode(SMALL)
    y = _states(model, 64, 2)
    p = model.init_parameter_values()
    full = model.numpy_monitor(y, 0.7, p)
    assert full.shape == (len(SMALL_NAMES), 64)
    np.testing.assert_array_equal(model.numpy_monitor(y, 0.7, p, names=None), full)
    pick = ["dca_dt", "i_in", "tau_n", "dV_dt", "i_in"]  # any order, a name twice
    np.testing.assert_array_equal(model.numpy_monitor(y, 0.7, p, pick), full[[model.monitor_index(nm) for nm in pick]])
    np.testing.assert_array_equal(model.numpy_monitor(y, 0.7, p, "j_pump"), full[[model.monitor_index("j_pump")]])


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
@pytest.mark.parametrize("stem,names", [("small_cell", None), ("language_cell", None), ("big_cell", BIG_EIGHT)])
def test_monitor_units_compile_for_gfx950(tmp_path, stem, names):
    """The translation unit the library writes for a selection -- beat_ode_kernel.h, the struct, an instantiation -- with the
    plain, the per-node and the class instance in one unit; a list longer than _hip.MAX_MONITORS comes as several structs."""
    from beat import _hip
    from beat.models import from_ode

    model = from_ode(DATA / f"{stem}.ode")
    units = model.monitor_sources(names)
    want = list(model.monitor_names) if names is None else names
    assert [nm for _, _, run in units for nm in run] == want
    assert len(units) == -(-len(want) // _hip.MAX_MONITORS) and all(len(run) <= _hip.MAX_MONITORS for _, _, run in units)
    for k, (name, source, run) in enumerate(units):
        assert name.startswith(f"Mon_{stem}_") and f"struct {name}" in source and f"NM = {len(run)}" in source
        assert "io.store" not in source  # read-only: the struct has no way to write a state
        inst = "".join(f"template __global__ void ode_monitor_kernel<{name}, {per_node}, {marked}>(\n    const double*, int64_t, int64_t, "
                       f"ParamPack<{name}::NP>, const double*, int64_t, MarkedArgs, int, double, double*, int64_t);\n"
                       for per_node, marked in (("false", "false"), ("true", "false"), ("false", "true")))
        unit = tmp_path / f"unit_{k}.hip"
        unit.write_text('#include "beat_ode_kernel.h"\n' + source + inst)
        out = tmp_path / f"unit_{k}.hsaco"
        run_ = subprocess.run([HIPCC, "--genco", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-DBEAT_ODE_WAVES=3",
                               "-mllvm", "-disable-machine-licm", "-w", f"-I{CSRC}", str(unit), "-o", str(out)],
                              capture_output=True, text=True, timeout=600)
        assert run_.returncode == 0, run_.stderr[-3000:]
        kernels = {s for s in out.read_bytes().split(b"\0") if s.startswith(b"_Z") and b"ode_monitor_kernel" in s and b"." not in s}
        assert len(kernels) == 3, kernels


def test_a_selection_loads_only_what_it_uses():
    """j_pump needs ca, v_pump and K_pump: one state row and two parameters are read, nothing else."""
    from beat.models import from_ode

    model = from_ode(SMALL)
    (name, source, run), = model.monitor_sources(["j_pump"])
    assert run == ("j_pump",)
    assert [ln.strip() for ln in source.splitlines() if "io.load" in ln] == [f"const double y_{model.state_index('ca')} = io.load({model.state_index('ca')});"]
    assert sorted(int(ln.split("p[")[1].split("]")[0]) for ln in source.splitlines() if "= p[" in ln) == sorted(
        [model.parameter_index("v_pump"), model.parameter_index("K_pump")])
    # the same selection gives the same struct (the library keys the compiled kernel on it)
    assert model.monitor_sources(["j_pump"])[0][:2] == (name, source)
    assert from_ode(SMALL).monitor_sources(["j_pump"])[0][:2] == (name, source)


def test_shipped_models_and_the_host_have_no_device_monitor():
    from beat.models import from_ode, tp06

    with pytest.raises(NotImplementedError, match="from_ode"):
        tp06.generalized_rush_larsen.monitor_values(0.0, tp06.init_state_values(), tp06.init_parameter_values())
    import torch

    if not torch.cuda.is_available():  # without a GPU monitor_values is numpy_monitor, as __call__ is numpy_step
        model = from_ode(SMALL)
        y = _states(model, 16, 1)
        np.testing.assert_array_equal(model.monitor_values(1.0, y, model.init_parameter_values(), ["i_in"]),
                                      model.numpy_monitor(y, 1.0, model.init_parameter_values(), ["i_in"]))
