"""CPU: the stages of the generator behind ``beat.models.from_ode``, one at a time: what each module may import
(``_ode_parse`` no SymPy; ``_ode_symbolic``, ``_ode_cxx`` and ``_ode_numpy`` neither torch nor the HIP library), what the parser
returns for tests/data/small_cell.ode, and the one stage writer of the C++ text serving GRL1 and GRL2's second stage alike."""
import importlib
import re
import sys
import types
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
MODELS = ROOT / "fenicsx-beat_amd" / "beat" / "models"
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
GRL1, GRL2 = "generalized_rush_larsen", "generalized_rush_larsen_2"
# the assignments of small_cell.ode in dependency order (tests/test_monitor_cpu.py's SMALL_NAMES)
SMALL_NAMES = ("alpha_m", "beta_m", "alpha_h", "beta_h", "n_inf", "tau_n", "i_in", "i_out", "i_leak", "i_stim", "j_pump",
               "dm_dt", "dh_dt", "dn_dt", "dV_dt", "j_in", "dca_dt")


@pytest.fixture
def bare(monkeypatch):
    """``bare(name, *blocked)``: beat/models/<name>.py imported afresh as a module of a package that holds that directory and
    nothing else -- no ``beat`` above it, so ``from .. import _hip`` cannot work -- while ``import <blocked>`` fails."""
    package = types.ModuleType("bare_models")
    package.__path__ = [str(MODELS)]
    monkeypatch.setitem(sys.modules, "bare_models", package)

    def load(name, *blocked):
        for module in blocked:
            monkeypatch.setitem(sys.modules, module, None)
        return importlib.import_module(f"bare_models.{name}")

    yield load
    for name in [nm for nm in sys.modules if nm.startswith("bare_models.")]:
        del sys.modules[name]


def test_the_parser_needs_no_sympy(bare):
    parse = bare("_ode_parse", "sympy", "torch")
    source = parse.parse_ode(SMALL)
    assert source.path == SMALL and source.missing_names == ()
    assert source.states == {"V": -84.0, "m": 0.002, "h": 0.98, "n": 0.01, "ca": 0.0001}
    assert list(source.states) == ["V", "m", "h", "n", "ca"]
    assert source.parameters == {"Cm": 1.0, "g_in": 12.0, "g_out": 0.9, "g_leak": 0.05, "E_in": 55.0, "E_out": -90.0, "E_leak": -70.0,
                                 "k_ca": 0.004, "ca_rest": 0.0001, "v_pump": 0.02, "K_pump": 0.0005,
                                 "stim_amplitude": 25.0, "stim_start": 0.5, "stim_duration": 1.0}
    assert list(source.parameters)[:2] == ["Cm", "g_in"] and list(source.parameters)[-1] == "stim_duration"
    assert tuple(name for name, _ in source.assignments) == SMALL_NAMES
    with pytest.raises(Exception):  # (frozen)
        source.states = {}


@pytest.mark.parametrize("name", ["_ode_symbolic", "_ode_cxx", "_ode_numpy"])
def test_the_generator_needs_neither_torch_nor_the_library(bare, name):
    module = bare(name, "torch")
    assert not any(nm in sys.modules for nm in ("bare_models._hip", "bare_models._base", "bare_models.ode_file"))
    system = module.OdeSystem.from_source(bare("_ode_parse").parse_ode(SMALL), GRL1)
    assert [str(s) for s in system.y] == ["V", "m", "h", "n", "ca"] and system.grl == [True] * 5 and tuple(system.assigned) == SMALL_NAMES


def test_one_stage_writer_writes_grl1_and_the_second_stage_of_grl2():
    """On small_cell, the lines of GRL1 over ``dt`` are, line for line, those of GRL2's second stage with b = f once yh_k reads
    y_k, xh_k reads x_k and th reads t: a stage is written in one place.  (The second stage here continues a first stage that
    has written nothing, so it defines the parameter-only temporaries itself, as GRL1 does.)"""
    from beat.models._ode_cxx import CxxOptions, _Body, _stage
    from beat.models._ode_parse import parse_ode
    from beat.models._ode_symbolic import OdeSystem

    opt = CxxOptions(fast_exp=True, branches=False, emit_global=False, v_last=True)
    order = [1, 2, 3, 4, 0]
    one_system, two_system = (OdeSystem.from_source(parse_ode(SMALL), scheme) for scheme in (GRL1, GRL2))
    one = _Body(one_system, one_system.repl, opt)
    _stage(one, order, "dt", about=False, store=True)
    second = _Body(two_system, two_system.repl, opt, second_of=_Body(two_system, two_system.repl, opt))
    _stage(second, order, "dt", about=False, store=True)
    assert any("yh_0" in ln for ln in second.lines) and any("xh_" in ln for ln in second.lines) and any(re.search(r"\bth\b", ln) for ln in second.lines)
    assert [re.sub(r"\bth\b", "t", ln.replace("yh_", "y_").replace("xh_", "x_")) for ln in second.lines] == one.lines
    assert sum(ln.count("io.store(") for ln in one.lines) == 5
