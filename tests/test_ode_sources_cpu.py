"""CPU: the C++ that ``beat.models.from_ode`` generates, pinned in ONE table: per case the struct's name (its digest is the
key of the compiled kernel's cache) and the SHA-256 of the source.  A change of the generator that is meant to leave its
output alone leaves every entry alone; one that is meant to change it records the table anew (``recorded()``), and the
diff of this file then says which kernels are other kernels.

Cases: every ``.ode`` of tests/data under each scheme (the split files with ``missing="auto"``; ``split_membrane.ode``
without ``missing`` must keep raising), libm's exp for the three files the other suites build with it, small_cell under
GRL2 with the two switches that reorder or rewrite the text (``BEAT_ODE_BRANCHES=1``, ``BEAT_ODE_EMIT=global``), and the
monitor structs the other suites compile."""
import hashlib
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
DATA = ROOT / "tests" / "data"
GRL1, FE, GRL2 = "generalized_rush_larsen", "forward_euler", "generalized_rush_larsen_2"
SWITCHES = {"": {}, "branches": {"BEAT_ODE_BRANCHES": "1"}, "global": {"BEAT_ODE_EMIT": "global"},
            "branches+global": {"BEAT_ODE_BRANCHES": "1", "BEAT_ODE_EMIT": "global"}}
# eight names of big_cell.ode spread over its components (tests/test_monitor_cpu.py compiles the same ones)
BIG_EIGHT = ("I_0", "E_3", "tau_x1_1", "dV_dt", "x5_2_inf", "dc_6_dt", "I_9", "dx11_0_dt")

# (file, scheme, fast_exp, missing, switches) -> (struct name, SHA-256 of the source)
STEP_SOURCES = {
    ("small_cell", GRL1, True, None, ""): ("Ode_small_cell_4a86df8afe8b", "dc7815471a235b46f3c1e2c9a3a8fa7641b056da7c1f57a90c4a44fe016dcbbf"),
    ("small_cell", FE, True, None, ""): ("Ode_small_cell_d16b21dfe508", "cc3543851725af9261c76c404a4f3e7e253cf5abeb1513ed648b9582fd2519a0"),
    ("small_cell", GRL2, True, None, ""): ("Ode_small_cell_341c758268be", "6764d3582e4847b2cea139ac7f078b917ad3f89e1aadf084995b7b2555154b08"),
    ("big_cell", GRL1, True, None, ""): ("Ode_big_cell_1df4f33e4540", "29511b037644b8919c91051d2310a0fd033f49a371bb815b084a7a9084cabdbc"),
    ("big_cell", FE, True, None, ""): ("Ode_big_cell_97d90ec5c42e", "bdbf1255da1ed6d58e95a26af6bbe753277ca2d935397ed14cbd8660b5a5e9df"),
    ("big_cell", GRL2, True, None, ""): ("Ode_big_cell_026710303fd7", "d3528a5b85b0d36a90d844c473cd80af23c4f30e8ac094b3b9d8970612634c40"),
    ("language_cell", GRL1, True, None, ""): ("Ode_language_cell_cc89bdcee1e2", "3a589d34c2dd0364a647a30d7dd3c2f5fe9d9efdcb26c75d120b60d800a44e04"),
    ("language_cell", FE, True, None, ""): ("Ode_language_cell_d3595b55437e", "5d0833fd4e8817ee21456ad5d7d521912695015f6cdce62369e64c5995480c1f"),
    ("language_cell", GRL2, True, None, ""): ("Ode_language_cell_94bcb6208375", "450552edc870f0bd948bc80683d8a712686c14e14f832feaff8f9f2ded963ded"),
    ("split_membrane_as_parameters", GRL1, True, None, ""): ("Ode_split_membrane_as_parameters_45f778e286fd", "fd0ee9a0382795ca0fb8d874440cfb7e9bc2bc47fb16cb73e521f3c1d8be8a0b"),
    ("split_membrane_as_parameters", FE, True, None, ""): ("Ode_split_membrane_as_parameters_de0707cfc372", "f4e1adb8871beb71f7d1ff42591603b24f7deb2d05c739d008b59e203f4e39ab"),
    ("split_membrane_as_parameters", GRL2, True, None, ""): ("Ode_split_membrane_as_parameters_e00f84f46ee9", "4978dd5e9c3fb71f99a4aca42d2aee81ad3236947a00e9f4c85e2b39b458ba0c"),
    ("small_cell", GRL1, False, None, ""): ("Ode_small_cell_d9e4a5c04f23", "a7209c00315f63ddd6063c8dc008815eea6781c40e47fc9b70c279633892358b"),
    ("small_cell", FE, False, None, ""): ("Ode_small_cell_7f7373f51d3a", "51729be0c5b314c8ec56154a825377f72575ebef6a49a0afd9d583880f53215e"),
    ("small_cell", GRL2, False, None, ""): ("Ode_small_cell_46e6713e9f72", "9682e8b29bdfc2afc5ff55370ded364b2e38a903a912c3d5b63f54105a2b941d"),
    ("big_cell", GRL1, False, None, ""): ("Ode_big_cell_00ab91ead402", "1ab965e184e5988353b7bcae5e801e89544861a998c0dc6f71ee24263a7f1934"),
    ("big_cell", FE, False, None, ""): ("Ode_big_cell_2d501dcfaf1b", "48dd22524ea05319d60eb019a59e4dd4b4f6c6f40256e26d8e8d9d70876c2c11"),
    ("big_cell", GRL2, False, None, ""): ("Ode_big_cell_83e5c43ff106", "eae797330995e7ec239ff215695aed507c381fab93f70c4796f234a2ac760056"),
    ("language_cell", GRL1, False, None, ""): ("Ode_language_cell_8c287b3e61ff", "d5a5fe7c73408873652978c041dc089098a863ce41126f153a57e139b2da7434"),
    ("language_cell", FE, False, None, ""): ("Ode_language_cell_99ac8eb1e7c2", "33d9a6caa9d13f8d0b44ab65fc43d2551349ce31c024ab5968be126ae53639f3"),
    ("language_cell", GRL2, False, None, ""): ("Ode_language_cell_93b0f05dc1dd", "c3eb1efbc871054b089d4c9d0fb16206ea1f2210f6ddb4cfe8a1196bb8d11818"),
    ("split_membrane", GRL1, True, "auto", ""): ("Ode_split_membrane_8c05dd640130", "63b8872782c6ab7bc8f18ff7c5f4e7437f2891b387f46019be75e44e38b3f5c0"),
    ("split_membrane", FE, True, "auto", ""): ("Ode_split_membrane_9dc04add5633", "36a996d58b7c5c9bb5aee3f166c9227bef8edefc80ed13b50be7e6af934dab65"),
    ("split_membrane", GRL2, True, "auto", ""): ("Ode_split_membrane_324957d24802", "692d2c906e8acadd2406e7c877cf3d1fa8b80cbc5aa092e955da1594cdd6262f"),
    ("split_calcium", GRL1, True, "auto", ""): ("Ode_split_calcium_d9408dd0c527", "fc7bbdcdf2e6b9b0097cda9f5613592bd635f23eb21803e5f7e518bfed403397"),
    ("split_calcium", FE, True, "auto", ""): ("Ode_split_calcium_64257c07524a", "748aef1ba7126cd47dee054fd571b1ad72f13191f9579a208dd602c26f736375"),
    ("split_calcium", GRL2, True, "auto", ""): ("Ode_split_calcium_fe2ef721cc37", "f156e8655ac03e7b100167109a1f2ac9a831ed7f373f64685275def30109ce2c"),
    ("split_membrane_as_parameters", GRL1, True, "auto", ""): ("Ode_split_membrane_as_parameters_45f778e286fd", "fd0ee9a0382795ca0fb8d874440cfb7e9bc2bc47fb16cb73e521f3c1d8be8a0b"),
    ("split_membrane_as_parameters", FE, True, "auto", ""): ("Ode_split_membrane_as_parameters_de0707cfc372", "f4e1adb8871beb71f7d1ff42591603b24f7deb2d05c739d008b59e203f4e39ab"),
    ("split_membrane_as_parameters", GRL2, True, "auto", ""): ("Ode_split_membrane_as_parameters_e00f84f46ee9", "4978dd5e9c3fb71f99a4aca42d2aee81ad3236947a00e9f4c85e2b39b458ba0c"),
    ("small_cell", GRL2, True, None, "branches"): ("Ode_small_cell_cb5ac7dcabe0", "57e9de18e9a66cf481c7c1e049f59e6bbf04c6a230da48ec86dad9dedb52da08"),
    ("small_cell", GRL2, True, None, "global"): ("Ode_small_cell_dcd6f1f90db0", "79b160a160ef16d1c5374163181145a890c8120fc4b54cb085546b3e00606fb1"),
    ("small_cell", GRL2, True, None, "branches+global"): ("Ode_small_cell_3b93a3fa9b58", "bbf476202515ae9ff170388bca128a0cf47404ac3ae44f97597ab01e1b141d65"),
}

# (file, missing, names: None for all) -> [(struct name, SHA-256 of the source)], one per launch
MONITOR_SOURCES = {
    ("small_cell", None, None): [("Mon_small_cell_cfff45f4ffa8", "4ec70ffbc594c4777c04a5a91cb6eae0de395c7001b9d99a901ee6d9dd7720b9")],
    ("language_cell", None, None): [("Mon_language_cell_3b35c055310c", "d521618e4abe240101911d3cc21d2346896feae9ce41d688fcfedc98222b1e3f"),
                                    ("Mon_language_cell_795938e83d2c", "03016ee8ba24a924953f5f1d6f8fc73d46026b377af819e47a51336fc34d3a19"),
                                    ("Mon_language_cell_bc57a27d1f56", "2bfa574fa4cbc6bd9159893610ce89a9fb9138077b46964b7b1c087231828276")],
    ("big_cell", None, BIG_EIGHT): [("Mon_big_cell_807958bec20c", "870f8f55697c47ad44aa2a177135cc0ca25db83fd6eebee705126f40e82b06a6")],
    ("split_membrane", ("ca",), None): [("Mon_split_membrane_303fbb785910", "4a1b36417c4b783bcc0afadeb414a1b1c59b3fcc717993cdd9ce572e80ec6570")],
}


def step_cases():
    for stem in ("small_cell", "big_cell", "language_cell", "split_membrane_as_parameters"):
        for scheme in (GRL1, FE, GRL2):
            yield stem, scheme, True, None, ""
    for stem in ("small_cell", "big_cell", "language_cell"):
        for scheme in (GRL1, FE, GRL2):
            yield stem, scheme, False, None, ""
    for stem in ("split_membrane", "split_calcium", "split_membrane_as_parameters"):
        for scheme in (GRL1, FE, GRL2):
            yield stem, scheme, True, "auto", ""
    for switches in ("branches", "global", "branches+global"):
        yield "small_cell", GRL2, True, None, switches


def monitor_cases():
    return [("small_cell", None, None), ("language_cell", None, None), ("big_cell", None, BIG_EIGHT), ("split_membrane", ("ca",), None)]


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def step_source(case, setenv):
    from beat.models import from_ode

    stem, scheme, fast_exp, missing, switches = case
    for name, value in SWITCHES[switches].items():
        setenv(name, value)
    model = from_ode(DATA / f"{stem}.ode", scheme=scheme, fast_exp=fast_exp, missing=missing)
    return model.cxx_name, _sha(model.source)


def monitor_source(case):
    from beat.models import from_ode

    stem, missing, names = case
    units = from_ode(DATA / f"{stem}.ode", missing=missing).monitor_sources(None if names is None else list(names))
    return [(name, _sha(source)) for name, source, _ in units]


def recorded():
    """The two tables as this checkout generates them (to record them: print what this returns)."""
    import os

    steps = {}
    for case in step_cases():
        steps[case] = step_source(case, os.environ.__setitem__)
        for name in SWITCHES[case[4]]:
            del os.environ[name]
    return steps, {case: monitor_source(case) for case in monitor_cases()}


def test_the_tables_hold_the_cases():
    assert set(STEP_SOURCES) == set(step_cases()) and set(MONITOR_SOURCES) == set(monitor_cases())
    assert len({name for name, _ in STEP_SOURCES.values()}) == len(set(STEP_SOURCES.values()))  # (one name, one source)


@pytest.mark.parametrize("case", list(step_cases()), ids=lambda c: "-".join(str(v) for v in c))
def test_step_source(case, monkeypatch):
    for name in ("BEAT_ODE_BRANCHES", "BEAT_ODE_EMIT", "BEAT_ODE_V_LAST"):
        monkeypatch.delenv(name, raising=False)
    assert step_source(case, monkeypatch.setenv) == STEP_SOURCES[case]


@pytest.mark.parametrize("case", monitor_cases(), ids=lambda c: c[0])
def test_monitor_source(case, monkeypatch):
    for name in ("BEAT_ODE_BRANCHES", "BEAT_ODE_EMIT", "BEAT_ODE_V_LAST"):
        monkeypatch.delenv(name, raising=False)
    assert monitor_source(case) == MONITOR_SOURCES[case]


@pytest.mark.parametrize("stem", ["split_membrane", "split_calcium"])
def test_a_split_file_without_missing_raises(stem):
    from beat.models import from_ode

    with pytest.raises(ValueError, match=f"{stem}.ode"):
        from_ode(DATA / f"{stem}.ode")
