"""The host half of csrc/beat_rows_kernel.h -- the argument checks and one node's rule, the functions the kernel calls -- compiled
stand-alone with the sanitizers (tests/rows_host_harness.cpp, a program of its own) and run over whole arrays against NumPy."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _rows_cases as cases
from beat import _rows_layout as rl

ROOT = Path(__file__).resolve().parents[1]
SHAPE = (6, 5, 4)
N = 120
# RowsError of the header
OK, NULL, NFIELDS, NCLASSES, BAD_N, CLASS_N, CLASS_LD, CLASS_ROWS, ALIGN, ROW, ROW_TWICE = range(11)


@pytest.fixture(scope="module")
def rows_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path_factory.mktemp("rows_host") / "rows_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe), str(ROOT / "tests" / "rows_host_harness.cpp")], check=True)
    return exe


def _case_text(pb, rows, fill=-1.5, **extra):
    items = {"n": [pb.n], "num_classes": [pb.k], "class_base": pb.base, "class_ld": pb.ld, "class_n": pb.cn, "class_rows": pb.rows,
             "nfields": [len(rows)], "rows": [r for rows_f in rows for r in rows_f], "arena": [pb.arena], "fill": [fill],
             "cls": list(pb.cls), "pos": [] if pb.pos is None else list(pb.pos)}
    items.update(extra)
    return "".join(f"{k} {len(v)} {' '.join(repr(float(x)) if k == 'fill' else str(int(x)) for x in v)}\n" for k, v in items.items())


def _run(exe, mode, text, tmp_path):
    path = tmp_path / "case.txt"
    path.write_text(text)
    run = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    return run.stdout.strip().splitlines()


def _problems():
    out = {}
    for pattern in ("checker", "checker_holes", "thirds"):
        cls = cases.cls_full(cases.markers(SHAPE, pattern))
        out[pattern, "grid"] = cases.shared_problem(rl.grid_layout(cls, 3, 5))
        out[pattern, "compact"] = cases.shared_problem(rl.compact_layout(N, *cases.compact_arrays(cls, 3), 3, 5))
        out[pattern, "markers"] = cases.separate_problem(rl.marker_layout(N, cases.index_lists(cls, 3), (4, 6, 5)))
    return out


PROBLEMS = _problems()


@pytest.mark.parametrize("key", list(PROBLEMS), ids=lambda k: "-".join(k))
def test_whole_arrays_against_numpy(rows_host, tmp_path, key):
    pb = PROBLEMS[key]
    rows = cases.pick_rows(pb, 3, seed=1)
    lines = _run(rows_host, "run", _case_text(pb, rows), tmp_path)
    got = {}
    for line in lines:
        words = line.split()
        if words[0] == "arena":
            got["arena"] = np.array(words[1:], dtype=np.float64)
        else:
            got[words[0], int(words[1])] = np.array(words[2:], dtype=np.float64)
    arena = np.arange(pb.arena, dtype=np.float64)
    prior = [-(1.0 + np.arange(pb.n) + 1000.0 * f) for f in range(3)]
    keep, fill = cases.expand_ref(pb, arena, rows, prior), cases.expand_ref(pb, arena, rows, prior, fill=-1.5)
    for f in range(3):
        np.testing.assert_array_equal(got["keep", f], keep[f])
        np.testing.assert_array_equal(got["fill", f], fill[f])
    fields = [1e7 + 1e5 * f + np.arange(pb.n) for f in range(3)]
    want = cases.collapse_ref(pb, arena, rows, fields)
    np.testing.assert_array_equal(got["arena"], want)
    # (the case says something: some nodes have a source, and where the pattern has holes or the array padding, some elements stay)
    marked = pb.cls < 3
    assert marked.any() and (want != arena).sum() == 3 * marked.sum()
    if key[1] == "compact":
        node_idx, ccls = cases.compact_arrays(cases.cls_full(cases.markers(SHAPE, key[0])), 3)
        for r in range(5):  # padding entries and entries without a model: untouched in every row
            row = want[pb.base[0] + r * pb.ld[0]: pb.base[0] + r * pb.ld[0] + pb.cn[0]]
            np.testing.assert_array_equal(row[ccls >= 3], arena[pb.base[0] + r * pb.ld[0]: pb.base[0] + r * pb.ld[0] + pb.cn[0]][ccls >= 3])


def _codes(exe, tmp_path, pb, rows, addr=None, **extra):
    addr = [4096, 8192, 1 << 20] + [(2 << 20) + 4096 * f for f in range(len(rows))] if addr is None else addr
    lines = _run(exe, "check", _case_text(pb, rows, addr=addr, **extra), tmp_path)
    return {k: int(v) for k, v in (line.split() for line in lines)}


def test_argument_checks(rows_host, tmp_path):
    from copy import deepcopy

    base = PROBLEMS["thirds", "markers"]
    rows = cases.pick_rows(base, 3, seed=2)
    good = [4096, 8192, 1 << 20] + [(2 << 20) + 4096 * f for f in range(3)]
    assert _codes(rows_host, tmp_path, base, rows) == {"plan": OK, "expand": OK, "collapse": OK}
    assert _codes(rows_host, tmp_path, base, rows, addr=[4096, 0] + good[2:])["plan"] == OK  # (no positions: fine)

    # nfields of 0 and 9
    assert _codes(rows_host, tmp_path, base, [])["expand"] == NFIELDS
    nine = [[0, 0, 0]] * 9
    got = _codes(rows_host, tmp_path, base, nine)
    assert got["expand"] == NFIELDS and got["collapse"] == NFIELDS
    big = cases.separate_problem(rl.marker_layout(N, cases.index_lists(base.cls, 3), (8, 9, 8)), S=(8, 9, 8))
    got = _codes(rows_host, tmp_path, big, cases.pick_rows(big, 8))  # (eight is fine)
    assert got["expand"] == OK and got["collapse"] == OK

    # num_classes of 0 and 33
    for k in (0, 33):
        pb = deepcopy(base)
        pb.base, pb.ld, pb.cn, pb.rows = [8] * k, [200] * k, [100] * k, [3] * k
        assert _codes(rows_host, tmp_path, pb, [[0] * k])["plan"] == NCLASSES

    # null and misaligned pointers
    assert _codes(rows_host, tmp_path, base, rows, addr=[0] + good[1:])["plan"] == NULL
    assert _codes(rows_host, tmp_path, base, rows, addr=[4096, 8194] + good[2:])["plan"] == ALIGN
    assert _codes(rows_host, tmp_path, base, rows, addr=good[:2] + [(1 << 20) + 4] + good[3:])["plan"] == ALIGN
    pb = deepcopy(base)
    pb.base[1] = 0  # (with the arena at address 0: a null class_base)
    assert _codes(rows_host, tmp_path, pb, rows, addr=good[:2] + [0] + good[3:])["plan"] == NULL
    got = _codes(rows_host, tmp_path, base, rows, addr=good[:4] + [0] + good[5:])
    assert got["expand"] == NULL and got["collapse"] == NULL
    got = _codes(rows_host, tmp_path, base, rows, addr=good[:5] + [good[5] + 4])
    assert got["expand"] == ALIGN and got["collapse"] == ALIGN
    assert _codes(rows_host, tmp_path, base, rows, null_rows=[1])["expand"] == NULL

    # a row outside [0, class_rows[c])
    for bad in (-1, base.rows[1]):
        r = deepcopy(rows)
        r[2][1] = bad
        got = _codes(rows_host, tmp_path, base, r)
        assert got["plan"] == OK and got["expand"] == ROW and got["collapse"] == ROW
    r = deepcopy(rows)
    r[1][1] = base.rows[1] - 1 if r[1][1] != base.rows[1] - 1 else 0  # the last row is fine
    assert _codes(rows_host, tmp_path, base, r)["expand"] == OK

    # collapse: two fields on one row of a class would race; expand may read a row twice
    r = deepcopy(rows)
    r[2][0] = r[0][0]
    got = _codes(rows_host, tmp_path, base, r)
    assert got["expand"] == OK and got["collapse"] == ROW_TWICE

    # n or a class_n at 2^31; just below is fine
    pb = deepcopy(base)
    pb.n = 2**31
    assert _codes(rows_host, tmp_path, pb, rows)["plan"] == BAD_N
    pb.n = 2**31 - 1
    assert _codes(rows_host, tmp_path, pb, rows)["plan"] == OK
    pb = deepcopy(base)
    pb.cn[2], pb.ld[2] = 2**31, 2**31 + 8
    assert _codes(rows_host, tmp_path, pb, rows)["plan"] == CLASS_N
    pb.cn[2], pb.ld[2] = 2**31 - 1, 2**31 + 8
    assert _codes(rows_host, tmp_path, pb, rows)["plan"] == OK
    pb = deepcopy(base)
    pb.ld[0] = pb.cn[0] - 1
    assert _codes(rows_host, tmp_path, pb, rows)["plan"] == CLASS_LD
    pb = deepcopy(base)
    pb.rows[1] = 0
    assert _codes(rows_host, tmp_path, pb, rows)["plan"] == CLASS_ROWS
