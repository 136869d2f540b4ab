"""CPU: how an instance compiled at run time is held against its reference instance (csrc/beat_jit_check.h: the comparison of the
two results row by row, and the switch BEAT_JIT_SELF_CHECK), built with g++ into tests/jit_check_harness.cpp -- once plain, once with
the address and undefined-behaviour sanitizers -- and driven line by line.  Every case runs with both tolerance pairs in use:
1e-9 / 1e-12 (a sparse-row instance against the run-time-index kernel) and 1e-10 / 1e-13 (a variant instance of a generated model
against its plain instance).  A value passes when |x - y| <= rtol |y| + atol S, S the largest finite |y| below 1e300 of its row."""
import math
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O1", "-Wall", "-Werror"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
TOLERANCES = [(1e-9, 1e-12), (1e-10, 1e-13)]
NAN, INF = math.nan, math.inf


@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    out = tmp_path_factory.mktemp("jit_check_harness")
    exes = {}
    for name, flags in BUILDS.items():
        exes[name] = out / f"jit_check_{name}"
        subprocess.run(["g++", "-std=c++17", *flags, f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exes[name]),
                        str(ROOT / "tests" / "jit_check_harness.cpp")], check=True)
    return exes


class Harness:
    """One child process; compare(a, b, rtol, atol) -> None when the rows agree, else (row, node, x, y) of the mismatch reported."""

    def __init__(self, exe):
        self.p = subprocess.Popen([str(exe)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)

    def call(self, command):
        self.p.stdin.write(command + "\n")
        self.p.stdin.flush()
        words = self.p.stdout.readline().split()
        assert words and words[0] == command.split()[0], (command, words, self.p.stderr.read() if self.p.poll() is not None else "")
        return dict(w.split("=") for w in words[1:])

    def compare(self, a, b, rtol, atol):
        assert len(a) == len(b) and all(len(ra) == len(rb) == len(a[0]) for ra, rb in zip(a, b))
        flat = [float(v).hex() for rows in (a, b) for row in rows for v in row]
        got = self.call(f"compare {len(a)} {len(a[0])} {float(rtol).hex()} {float(atol).hex()} " + " ".join(flat))
        if got["ok"] == "1":
            return None
        return int(got["row"]), int(got["node"]), float.fromhex(got["x"]), float.fromhex(got["y"])

    def close(self):
        _, err = self.p.communicate(timeout=60)
        assert self.p.returncode == 0 and err == "", err  # (a sanitizer reports on stderr and fails the process)


@pytest.fixture(params=list(BUILDS))
def harness(executables, request):
    h = Harness(executables[request.param])
    yield h
    h.close()


def _rows(rows=3, nc=9):
    """rows x nc values of mixed sign and size, nc no multiple of 8; row k has the scale 10^k (its node 0)."""
    return [[10.0**k] + [(-1) ** i * 10.0**k * (i + 1) / (nc + 1) for i in range(1, nc)] for k in range(rows)]


@pytest.mark.parametrize("rtol,atol", TOLERANCES)
def test_equal_arrays_pass(harness, rtol, atol):
    b = _rows()
    assert harness.compare([row[:] for row in b], b, rtol, atol) is None
    for v in (0.0, -0.0, 1.0, -3.5e-300, 1e299, 2e305):  # one row of one node
        assert harness.compare([[v]], [[v]], rtol, atol) is None, v
    assert harness.compare([[1.0]], [[2.0]], rtol, atol) == (0, 0, 1.0, 2.0)


@pytest.mark.parametrize("rtol,atol", TOLERANCES)
def test_nan(harness, rtol, atol):
    """NaN on both sides of a pair passes (a caller's garbage in, the same garbage out); NaN against a number fails, whichever side
    holds it -- the comparison is written !(... <= ...)."""
    a, b = _rows(), _rows()
    a[1][4] = b[1][4] = NAN
    assert harness.compare(a, b, rtol, atol) is None
    assert harness.compare([[NAN]], [[NAN]], rtol, atol) is None
    a, b = _rows(), _rows()
    a[1][4] = NAN
    got = harness.compare(a, b, rtol, atol)
    assert got[:2] == (1, 4) and math.isnan(got[2]) and got[3] == b[1][4]
    a, b = _rows(), _rows()
    b[2][8] = NAN
    got = harness.compare(a, b, rtol, atol)
    assert got[:2] == (2, 8) and got[2] == a[2][8] and math.isnan(got[3])


@pytest.mark.parametrize("rtol,atol", TOLERANCES)
def test_half_the_bound_passes_twice_the_bound_fails(harness, rtol, atol):
    """x = y +- factor (rtol |y| + atol S): on the row's largest value (S = |y|), on a value far below the row's scale (the atol
    term alone decides) and on a zero among non-zeros."""
    for k, i in ((0, 0), (2, 0), (1, 3), (2, 8)):
        for y in (None, 1e-9, 0.0):
            for sign in (1.0, -1.0):
                b = _rows()
                if y is not None:
                    b[k][i] = y
                scale = max(abs(v) for v in b[k])
                bound = rtol * abs(b[k][i]) + atol * scale
                for factor, passes in ((0.5, True), (2.0, False)):
                    a = [row[:] for row in b]
                    a[k][i] = b[k][i] + sign * factor * bound
                    assert a[k][i] != b[k][i]
                    got = harness.compare(a, b, rtol, atol)
                    assert got == (None if passes else (k, i, a[k][i], b[k][i])), (k, i, y, sign, factor)


@pytest.mark.parametrize("rtol,atol", TOLERANCES)
def test_the_scale_is_the_largest_finite_reference_value_below_1e300(harness, rtol, atol):
    """NaN, inf and values >= 1e300 of b do not enter the row's scale, and a's values never do: a row whose other reference values
    have the scale 1 holds such a value (a pair that passes by itself: the same NaN or huge number on both sides; a finite x against
    y = inf, where the bound is infinite -- which is how a can hold 1e200 against it), and a node of that row that is off by twice
    the bound FOR SCALE 1 must still be found.  Were the special value part of the scale, the bound would swallow it."""
    y = 1e-6
    bound = rtol * y + atol * 1.0
    for special_a, special_b in ((NAN, NAN), (0.0, INF), (0.0, -INF), (1e300, 1e300), (-2e305, -2e305), (1e200, INF), (-1e250, INF)):
        for factor, passes in ((0.5, True), (2.0, False)):
            b = [[5.0, 5.0, 5.0], [1.0, special_b, y]]
            a = [[5.0, 5.0, 5.0], [1.0, special_a, y + factor * bound]]
            assert harness.compare(a, b, rtol, atol) == (None if passes else (1, 2, a[1][2], y)), (special_a, special_b, factor)
    # the largest finite value below 1e300 counts in full: 9e299
    b = [[9e299, 1.0]]
    assert harness.compare([[9e299, 1.0 + 0.5 * atol * 9e299]], b, rtol, atol) is None


@pytest.mark.parametrize("rtol,atol", TOLERANCES)
def test_an_all_zero_reference_row_takes_equality_only(harness, rtol, atol):
    zeros = [[1.0] * 9, [0.0] * 9]
    assert harness.compare([[1.0] * 9, [0.0] * 9], zeros, rtol, atol) is None
    assert harness.compare([[1.0] * 9, [0.0] * 4 + [-0.0] + [0.0] * 4], zeros, rtol, atol) is None  # (-0.0 == 0.0)
    for x in (5e-324, -5e-324, 1e-300, atol):
        a = [[1.0] * 9, [0.0] * 8 + [x]]
        assert harness.compare(a, zeros, rtol, atol) == (1, 8, x, 0.0), x


@pytest.mark.parametrize("rtol,atol", TOLERANCES)
def test_the_first_mismatch_in_row_major_order_is_reported(harness, rtol, atol):
    b = _rows()
    a = [row[:] for row in b]
    a[1][2] = b[1][2] * 1.5   # an earlier node of a later row
    a[0][8] = b[0][8] + 0.25  # the last node of the first row: comes first
    a[2][0] = -b[2][0]
    assert harness.compare(a, b, rtol, atol) == (0, 8, a[0][8], b[0][8])
    a[0][8] = b[0][8]
    assert harness.compare(a, b, rtol, atol) == (1, 2, a[1][2], b[1][2])
    a[1][1] = b[1][1] * 3.0
    assert harness.compare(a, b, rtol, atol) == (1, 1, a[1][1], b[1][1])


def test_the_switch(harness):
    """BEAT_JIT_SELF_CHECK turns the checks off when it is set and its first character is '0'."""
    assert harness.call("env unset") == {"off": "0"}
    for value, off in (("0", 1), ("0x", 1), ("", 0), ("1", 0), ("no", 0), ("00", 1), ("10", 0)):
        assert harness.call(f"env set {value}") == {"off": str(off)}, value
    assert harness.call("env unset") == {"off": "0"}
