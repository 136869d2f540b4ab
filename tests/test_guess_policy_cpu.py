"""CPU: the host's bookkeeping of the extrapolated initial guess (csrc/beat_guess.h: which history field plays which role, the
coefficients of the next guess, when the history is dropped, what a deferring solve leaves to its caller, the adaptive choice of
the order), built with g++ into tests/guess_harness.cpp -- once plain, once with the address and undefined-behaviour sanitizers --
and driven line by line.  Fields are host arrays of 3 doubles; all numbers are small integers (or dyadic fractions), so every fma
is exact and every comparison is ==."""
import itertools
import math
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O1", "-Wall", "-Werror"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
FIELDS_NEEDED = {0: 0, 1: 2, 2: 2, 3: 3, 4: 4, -1: 4}  # the max(order - 1, 1) increments kept + the guess; -1 (auto): as order 4


@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    out = tmp_path_factory.mktemp("guess_harness")
    exes = {}
    for name, flags in BUILDS.items():
        exes[name] = out / f"guess_{name}"
        subprocess.run(["g++", "-std=c++17", *flags, f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exes[name]),
                        str(ROOT / "tests" / "guess_harness.cpp")], check=True)
    return exes


class Harness:
    """One child process; call(command) -> {key: value} of its answer (numbers parsed, a,b,c lists split)."""

    def __init__(self, exe):
        self.p = subprocess.Popen([str(exe)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)

    @staticmethod
    def _value(s):
        if "," in s:
            return [Harness._value(v) for v in s.split(",")]
        if s == "none":
            return None
        return float(s) if any(c in s for c in ".e") else int(s)

    def call(self, command):
        self.p.stdin.write(command + "\n")
        self.p.stdin.flush()
        words = self.p.stdout.readline().split()
        assert words and words[0] == command.split()[0], (command, words, self.p.stderr.read() if self.p.poll() is not None else "")
        return {k: self._value(v) for k, v in (w.split("=") for w in words[1:])}

    def close(self):
        _, err = self.p.communicate(timeout=60)
        assert self.p.returncode == 0 and err == "", err  # (a sanitizer reports on stderr and fails the process)

    # one solve as the multi-launch path runs it: terms, the x update's record (one ring cycle), the observation, the end
    def solve(self, inc, iterations=3, nupd=3, ring=6):
        began = self.call("begin")
        self.call("record 0 " + " ".join(str(v) for v in inc))
        self.call(f"observe {iterations}")
        self.call(f"end {nupd} 0 {ring}")
        return began


@pytest.fixture(params=list(BUILDS))
def harness(executables, request):
    h = Harness(executables[request.param])
    yield h
    h.close()


def _poly(m, node):
    """An integer polynomial of degree m - 1 with a non-zero leading coefficient, one per node."""
    coef = [(node + 2) * (j + 1) * (-1) ** j for j in range(m)]
    return lambda k: sum(c * k**j for j, c in enumerate(coef))


def _extrapolation(m, last):
    """sum_{i=1..m} (-1)^(i+1) C(m, i) d_i over the increments `last`, newest first."""
    return sum((-1) ** (i + 1) * math.comb(m, i) * last[i - 1] for i in range(1, m + 1))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_extrapolation_is_exact(harness, order, split):
    """Solve k's increment is P(k), deg P = order - 1: once `order` increments are on record the prepared e is P(k + 1), before that
    the extrapolation through the increments there are.  split: each increment arrives in two ring cycles (terms(0), then terms(ring),
    which accumulates) -- d and e come out the same."""
    P = [_poly(order, node) for node in range(3)]
    assert harness.call(f"configure {order}")["need"] == FIELDS_NEEDED[order]
    ring = 6
    for k in range(12):
        began = harness.call("begin")
        assert began["use_e"] == (1 if k else 0)
        inc = [p(k) for p in P]
        if split:
            first = [7 * (node + 1) - k for node in range(3)]
            assert harness.call("record 0 " + " ".join(map(str, first)))["acc"] == 0
            assert harness.call(f"record {ring} " + " ".join(str(a - b) for a, b in zip(inc, first)))["acc"] == 1
        else:
            assert harness.call("record 0 " + " ".join(map(str, inc)))["acc"] == 0
        assert harness.call(f"end {ring + 2 if split else 3} 0 {ring}")["due"] == 1
        got = harness.call("history")
        m = min(order, k + 1)
        assert got["count"] == min(4, k + 1)
        assert got["d"] == inc
        assert got["e"] == [_extrapolation(m, [p(k - i) for i in range(m)]) for p in P]
        if m == order:
            assert got["e"] == [p(k + 1) for p in P]


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, -1])
def test_history_roles(harness, order):
    """After every advance(): d is the storage of the oldest increment kept and never one of dp[], dp[] lists the newer increments
    newest first, the count saturates at 4."""
    conf = harness.call(f"configure {order}")
    assert conf["need"] == conf["fields"] == FIELDS_NEEDED[order]
    kept = max(1, (4 if order < 0 else order) - 1)
    for k in range(9):
        began = harness.call("begin")
        if order == 0:
            assert began["d"] == began["e"] == -1 and harness.call("record 0 1 1 1") == {"d": -1}
            assert harness.call("end 3 0 6") == {"due": 1, "pending": 0, "count": 0}
            continue
        fields = harness.call("fields")
        d, dps = began["d"], [began[f"dp{j}"] for j in range(2) if began[f"dp{j}"] >= 0]
        assert len(dps) == kept - 1 and d not in dps and began["e"] not in dps + [d] and len(set(dps)) == len(dps)
        for j, f in enumerate(dps):  # the increment of solve k - 1 - j (fields are zeroed before the first solves)
            assert fields[f"f{f}"] == [100 + k - 1 - j if k - 1 - j >= 0 else 0] * 3
        assert fields[f"f{d}"] == [100 + k - kept if k - kept >= 0 else 0] * 3  # the oldest one kept: overwritten by this solve
        harness.call(f"record 0 {100 + k} {100 + k} {100 + k}")
        harness.call("observe 5")
        assert harness.call("end 3 0 6")["count"] == min(4, k + 1)
        assert harness.call("history")["d"] == [100 + k] * 3
        assert harness.call("state")["guess"] == began["e"]


END_CASES = list(itertools.product((0, 1, 5, 6, 7, 12, 13), (6, 12), (0, 1), (0, 1)))


def test_end_of_a_solve(harness):
    empty = {"a": 1, "cd": 0, "cp0": 0, "cp1": 0, "use_e": 0, "acc": 0, "d": -1, "dp0": -1, "dp1": -1, "e": -1}
    for nupd, ring, use_e, deferred in END_CASES:
        harness.call("configure 2")
        if use_e:  # one solve on record: the next starts from x0 = v_ + e
            harness.solve([1, 2, 3], ring=ring)
        began = harness.call("begin")
        assert began["use_e"] == use_e and began["d"] >= 0
        end = harness.call(f"end {nupd} {deferred} {ring}")
        partial, case = nupd % ring != 0, (nupd, ring, use_e, deferred)
        if nupd == 0 and not use_e:  # x = v_ is the answer, nothing was recorded: the history is dropped
            assert end == {"due": 0, "pending": 0, "count": 0}, case
            assert harness.call("begin")["use_e"] == 0
            continue
        due = partial or nupd == 0  # a partial ring cycle, or e alone (no cycle carried it to x)
        assert end == {"due": int(due), "pending": int(due and deferred), "count": use_e + 1}, case
        assert harness.call("traffic")["who"] == int(due and deferred)
        first, second = harness.call("take"), harness.call("take")
        if due and deferred:
            base = (nupd // ring) * ring
            assert first == {**began, "acc": int(base > 0)}, case
        else:
            assert first == empty, case
        assert second == empty and harness.call("state")["pending"] == 0, case


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_fixed_orders_observe_changes_nothing(harness, order):
    harness.call(f"configure {order}")
    for k in range(6):
        harness.call("begin")
        harness.call(f"record 0 {k} {k} {k}")
        before = harness.call("state")
        harness.call(f"observe {3 + 5 * k}")
        assert harness.call("state") == before
        harness.call("end 3 0 6")
    assert harness.call("traffic")["order"] == order


class Auto:
    """The adaptive order driven with a fixed cost per order: a solve costs cost[order its guess was built with] iterations.  The
    order a solve prepares shows in its terms (a = C(m, 1) = m)."""

    def __init__(self, harness, cost):
        self.h, self.cost, self.prepared, self.position = harness, dict(zip((1, 2, 3, 4), cost)), [], []
        harness.call("configure -1")

    def run(self, solves):
        for _ in range(solves):
            built = self.prepared[-1] if self.prepared else None  # the order behind the e this solve starts from
            began = self.h.solve([1, 1, 1], iterations=self.cost[built] if built else 20)
            self.prepared.append(began["a"])
            self.position.append(self.h.call("traffic")["order"])


def _trace(position, probes, solves):
    """`position` prepared by every solve from the third on (the first two have too few increments), except at the probes {solve: order}"""
    return [1, 2] + [probes.get(k, position) for k in range(2, solves)]


def test_auto_stays_where_the_neighbours_cost_more(harness):
    """Starts at 3; the third solve is the first whose guess has the full order, so the 4th (k = 3) makes the first observation at a
    seen order: the 12th such observation is solve 14's, and solve 15 prepares the neighbour -- above and below in turn."""
    a = Auto(harness, (9, 7, 5, 6))
    a.run(90)
    assert a.prepared == _trace(3, {15 + 12 * j: (4, 2)[j % 2] for j in range(7)}, 90)
    assert set(a.position) == {3}


def test_auto_ties_stay(harness):
    a = Auto(harness, (5, 5, 5, 5))
    a.run(90)
    assert set(a.position) == {3} and a.prepared[15] == 4 and a.prepared[27] == 2


def test_auto_scores_only_full_order_guesses(harness):
    """Nothing is scored until a solve starts from a guess built with the full order prepared -- after the start and after the history
    was dropped, whatever those solves cost."""
    harness.call("configure -1")
    for k in range(3):
        harness.solve([1, 1, 1], iterations=1000)
        assert harness.call("state")["seen"] == [0, 0, 0, 0]
    harness.solve([1, 1, 1], iterations=5)
    st = harness.call("state")
    assert st["seen"] == [0, 0, 1, 0] and st["score"][2] == 5
    harness.solve([1, 1, 1], iterations=7)  # the running mean: half the old score, half the new count
    assert harness.call("state")["score"][2] == 6
    harness.call("reset")
    for k in range(3):
        harness.solve([1, 1, 1], iterations=1000)
        st = harness.call("state")
        assert st["seen"] == [0, 0, 1, 0] and st["score"][2] == 6
    harness.solve([1, 1, 1], iterations=8)
    assert harness.call("state")["score"][2] == 7


def test_auto_moves_down_to_1(harness):
    """(3, 5, 7, 9): the probe of 4 (solve 15) changes nothing; the probe of 2 (solve 27) is observed by solve 28, which moves the
    position; the next probe is prepared 12 solves after that observation (up: 3), the one after goes down to 1, where it settles --
    at 1 every probe is turned inward."""
    a = Auto(harness, (3, 5, 7, 9))
    a.run(140)
    expect = _trace(3, {15: 4, 27: 2}, 29) + [2] * 11 + [3] + [2] * 11 + [1] + [2]  # solves 29..39 | 40 | 41..51 | 52 | 53
    expect += [{65: 2, 77: 2, 89: 2, 101: 2, 113: 2, 125: 2, 137: 2}.get(k, 1) for k in range(54, 140)]
    assert a.prepared == expect
    assert a.position[:28] == [3] * 28 and a.position[28:53] == [2] * 25 and set(a.position[53:]) == {1}


def test_auto_moves_up_to_4_and_follows_a_swap(harness):
    a = Auto(harness, (9, 8, 7, 6))
    a.run(60)
    # the probe of 4 (solve 15) is observed by solve 16: the move; from 4 every probe is turned inward (3)
    assert a.position[:16] == [3] * 16 and set(a.position[16:]) == {4}
    assert a.prepared == _trace(3, {15: 4}, 17) + [{28: 3, 40: 3, 52: 3}.get(k, 4) for k in range(17, 60)]
    a.cost = dict(zip((1, 2, 3, 4), (3, 5, 7, 9)))
    a.run(200)
    assert set(a.position[-60:]) == {1}
    a.cost = dict(zip((1, 2, 3, 4), (9, 8, 7, 6)))
    a.run(200)
    assert set(a.position[-60:]) == {4}


def _batch(harness, its):
    harness.call("batch " + " ".join(map(str, its)))
    return harness.call("state")


def test_batch_scoring(harness):
    """beat_split_steps: a batch is scored as one solve, by the mean iteration count of its steps 2.., under the order it ran with."""
    harness.call("configure -1")
    for k in range(3):
        harness.solve([1, 1, 1])
    assert harness.call("state")["e_order"] == 3
    before = harness.call("state")
    for n in (1, 2, 3):  # too short to score: only the "built with" order is cleared
        assert _batch(harness, [50] * n) == {**before, "e_order": 0}
    st = _batch(harness, [50, 50, 5, 7, 6, 6])  # the first two steps ran on the previous batch's guess: not counted
    assert st["seen"] == [0, 0, 1, 0] and st["score"][2] == 6 and st["e_order"] == 0
    assert (st["cur"], st["next"], st["since"]) == (3, 3, 6)  # the cadence: +5 per batch and the policy's own +1
    st = _batch(harness, [50, 50, 8, 8])
    assert st["score"][2] == 7  # 0.5 / 0.5 running mean
    assert (st["cur"], st["next"], st["since"], st["up"]) == (3, 4, 0, 0)  # 12 reached: the next batch runs the neighbour
    st = _batch(harness, [0, 0, 9, 9])
    assert st["seen"] == [0, 0, 1, 1] and st["score"][3] == 9 and (st["cur"], st["next"], st["since"]) == (3, 3, 6)
    st = _batch(harness, [0, 0, 7, 7])
    assert (st["cur"], st["next"], st["since"], st["up"]) == (3, 2, 0, 1)  # every second batch runs a neighbour, above and below in turn
    st = _batch(harness, [0, 0, 7, 7])  # order 2 at the same cost: ties stay
    assert st["score"][1] == 7 and (st["cur"], st["next"]) == (3, 3)


def test_batch_move_needs_more_than_the_margin(harness):
    """The position moves to a neighbour only when its score is lower by more than 0.05 (dyadic means: exact)."""
    harness.call("configure -1")
    _batch(harness, [6] * 4)
    assert _batch(harness, [6] * 4)["next"] == 4
    st = _batch(harness, [0, 0] + [6] * 31 + [5])  # 6 - 1/32: lower, not by enough
    assert st["score"][3] == 6 - 1 / 32 and (st["cur"], st["next"]) == (3, 3)
    assert _batch(harness, [6] * 4)["next"] == 2
    assert _batch(harness, [6] * 4)["next"] == 3
    assert _batch(harness, [6] * 4)["next"] == 4
    st = _batch(harness, [0, 0] + [6] * 7 + [5])  # 6 - 1/8; the running mean is 6 - 5/64 < 6 - 0.05
    assert st["score"][3] == 6 - 5 / 64 and (st["cur"], st["next"], st["since"]) == (4, 4, 1)
    assert harness.call("traffic")["order"] == 4


def test_traffic_and_ghost_planes(harness):
    """traffic(): fields read and written by the x update that carries the guess terms, and who applies it; ghost_e(): the guess
    increment travels with v_'s ghost planes once a solve is on record."""
    harness.call("configure 0")
    assert harness.call("ghost")["e"] == -1
    harness.call("configure 3")
    assert harness.call("ghost")["e"] == -1  # nothing on record: the next solve starts from x0 = v_
    harness.call("begin")
    assert harness.call("traffic") == {"reads": 0, "writes": 2, "order": 3, "who": 0}
    harness.call("end 3 0 6")
    assert harness.call("ghost")["e"] == harness.call("state")["guess"] >= 0
    harness.solve([1, 1, 1])
    began = harness.call("begin")  # third solve: e, d (the oldest kept) and dp[0] are read
    assert (began["a"], began["cp0"], began["cd"]) == (3, -3, 1)
    assert harness.call("traffic") == {"reads": 3, "writes": 2, "order": 3, "who": 0}
    harness.call("end 8 1 6")  # a later ring cycle is pending: it accumulates into d and e
    assert harness.call("traffic") == {"reads": 2, "writes": 2, "order": 3, "who": 1}
    harness.call("applied")  # the launch behind the open solve has applied it
    assert harness.call("traffic") == {"reads": 2, "writes": 2, "order": 3, "who": 2}
    assert harness.call("take")["d"] == -1
    harness.call("skip")
    assert harness.call("ghost")["e"] == -1 and harness.call("history")["count"] == 0
