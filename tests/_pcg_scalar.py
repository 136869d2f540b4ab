"""tests/pcg_scalar_harness.cpp from Python: build it with g++ and drive it line by line (test_pcg_scalar_cpu.py, test_pcg_scalar_gpu.py).
Nothing is loaded into this process: csrc/beat_pcg_scalar.h runs in a child and answers with the bits of its state."""
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O1", "-Wall", "-Werror"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build(out_dir, name):
    exe = Path(out_dir) / f"pcg_scalar_{name}"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[name], f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "pcg_scalar_harness.cpp")], check=True)
    return exe


class Harness:
    """One child process.  Every step returns (st, alphas): float64 arrays made of the very bits the header left."""

    def __init__(self, exe):
        self.p = subprocess.Popen([str(exe)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, bufsize=1)

    def _ask(self, command):
        self.p.stdin.write(command + "\n")
        self.p.stdin.flush()
        words = self.p.stdout.readline().split()
        assert words and words[0] == command.split()[0], (command, words, self.p.stderr.read() if self.p.poll() is not None else "")
        return words[1:]

    def _state(self, command):
        got = dict(w.split("=") for w in self._ask(command))
        bits = lambda s: np.array([int(b, 16) for b in s.split(",")], dtype=np.uint64).view(np.float64)  # noqa: E731
        return bits(got["st"]), bits(got["alphas"])

    def layout(self):
        return {k: int(v) for k, v in (w.split("=") for w in self._ask("layout"))}

    @staticmethod
    def _pairs(values, first=0):
        return " ".join(f"{first + i} {float(v).hex()}" for i, v in enumerate(values))

    def set(self, values, first=0):
        """State slots first, first + 1, .. = values."""
        return self._state("set " + self._pairs(values, first))

    def alpha(self, values):
        return self._state("alpha " + self._pairs(values))

    def begin(self, rtol, atol, max_it):
        return self._state(f"begin {float(rtol).hex()} {float(atol).hex()} {int(max_it)}")

    def roll(self):
        return self._state("roll")

    def predict(self, slot, c):
        return self._state(f"predict {int(slot)} {float(c).hex()}")

    def merged(self, slot):
        return self._state(f"merged {int(slot)}")

    def dump(self):
        return self._state("dump")

    def close(self):
        _, err = self.p.communicate(timeout=60)
        assert self.p.returncode == 0 and err == "", err  # (a sanitizer reports on stderr and fails the process)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))
