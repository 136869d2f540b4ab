"""tests/fibres_host_harness.cpp from Python: build it with g++ and run a problem through it over a pipe (test_fibres_cpu.py).
Nothing is loaded into this process: csrc/beat_fibres_kernel.h runs in a child and answers with the bits of its results."""
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O1", "-Wall", "-Werror"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build(out_dir, name):
    exe = Path(out_dir) / f"fibres_host_{name}"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[name], f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "fibres_host_harness.cpp")], check=True)
    return exe


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel())


def run(exe, cells, h, phi, psi, axis, angles_rad, s_l, s_t, active=None):
    """One problem through one child process; (f, s, n (nvoxels, 3), M (nvoxels, 3, 3), degenerate count) made of the bits it printed."""
    lines = ["cells " + " ".join(str(int(c)) for c in cells), "h " + _hex(h), "angles " + _hex(angles_rad), "cond " + _hex([s_l, s_t]),
             "phi " + _hex(phi)]
    if psi is not None:
        lines.append("psi " + _hex(psi))
    if axis is not None:
        lines.append("axis " + _hex(axis))
    if active is not None:
        lines.append("active " + "".join("1" if a else "0" for a in np.asarray(active).ravel()))
    lines.append("run")
    p = subprocess.Popen([str(exe)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = p.communicate("\n".join(lines) + "\n", timeout=120)
    assert p.returncode == 0 and err == "", (p.returncode, out[:200], err)  # (a sanitizer reports on stderr and fails the process)
    words = out.split()
    assert words and words[0] == "run", out[:200]
    got = dict(w.split("=") for w in words[1:])
    bits = lambda s: np.array([int(b, 16) for b in s.split(",")], dtype=np.uint64).view(np.float64)  # noqa: E731
    nvox = int(np.prod(cells))
    return SimpleNamespace(f=bits(got["f"]).reshape(nvox, 3), s=bits(got["s"]).reshape(nvox, 3), n=bits(got["n"]).reshape(nvox, 3),
                           M=bits(got["M"]).reshape(nvox, 3, 3), count=int(got["degenerate"]))
