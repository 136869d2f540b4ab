"""tests/fibres_biv_host_harness.cpp from Python: build it with g++ and run a problem through it over a pipe (test_fibres_biv_cpu.py).
Nothing is loaded into this process: csrc/beat_fibres_kernel.h runs in a child and answers with the bits of its results."""
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O1", "-Wall", "-Werror"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build(out_dir, name):
    exe = Path(out_dir) / f"fibres_biv_host_{name}"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[name], f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "fibres_biv_host_harness.cpp")], check=True)
    return exe


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel())


def _bits(s):
    return np.array([int(b, 16) for b in s.split(",")], dtype=np.uint64).view(np.float64)


def _ask(exe, lines, answer):
    p = subprocess.Popen([str(exe)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = p.communicate("\n".join(lines) + "\n", timeout=120)
    assert p.returncode == 0 and err == "", (p.returncode, out[:200], err)  # (a sanitizer reports on stderr and fails the process)
    words = out.split()
    assert words and words[0] == answer, out[:200]
    return dict(w.split("=") for w in words[1:])


def run(exe, cells, h, phi_lv, phi_rv, phi_epi, psi, axis, angles_rad, s_l, s_t, active=None):
    """One problem through one child process; (f, s, n (nvoxels, 3), M (nvoxels, 3, 3), degenerate count) made of the bits it printed."""
    lines = ["cells " + " ".join(str(int(c)) for c in cells), "h " + _hex(h), "angles " + _hex(angles_rad), "cond " + _hex([s_l, s_t]),
             "phi_lv " + _hex(phi_lv), "phi_rv " + _hex(phi_rv), "phi_epi " + _hex(phi_epi)]
    if psi is not None:
        lines.append("psi " + _hex(psi))
    if axis is not None:
        lines.append("axis " + _hex(axis))
    if active is not None:
        lines.append("active " + "".join("1" if a else "0" for a in np.asarray(active).ravel()))
    lines.append("run")
    got = _ask(exe, lines, "run")
    nvox = int(np.prod(cells))
    return SimpleNamespace(f=_bits(got["f"]).reshape(nvox, 3), s=_bits(got["s"]).reshape(nvox, 3), n=_bits(got["n"]).reshape(nvox, 3),
                           M=_bits(got["M"]).reshape(nvox, 3, 3), count=int(got["degenerate"]))


def bislerp(exe, Qa, Qb, t):
    """The header's bislerp of two frames given as matrices [f | n | s]: the quaternions of both (w, x, y, z), the blend's, and the
    blend as a matrix [f | n | s]."""
    cols = lambda Q: [Q[:, 0], Q[:, 2], Q[:, 1]]  # noqa: E731  (the harness takes f, s, n)
    got = _ask(exe, ["bislerp " + _hex(np.concatenate(cols(np.asarray(Qa)) + cols(np.asarray(Qb)))) + " " + _hex([t])], "bislerp")
    return SimpleNamespace(qa=_bits(got["qa"]), qb=_bits(got["qb"]), q=_bits(got["q"]),
                           Q=np.stack([_bits(got["f"]), _bits(got["n"]), _bits(got["s"])], axis=1))
