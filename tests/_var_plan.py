"""tests/var_plan_harness.cpp from Python: build it with g++, send it a grid with its tissue bits and a list of commands, read the plans
of csrc/beat_var_plan.h back (test_var_plan_cpu.py).  Nothing is loaded into this process: the header runs in a child."""
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O1", "-Wall", "-Werror"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SEG = 62            # x-nodes per column (csrc/beat_var_plan.h)
MAX_ITEMS = 16384   # BEAT_MAX_PARTIALS of csrc/beat_common.h: what the library passes


def build(out_dir, name):
    exe = Path(out_dir) / f"var_plan_{name}"
    subprocess.run(["g++", "-std=c++17", *BUILDS[name], f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "var_plan_harness.cpp")], check=True)
    return exe


def flag_words(tissue) -> np.ndarray:
    """bool per node (x fastest) -> the 64-node flag words: bit l of word s = node 64 s + l."""
    t = np.asarray(tissue, dtype=bool).ravel()
    padded = np.zeros(-(-len(t) // 64) * 64, dtype=np.uint8)
    padded[: len(t)] = t
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def case_line(shape, faces, tissue) -> str:
    words = flag_words(tissue)
    return f"case {shape[0]} {shape[1]} {shape[2]} {faces[0]} {faces[1]} {len(words)} " + " ".join(f"{int(w):x}" for w in words)


def ask(exe, lines) -> list:
    """One child for all of `lines`; the answers of the commands that answer (all but `case`), each {first word of a line: the rest}."""
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])  # (a sanitizer reports on stderr and fails the process)
    answers, cur = [], {}
    for line in p.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "end":
            answers.append(cur)
            cur = {}
        else:
            assert key not in cur, key
            cur[key] = rest
    assert not cur and len(answers) == sum(1 for ln in lines if not ln.startswith("case")), (len(answers), len(lines))
    return answers


def _counted(text, base=10, dtype=np.int64):
    n, *v = text.split()
    assert int(n) == len(v)
    return np.array([int(x, base) for x in v], dtype=dtype)


def items_of(text) -> np.ndarray:
    """(n, 4) rows of seg, rb, zb, ze."""
    n, *v = text.split()
    assert 4 * int(n) == len(v)
    return np.array(v, dtype=np.int64).reshape(-1, 4)


def seg_answer(a) -> dict:
    return {"seg": _counted(a["seg"]), "segmask": _counted(a["segmask"], 16, np.uint64), "tiled": _counted(a["tiled"]),
            "tiledmask": _counted(a["tiledmask"], 16, np.uint64)}


def vtl_answer(a):
    """None where the plan declines; else nsegx, nzp, run, base[3], count[3], first (3, 9), the three lists and, if asked for, the masks
    as an (ny + 2, nsegx, nzp) array."""
    if a["vtl"] == "declined":
        assert set(a) == {"vtl"}
        return None
    nsegx, nzp, run = map(int, a["vtl"].split())
    lists = np.array(a["lists"].split(), dtype=np.int64).reshape(3, 2)
    items = items_of(a["items"])
    out = {"nsegx": nsegx, "nzp": nzp, "run": run, "base": lists[:, 0], "count": lists[:, 1],
           "first": np.array(a["first"].split(), dtype=np.int64).reshape(3, 9), "n_items": len(items),
           "lists": [items[b: b + c] for b, c in lists], "mask_id": a["mask"]}
    if "maskwords" in a:
        out["mask"] = _counted(a["maskwords"], 16, np.uint64).reshape(-1, nsegx, nzp)
    return out


def vrr_answer(a) -> dict:
    fc = np.array(a["vrr"].split(), dtype=np.int64).reshape(3, 2)
    items = items_of(a["items"])
    return {"first": fc[:, 0], "count": fc[:, 1], "n_items": len(items), "lists": [items[f: f + c] for f, c in fc]}


def parts_answer(a) -> list:
    """[part 0's plane ranges, part 1's]: [(z_lo, z_hi), ...] each."""
    out = []
    for k in ("part0", "part1"):
        z = _counted(a[k])
        out.append(list(zip(z[0::2].tolist(), z[1::2].tolist())))
    return out
