"""GPU: ``bench.py --dump-outputs DIR`` -- what the headline's last timed step left to the caller, written so that two builds
can be compared output for output: the same arguments give the same inputs and the same files, ``--steps`` is the number of
steps those files are the result of, and a run decomposed over ranks writes the same sample of nodes."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
COMMON = ["--size", "48", "--warmup", "1", "--cpu-sample", "0", "--no-front"]


def _bench(out_dir, steps, *extra, env=None):
    cmd = [sys.executable, str(ROOT / "bench.py"), *COMMON, "--steps", str(steps), "--dump-outputs", str(out_dir), *extra]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0]), {f.stem: np.load(f) for f in sorted(Path(out_dir).glob("*.npy"))}


@pytest.mark.gpu
def test_bench_dump_outputs_are_reproducible_and_follow_steps(tmp_path):
    from beat.models import tp06

    r1, a = _bench(tmp_path / "a", 3)
    _, b = _bench(tmp_path / "b", 3)
    r3, c = _bench(tmp_path / "c", 2)
    assert r1["steps"] == 3 and r3["steps"] == 2 and r1["config"]["finite"]
    assert set(a) == {"v", "states"}
    n = 48**3  # below both sample sizes: the whole grid
    assert a["v"].shape == (n,) and a["states"].shape == (19, n)
    assert all(x.dtype == np.float64 and np.isfinite(x).all() for x in a.values())
    np.testing.assert_array_equal(a["v"], a["states"][tp06.state_index("V")])
    assert a["v"].min() == r1["config"]["v_min"] and a["v"].max() == r1["config"]["v_max"]
    for k in a:  # same arguments, same outputs
        np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=0.0)
    assert np.abs(c["v"] - a["v"]).max() > 1e-6  # one step fewer is another answer
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20


@pytest.mark.gpu
def test_bench_dump_outputs_of_two_ranks_sharing_one_gpu(tmp_path):
    """Two ranks over the host-staged transport (BEAT_DIST_BACKEND=gloo, both on this box's GPU): rank 0 gathers the slabs'
    samples in node order, so the files have the one-rank shapes and the potential still is the V row of the states."""
    from beat.models import tp06

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(BEAT_DIST_BACKEND="gloo", BEAT_BENCH_ALT="0", BEAT_BENCH_PARITY="0")
    r, d = _bench(tmp_path / "two", 2, "--gpus", "2", env=env)
    n = 48**3
    assert r["n_gpus"] == 2 and d["v"].shape == (n,) and d["states"].shape == (19, n)
    np.testing.assert_array_equal(d["v"], d["states"][tp06.state_index("V")])
    assert np.isfinite(d["states"]).all() and d["v"].min() == r["config"]["v_min"] and d["v"].max() == r["config"]["v_max"]
