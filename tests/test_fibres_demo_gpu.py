"""GPU: demos/lv_fibres.py at its smallest size runs to the end and finds no degenerate voxel outside the apex cap."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_lv_fibres_demo():
    smallest = re.search(r"^MIN_SIZE = (\d+)", (ROOT / "demos" / "lv_fibres.py").read_text(), flags=re.M).group(1)
    run = subprocess.run([sys.executable, str(ROOT / "demos" / "lv_fibres.py"), "--size", smallest, "--steps", "2"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    m = re.search(r"degenerate voxels: (\d+) \((\d+) outside the apex cap\)", run.stdout)
    assert m, run.stdout
    assert int(m.group(2)) == 0
    assert re.search(r"closed form: mean [0-9.]+ deg, max [0-9.]+ deg", run.stdout), run.stdout
