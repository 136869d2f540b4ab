"""beat.output without a device: the files it writes, read back by a parser of this suite's own (tests/_vti.py); the sample lattice
of csrc/beat_snap_kernel.h, built for the host (tests/snap_host_harness.cpp), against NumPy slicing; the arguments FieldWriter
refuses before it touches the device."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from _vti import read_pvd, read_vti

from beat import output

ROOT = Path(__file__).resolve().parents[1]


def _fields(rng, shape, nfields, dtype):
    names = ["v", "act", "cai"][:nfields]
    return {n: rng.standard_normal(shape).astype(dtype) for n in names}


# ---- .vti ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfields", [1, 3])
@pytest.mark.parametrize("shape", [(7,), (5, 4), (3, 4, 6)])
def test_vti_round_trip(tmp_path, shape, nfields, dtype):
    rng = np.random.default_rng(len(shape) * 10 + nfields)
    arrays = _fields(rng, shape, nfields, dtype)
    arrays["v"].flat[0] = np.nan  # (what a sample outside the tissue holds)
    dim = len(shape)
    origin, spacing = [0.5, -1.0, 2.0][:dim], [0.25, 0.5, 0.125][:dim]
    output.write_vti(tmp_path / "a.vti", arrays, origin, spacing)
    got = read_vti(tmp_path / "a.vti")
    nx, ny, nz = list(reversed(shape)) + [1] * (3 - dim)
    assert got.extent == [0, nx - 1, 0, ny - 1, 0, nz - 1]  # (unused axes: 0 0)
    assert got.origin == origin + [0.0] * (3 - dim) and got.spacing == spacing + [1.0] * (3 - dim)
    assert got.scalars == "v" and list(got.arrays) == list(arrays)
    item = np.dtype(dtype).itemsize
    off = 0
    for name, a in arrays.items():
        assert got.offsets[name] == off  # counted from the byte after the underscore: 8 + nbytes per array before it
        off += 8 + a.size * item
        assert got.arrays[name].dtype.itemsize == item
        assert np.array_equal(got.arrays[name].view(f"u{item}"), a.reshape(nz, ny, nx).view(f"u{item}"))  # bit for bit, NaN included


def test_vti_refuses():
    with pytest.raises(ValueError):
        output.write_vti("x.vti", {})
    with pytest.raises(ValueError):
        output.write_vti("x.vti", {"a": np.zeros((2, 3)), "b": np.zeros((3, 2))})
    with pytest.raises(ValueError):
        output.write_vti("x.vti", {"a": np.zeros(3, dtype=np.int32)})
    with pytest.raises(ValueError):
        output.write_vti("x.vti", {"a": np.zeros((2, 2, 2, 2))})


# ---- a run's files -----------------------------------------------------------------------------------------------------------------
def test_vti_frames_and_pvd_valid_after_every_frame(tmp_path):
    rng = np.random.default_rng(1)
    files = output.FrameFiles(tmp_path / "out" / "run", ("v", "act"), "vti", origin=(1.0, 2.0), spacing=(0.5, 0.25), stride=(2, 1),
                              box=[(2, 9), (0, 4)])
    sent = []
    for k in range(3):
        arrays = _fields(rng, (4, 4), 2, np.float32)
        files.add(0.5 * k, arrays, {"v": (-1.0, 2.0, 0), "act": (float("nan"), float("nan"), 3)})
        sent.append(arrays)
        entries = read_pvd(tmp_path / "out" / "run.pvd")  # valid, and complete up to this frame
        assert entries == [(0.5 * j, f"run_{j:06d}.vti") for j in range(k + 1)]
        assert not list((tmp_path / "out").glob("*.tmp"))
    for (t, name), arrays in zip(entries, sent):
        got = read_vti(tmp_path / "out" / name)
        assert got.origin == [1.0, 2.0, 0.0] and got.spacing == [0.5, 0.25, 1.0]
        for n in arrays:
            assert np.array_equal(got.arrays[n][0], arrays[n])
    files.close()
    files.close()  # idempotent
    assert read_pvd(tmp_path / "out" / "run.pvd") == entries
    with pytest.raises(ValueError):
        files.add(9.0, sent[0])


def test_npy_frames_and_index_valid_after_every_frame(tmp_path):
    rng = np.random.default_rng(2)
    files = output.FrameFiles(tmp_path / "frames", ("v",), "npy", origin=(0.0, 0.0, 0.3), spacing=(0.2, 0.2, 0.6), stride=(1, 1, 3),
                              box=[(0, 4), (0, 3), (1, 5)])
    sent = []
    for k in range(3):
        a = _fields(rng, (2, 3, 4), 1, np.float64)
        files.add(1.0 + k, a, {"v": (float(a["v"].min()), float(a["v"].max()), 0)} if k else {"v": (float("nan"), float("nan"), 5)})
        sent.append(a["v"])
        index = json.loads((tmp_path / "frames" / "index.json").read_text())  # strict JSON after every frame (NaN is null)
        assert index["times"] == [1.0 + j for j in range(k + 1)] and index["fields"] == ["v"]
        assert index["origin"] == [0.0, 0.0, 0.3] and index["spacing"] == [0.2, 0.2, 0.6] and index["stride"] == [1, 1, 3]
        assert index["box"] == [[0, 4], [0, 3], [1, 5]]
        assert index["stats"][0]["v"] == [None, None, 5]
        for j in range(k + 1):
            got = np.load(tmp_path / "frames" / index["files"][j]["v"])
            assert got.shape == (2, 3, 4) and np.array_equal(got, sent[j])
    assert index["stats"][2]["v"] == [float(sent[2].min()), float(sent[2].max()), 0]
    files.close()
    files.close()


def test_frame_files_refuse():
    with pytest.raises(ValueError):
        output.FrameFiles("x", ("v",), "xdmf")
    files = output.FrameFiles("x", ("v",), "vti")
    with pytest.raises(ValueError):
        files.add(0.0, {"w": np.zeros(3)})


# ---- the lattice of the kernel header against NumPy slicing -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def snap_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path_factory.mktemp("snap_host") / "snap_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe), str(ROOT / "tests" / "snap_host_harness.cpp")], check=True)
    return exe


LATTICES = [  # n, lo, hi, stride
    ((7, 5, 4), (0, 0, 0), (7, 5, 4), (1, 1, 1)),
    ((7, 5, 4), (0, 0, 0), (7, 5, 4), (2, 2, 2)),     # strides that do not divide the extents
    ((7, 5, 4), (0, 0, 0), (7, 5, 4), (3, 2, 3)),
    ((9, 6, 5), (2, 1, 1), (8, 5, 4), (4, 3, 2)),     # an interior box
    ((9, 6, 5), (4, 3, 2), (5, 4, 3), (1, 1, 1)),     # a single node
    ((9, 6, 5), (4, 3, 2), (5, 4, 3), (3, 2, 5)),
    ((9, 6, 5), (1, 0, 2), (4, 6, 4), (7, 11, 2)),    # a stride larger than the box
    ((13, 1, 1), (3, 0, 0), (12, 1, 1), (4, 1, 1)),   # 1-D
    ((6, 8, 1), (0, 2, 0), (6, 7, 1), (5, 3, 1)),     # 2-D
]


@pytest.mark.parametrize("n,lo,hi,stride", LATTICES)
def test_lattice_header_matches_numpy_slicing(snap_host, n, lo, hi, stride):
    run = subprocess.run([str(snap_host), *map(str, (*n, *lo, *hi, *stride))], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr)
    lines = dict(line.split(" ", 1) for line in run.stdout.strip().splitlines())
    ids = np.arange(n[0] * n[1] * n[2]).reshape(n[2], n[1], n[0])
    want = ids[lo[2]:hi[2]:stride[2], lo[1]:hi[1]:stride[1], lo[0]:hi[0]:stride[0]]
    assert [int(w) for w in lines["counts"].split()] == list(reversed(want.shape))
    got = np.array([int(w) for w in lines["samples"].split()])
    assert got.shape == (ids.size,)
    # the nodes that map to a sample are exactly the slice's, in the slice's order; every other node maps to none
    on = np.nonzero(got >= 0)[0]
    assert np.array_equal(np.sort(got[on]), np.arange(want.size))
    assert np.array_equal(on[np.argsort(got[on])], want.ravel())
    big = 1 << 33
    assert [int(w) for w in lines["wide"].split()] == [3, -1, -1 if (big + 6) % 3 else (big + 6) // 3, (big + 7) // 3]
    # and the Python side's reading of stride and box gives the same counts
    dim = 3 if n[2] > 1 else 2 if n[1] > 1 else 1
    assert output.lattice(n[:dim], stride[:dim], list(zip(lo, hi))[:dim])[3] == list(reversed(want.shape))[:dim]


def test_row_shift(snap_host):
    for address, want in ((512 * 7, 0), (512 * 7 + 8, 1), (512 * 7 + 504, 63), ((1 << 40) + 512 * 3 + 16, 2)):
        run = subprocess.run([str(snap_host), "shift", str(address)], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stdout.split() == ["shift", str(want)], (run.stdout, run.stderr)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_lattice_arguments():
    assert output.lattice((7, 5), 2) == ([0, 0], [7, 5], [2, 2], [4, 3])
    assert output.lattice((7, 5, 4), (1, 2, 3), [(1, 6), (0, 5), (3, 4)]) == ([1, 0, 3], [6, 5, 4], [1, 2, 3], [5, 3, 1])
    for bad in (dict(stride=0), dict(stride=-1), dict(stride=1.5), dict(stride=(1, 2)), dict(box=[(0, 7)]), dict(box=[(0, 8), (0, 5), (0, 4)]),
                dict(box=[(3, 3), (0, 5), (0, 4)]), dict(box=[(-1, 3), (0, 5), (0, 4)]), dict(box=[(0, 7, 1), (0, 5), (0, 4)])):
        with pytest.raises(ValueError):
            output.lattice((7, 5, 4), **bad)


def test_field_writer_refuses_before_it_touches_the_device(tmp_path):
    good = {"v": lambda x: x}  # (a host callable is no field either; the scalar arguments are looked at first)
    for bad in (dict(format="xdmf"), dict(dtype="float16"), dict(depth=0), dict(depth=17), dict(every=0), dict(every=1.5)):
        with pytest.raises(ValueError):
            output.FieldWriter(tmp_path / "x", good, **bad)
    with pytest.raises(ValueError):
        output.FieldWriter(tmp_path / "x", {})
    with pytest.raises(ValueError):
        output.FieldWriter(tmp_path / "x", {f"f{k}": None for k in range(9)})
    with pytest.raises(ValueError):
        output.FieldWriter(tmp_path / "x", good)  # a host callable
    with pytest.raises(ValueError):
        output.FieldWriter(tmp_path / "x", {'a"b': None})
    with pytest.raises(ValueError):
        output.FieldWriter(tmp_path / "x", {"v": np.zeros(4)})
    assert not (tmp_path / "x").exists() and not list(tmp_path.iterdir())


def test_exports():
    import beat

    assert beat.FieldWriter is output.FieldWriter and beat.output is output
    assert type(beat.grid.VTXWriter()).__name__ == "VTXWriter"  # (the shim stays what it is)
