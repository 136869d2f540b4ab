"""CPU: how many blocks an ionic launch gets (csrc/beat_ode_grid.h, the arithmetic behind ode_grid in csrc/beat_ode.hip and
beat_ode_launch_blocks), built with g++ into tests/ode_grid_harness.cpp.  A block walks the tiles b, b + blocks, ...: whatever the
cap, every tile of 256 nodes is visited once, and balancing a cap never lengthens the longest block."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CAPS = (0, 1, 2, 3, 5, 7, 8, 64, 24576)
TILES = range(1, 601)
SMALL_CAP, BALANCE_MAX = 24576, 8  # what ode_grid's comments say: 24 576 looping blocks for small models, balanced up to 8 tiles per block


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    """{(tiles, num_states, cap_env, tile_min_states, balance): blocks} from one run of the harness."""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path_factory.mktemp("ode_grid") / "ode_grid"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'fenicsx-beat_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "ode_grid_harness.cpp")], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        *key, b = map(int, line.split())
        assert tuple(key) not in out
        out[tuple(key)] = b
    assert {(t, 19, c, 12, bal) for t in TILES for c in CAPS for bal in (0, 1)} <= set(out)
    return out


def _ceil(a, b):
    return -(-a // b)


def _walk(tiles, nblocks):
    """Tiles each block takes, as the kernel's loop walks them."""
    return [list(range(b, tiles, nblocks)) for b in range(nblocks)]


@pytest.mark.parametrize("balance", [0, 1])
@pytest.mark.parametrize("cap", CAPS)
def test_blocks_within_bounds_and_every_tile_visited_once(blocks, cap, balance):
    for tiles in TILES:
        b = blocks[(tiles, 19, cap, 12, balance)]
        assert 1 <= b <= tiles, (tiles, b)
        if cap == 0 or tiles <= cap:
            assert b == tiles, (tiles, b)
        else:
            assert b <= cap, (tiles, b)
        walked = sorted(t for mine in _walk(tiles, b) for t in mine)
        assert walked == list(range(tiles)), (tiles, b)  # (as lists: a tile walked twice would show)


@pytest.mark.parametrize("cap", [c for c in CAPS if c > 0])
def test_balancing_evens_the_blocks_and_never_lengthens_the_longest(blocks, cap):
    for tiles in TILES:
        if tiles <= cap:
            continue
        per_block = _ceil(tiles, cap)
        b = blocks[(tiles, 19, cap, 12, 1)]
        if per_block > BALANCE_MAX:
            assert b == cap, (tiles, b)
            continue
        assert b == _ceil(tiles, per_block), (tiles, b)
        lengths = [len(mine) for mine in _walk(tiles, b)]
        assert max(lengths) == per_block == max(len(mine) for mine in _walk(tiles, cap)), (tiles, b)
        assert set(lengths) <= {per_block, per_block - 1}, (tiles, b)
        assert sum(1 for k in lengths if k == per_block - 1) < per_block, (tiles, b)


@pytest.mark.parametrize("cap", [c for c in CAPS if c > 0])
def test_without_balancing_the_cap_is_the_launch(blocks, cap):
    for tiles in TILES:
        if tiles > cap:
            assert blocks[(tiles, 19, cap, 12, 0)] == cap, tiles


def test_an_unset_cap_goes_by_the_number_of_states(blocks):
    for tiles in (1, 12, 600, 24576, 24577, 65536, 196608, 196609, 524288):
        for balance in (0, 1):
            for tmin in (12, 6, 46):
                for ns in (2, 5, 11, 12, 19, 45):
                    got = blocks[(tiles, ns, -1, tmin, balance)]
                    if ns >= tmin:  # a block per tile
                        assert got == tiles, (tiles, ns, tmin)
                    else:  # what BEAT_ODE_GRID=24576 gives: the explicit cap goes by no model size
                        assert got <= SMALL_CAP, (tiles, ns, tmin)
                        per_block = _ceil(tiles, SMALL_CAP)
                        want = tiles if tiles <= SMALL_CAP else (_ceil(tiles, per_block) if balance and per_block <= BALANCE_MAX else SMALL_CAP)
                        assert got == want, (tiles, ns, tmin, balance)
    assert blocks[(600, 11, -1, 12, 1)] == 600 and blocks[(65536, 11, -1, 12, 1)] < 65536 == blocks[(65536, 12, -1, 12, 1)]
    assert blocks[(65536, 11, -1, 6, 1)] == 65536 and blocks[(65536, 19, -1, 46, 1)] < 65536  # tile_min_states is honoured


def test_the_sizes_the_comments_quote(blocks):
    # 256^3 = 65 536 tiles, a small model: 2.67 tiles per block on 24 576 blocks -> 21 846 blocks of 3 (the last two of 2)
    assert blocks[(65536, 5, -1, 12, 1)] == 21846
    lengths = [len(mine) for mine in _walk(65536, 21846)]
    assert max(lengths) == 3 and set(lengths) == {2, 3} and lengths.count(2) == 2
    assert blocks[(65536, 5, -1, 12, 0)] == 24576
    # 512^3 = 524 288 tiles: 21.3 tiles per block, the plain cap
    assert blocks[(524288, 5, -1, 12, 1)] == blocks[(524288, 5, -1, 12, 0)] == 24576
    # TP06 (19 states): one block per tile at both sizes
    assert blocks[(65536, 19, -1, 12, 1)] == 65536 and blocks[(524288, 19, -1, 12, 1)] == 524288
    # the launch shapes tests/test_ode_tile_loop_gpu.py asks for: 12, 8, 9 tiles and one tile
    assert [blocks[(12, 19, c, 12, bal)] for c, bal in ((0, 1), (1, 1), (5, 1), (5, 0))] == [12, 1, 4, 5]
    assert [blocks[(t, 19, 5, 12, 1)] for t in (8, 9, 1)] == [4, 5, 1]
