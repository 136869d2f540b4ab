"""CPU: the host-built work plans of the per-node-coefficient diffusion path -- the segment list and its tile order, the lane masks, tile
lists and parts of vtl_spmv_kernel, the column runs of vrr_spmv_kernel -- as csrc/beat_var_plan.h builds them, printed by
tests/var_plan_harness.cpp (g++, once plain, once with the address and undefined-behaviour sanitizers; child processes).  Every
assertion is stated on a plan and the tissue bits it was made from: which nodes a list covers and how often, what an item may span,
the order of a list, where the parts begin.  The grids and masks are the 3-D cases of tests/_var_ref.py (the tissue nodes of
tests/test_var_iterates_gpu.py: the nodes of active cells), each with physical and live faces in all four combinations."""
import itertools
import shutil

import numpy as np
import pytest

import _var_plan as vp
import _var_ref as vr
from _var_plan import MAX_ITEMS, SEG

FACES = list(itertools.product((0, 1), (0, 1)))  # (z_lo_phys, z_hi_phys)
CASES_3D = [c for c in vr.CASES if vr.SHAPES[c[0]] == 3]
VTL_OPTIONS = list(itertools.product((4, 8), (5, 16), (0, 1, 2)))  # ry, max_run, aligned
VRR_OPTIONS = list(itertools.product((2, 4), (5, 48)))             # ry, max_run
TILE_EDGES = (8, 3)


@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    out = tmp_path_factory.mktemp("var_plan_harness")
    return {name: vp.build(out, name) for name in vp.BUILDS}


@pytest.fixture(params=list(vp.BUILDS))
def exe(executables, request):
    return executables[request.param]


def tissue_of(c) -> np.ndarray:
    """bool (nz, ny, nx)."""
    nx, ny, nz = c[0]
    return vr.case(c).tissue.reshape(nz, ny, nx)


def column_activity(T, ry) -> np.ndarray:
    """bool (nz, row blocks, x segments): the column of ry rows x 62 x-nodes holds tissue on that plane."""
    nz, ny, nx = T.shape
    nrb, nsegx = -(-ny // ry), -(-nx // SEG)
    P = np.zeros((nz, nrb * ry, nsegx * SEG), dtype=bool)
    P[:, :ny, :nx] = T
    return P.reshape(nz, nrb, ry, nsegx, SEG).any(axis=(2, 4))


def planes_of(ranges, nz) -> np.ndarray:
    R = np.zeros(nz, dtype=bool)
    for z_lo, z_hi in ranges:
        assert 0 <= z_lo <= z_hi <= nz and not R[z_lo:z_hi].any()
        R[z_lo:z_hi] = True
    return R


def check_cover(items, A, ranges):
    """The items cover every column plane with tissue of the planes `ranges` exactly once and nothing outside them; an item lies inside
    one of the ranges and holds tissue."""
    nz, nrb, nsegx = A.shape
    R = planes_of(ranges, nz)
    C = np.zeros(A.shape, dtype=np.int64)
    for seg, rb, zb, ze in items:
        assert 0 <= seg < nsegx and 0 <= rb < nrb and 0 <= zb < ze <= nz
        assert any(z_lo <= zb and ze <= z_hi for z_lo, z_hi in ranges), (zb, ze, ranges)
        assert A[zb:ze, rb, seg].any(), "an item without tissue in lanes 1..62"
        C[zb:ze, rb, seg] += 1
    assert (C[A & R[:, None, None]] == 1).all() and (C <= 1).all() and (C[~R] == 0).all()


def range_of(zb, ranges):
    return next((z_lo, z_hi) for z_lo, z_hi in ranges if z_lo <= zb < z_hi)


def check_vtl_list(items, A, ranges, run, aligned, whole):
    check_cover(items, A, ranges)
    for seg, rb, zb, ze in items:
        assert zb // run == (ze - 1) // run, "a tile crosses a multiple of the run"
        act = A[zb:ze, rb, seg]
        z_lo, z_hi = range_of(zb, ranges)
        c0, c1 = max(zb // run * run, z_lo), min((zb // run + 1) * run, z_hi)
        if aligned == 0:
            assert act[0] and act[-1]
            assert not (~act[:-2] & ~act[1:-1] & ~act[2:]).any(), "a gap of three planes inside a tile"
        elif aligned == 2:
            assert (zb, ze) == (c0, c1)
        else:
            on = np.nonzero(A[c0:c1, rb, seg])[0]
            assert (zb, ze) == (c0 + on[0], c0 + on[-1] + 1)
    key = [(zb // run, rb, seg) for seg, rb, zb, ze in items]
    if whole or len(ranges) < 2:
        assert key == sorted(key)
    else:  # the two boundary planes: the lower plane's tiles, then the upper plane's, each in order
        lower = [k for k, it in zip(key, items) if it[2] == ranges[0][0]]
        upper = [k for k, it in zip(key, items) if it[2] != ranges[0][0]]
        assert key == lower + upper and lower == sorted(lower) and upper == sorted(upper)
    if whole and aligned == 0:
        by_column = {}
        for seg, rb, zb, ze in items:
            by_column.setdefault((seg, rb), []).append((zb, ze))
        for runs in by_column.values():
            runs.sort()
            for (_, e0), (b1, _) in zip(runs, runs[1:]):
                # (the planes between two items hold no tissue: check_cover)
                assert b1 - e0 >= 3 or (b1 // run) * run >= e0, "two tiles of a column that one run of planes would have held"


def check_parts(plan):
    for k in range(3):
        items, base, first = plan["lists"][k], plan["base"][k], plan["first"][k]
        assert first[0] == base and first[8] == base + plan["count"][k] and (np.diff(first) >= 0).all()
        cum = np.concatenate([[0], np.cumsum(items[:, 3] - items[:, 2] + 2)]).astype(np.int64)  # weight: planes + 2 per item
        want = [int(cum[-1]) * x // 8 for x in range(9)]
        assert (first == base + np.searchsorted(cum, want, side="left")).all()
    assert plan["base"][0] == 0 and plan["base"][1] == plan["count"][0] and plan["base"][2] == plan["base"][1] + plan["count"][1]
    assert plan["n_items"] == plan["count"].sum()


def expected_masks(T, faces):
    """(ny + 2, nsegx, nz + 6) words: bit l of [y + 1, seg, z + 1] = tissue(62 seg - 1 + l, y, z) inside the box; planes -1 and nz:
    the in-box lanes on a live face; everything else 0."""
    nz, ny, nx = T.shape
    nsegx = -(-nx // SEG)

    def words(F):  # (planes, ny, nx) -> (ny, nsegx, planes)
        P = np.zeros((F.shape[0], ny, nsegx * SEG + 2), dtype=np.uint64)
        P[:, :, 1: nx + 1] = F
        lanes = np.stack([P[:, :, SEG * s: SEG * s + 64] for s in range(nsegx)], axis=2)  # (planes, ny, nsegx, 64)
        return (lanes << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64).transpose(1, 2, 0)

    out = np.zeros((ny + 2, nsegx, nz + 6), dtype=np.uint64)
    out[1: ny + 1, :, 1: nz + 1] = words(T)
    box = words(np.ones((1, ny, nx), dtype=bool))[:, :, 0]
    if not faces[0]:
        out[1: ny + 1, :, 0] = box
    if not faces[1]:
        out[1: ny + 1, :, nz + 1] = box
    return out


def check_vtl_plan(plan, T, faces, parts, ry, max_run, aligned, max_items, unlimited=None):
    """`unlimited`, where max_items is not the library's: the plan of the same grid, faces and options at the library's max_items and at
    max_run = this plan's run.  Lists 1 and 2 may be empty on a slab with a live face only where `unlimited` (held to the tissue like
    every plan at the library's max_items) shows that the two of them need more than max_items slots."""
    A = column_activity(T, ry)
    nz = T.shape[0]
    assert plan["nsegx"] == A.shape[2] and plan["nzp"] == nz + 6 and plan["count"][0] <= max_items
    run = plan["run"]
    assert run >= max_run and run % max_run == 0 and (run // max_run) & (run // max_run - 1) == 0  # doubled, if changed at all
    check_vtl_list(plan["lists"][0], A, [(0, nz)], run, aligned, whole=True)
    dropped = False
    if max_items != MAX_ITEMS:
        assert unlimited["run"] == run
        dropped = unlimited["count"][1] + unlimited["count"][2] > max_items
    if faces == (1, 1) or dropped:
        assert plan["count"][1] == plan["count"][2] == 0
    else:
        # (at the library's max_items the grids of this module can never fill the slots: a tile per column and plane at the most)
        assert A.size <= MAX_ITEMS and plan["count"][1] + plan["count"][2] <= max_items
        check_vtl_list(plan["lists"][1], A, parts[0], run, aligned, whole=False)
        check_vtl_list(plan["lists"][2], A, parts[1], run, aligned, whole=False)
    check_parts(plan)


def check_vrr_plan(plan, T, parts, ry, max_run):
    A = column_activity(T, ry)
    nz = T.shape[0]
    for items, ranges in zip(plan["lists"], ([(0, nz)], parts[0], parts[1])):
        check_cover(items, A, ranges)
        for seg, rb, zb, ze in items:
            act = A[zb:ze, rb, seg]
            assert ze - zb <= max_run and not (~act[:-2] & ~act[1:-1] & ~act[2:]).any()
        key = [(-(ze - zb), rb, seg, zb) for seg, rb, zb, ze in items]  # long runs first, ties in generation order
        assert key == sorted(key)
    assert plan["first"][0] == 0 and (plan["first"][1:] == np.cumsum(plan["count"])[:2]).all() and plan["n_items"] == plan["count"].sum()


def check_segments(got, T, edge):
    nz, ny, nx = T.shape
    words = vp.flag_words(T)
    assert (got["seg"] == np.nonzero(words)[0]).all() and (got["segmask"] == words[words != 0]).all()
    if edge == 0:
        assert len(got["tiled"]) == len(got["tiledmask"]) == 0
        return
    first_node = got["seg"] * 64
    key = (first_node // (nx * ny) // edge) * (-(-ny // edge)) + first_node % (nx * ny) // nx // edge
    order = np.argsort(key, kind="stable")
    assert (got["tiled"] == got["seg"][order]).all() and (got["tiledmask"] == got["segmask"][order]).all()


def commands(max_items_of=lambda options: MAX_ITEMS):
    """The commands sent behind every `case` line, and what each of them is: (kind, its arguments)."""
    what = [("parts", ())] + [("seg", (t,)) for t in TILE_EDGES + (0,)]
    what += [("vtl", o + (max_items_of(o),)) for o in VTL_OPTIONS] + [("vrr", o) for o in VRR_OPTIONS]
    lines = []
    for kind, args in what:
        # (the masks depend on the grid and the faces alone: printed in full once per case, named by their hash otherwise)
        want_mask = kind == "vtl" and args[:3] == VTL_OPTIONS[0]
        lines.append(" ".join([kind, *map(str, args)] + (["1" if want_mask else "0"] if kind == "vtl" else [])))
    return what, lines


def check_case(exe, shape, T, faces_list=FACES, expect_vtl=True):
    what, lines = commands()
    sent = []
    for faces in faces_list:
        sent += [vp.case_line(shape, faces, T)] + lines
    answers = iter(vp.ask(exe, sent))
    plans = {}
    for faces in faces_list:
        parts, mask_id = None, None
        for kind, args in what:
            a = next(answers)
            if kind == "parts":
                parts = vp.parts_answer(a)
            elif kind == "seg":
                check_segments(vp.seg_answer(a), T, args[0])
            elif kind == "vtl":
                plan = vp.vtl_answer(a)
                assert (plan is not None) == expect_vtl
                if plan is None:
                    continue
                check_vtl_plan(plan, T, faces, parts, *args)
                if "mask" in plan:
                    assert (plan["mask"] == expected_masks(T, faces)).all()
                    mask_id = plan["mask_id"]
                assert plan["mask_id"] == mask_id
                plans[(faces, args)] = plan
            else:
                check_vrr_plan(vp.vrr_answer(a), T, parts, *args)
    return plans


@pytest.mark.parametrize("case", CASES_3D, ids=vr.case_key)
def test_plans_of_the_reference_cases(exe, case):
    T = tissue_of(case)
    plans = check_case(exe, case[0], T)
    # lists 1 and 2 are dropped together when they do not fit together: offered exactly as many slots as list 0 needs, the plan keeps
    # list 0 as it is and the other two only where they are no longer (every command of one child, the case sent once per face pair)
    sent, asked = [], []
    for faces in FACES[:3]:
        sent.append(vp.case_line(case[0], faces, T))
        for o in VTL_OPTIONS:
            full = plans[(faces, o + (MAX_ITEMS,))]
            sent.append(f"vtl {o[0]} {o[1]} {o[2]} {max(1, full['count'][0])} 0")
            asked.append((faces, o, full))
    for (faces, o, full), a in zip(asked, vp.ask(exe, sent)):
        tight = vp.vtl_answer(a)
        assert tight["run"] == full["run"] and (tight["lists"][0] == full["lists"][0]).all()
        if full["count"][1] + full["count"][2] > max(1, full["count"][0]):
            assert tight["count"][1] == tight["count"][2] == 0
        else:
            assert all((tight["lists"][k] == full["lists"][k]).all() for k in (1, 2))
        check_parts(tight)


def test_run_doubled_until_the_tiles_fit_and_declined_when_they_never_do(exe):
    case = ((6, 4, 71), "layers")
    T = tissue_of(case)
    nz = T.shape[0]
    # with all the slots of the library, per face pair: runs of 5, of 10 and of the whole slab (list 0 does not depend on the faces)
    sent = []
    for faces in FACES:
        sent.append(vp.case_line(case[0], faces, T))
        sent += ["parts", f"vtl 4 5 0 {MAX_ITEMS} 0", f"vtl 4 10 0 {MAX_ITEMS} 0", f"vtl 4 {nz} 0 {MAX_ITEMS} 0"]
    answers = iter(vp.ask(exe, sent))
    unlimited = {}
    for faces in FACES:
        parts = vp.parts_answer(next(answers))
        unlimited[faces] = [vp.vtl_answer(next(answers)) for _ in range(3)]
        for plan, max_run in zip(unlimited[faces], (5, 10, nz)):
            assert plan["run"] == max_run
            check_vtl_plan(plan, T, faces, parts, 4, max_run, 0, MAX_ITEMS)
    n5, n10, n_all = (int(p["count"][0]) for p in unlimited[FACES[0]])
    assert all([int(p["count"][0]) for p in unlimited[faces]] == [n5, n10, n_all] for faces in FACES)
    assert n5 > n10 > n_all >= 1  # (one column: runs of 5 planes cut the layers more often than runs of 10)
    sent = []
    for faces in FACES:
        sent.append(vp.case_line(case[0], faces, T))
        sent += ["parts", f"vtl 4 5 0 {n5 - 1} 0", f"vtl 4 5 0 {n_all - 1} 0", f"vtl 4 5 0 {n5} 0"]
    answers = iter(vp.ask(exe, sent))
    for faces in FACES:
        parts = vp.parts_answer(next(answers))
        doubled, declined, kept = (vp.vtl_answer(next(answers)) for _ in range(3))
        assert doubled is not None and doubled["run"] == 10 and doubled["count"][0] == n10
        check_vtl_plan(doubled, T, faces, parts, 4, 5, 0, n5 - 1, unlimited=unlimited[faces][1])
        assert declined is None  # more tiles than slots with one run over the whole slab
        assert kept is not None and kept["run"] == 5 and kept["count"][0] == n5
        check_vtl_plan(kept, T, faces, parts, 4, 5, 0, n5, unlimited=unlimited[faces][0])


def test_empty_mask(exe):
    shape = (63, 16, 6)
    plans = check_case(exe, shape, np.zeros(shape[::-1], dtype=bool))
    assert plans and all(p["n_items"] == 0 and (p["first"] == 0).all() for p in plans.values())


def test_one_plane_slab_with_two_live_faces(exe):
    case = ((41, 32, 1), "cutshell")
    T = tissue_of(case)
    assert T.any() and not T.all()
    check_case(exe, case[0], T, faces_list=[(0, 0)], expect_vtl=False)  # the tile plan declines; the column runs and the segments do not
    what, lines = commands()
    answers = vp.ask(exe, [vp.case_line(case[0], (0, 0), T)] + lines)
    vrr = [vp.vrr_answer(a) for (kind, _), a in zip(what, answers) if kind == "vrr"]
    assert all(p["count"][0] > 0 and p["count"][1] == 0 and p["count"][2] == p["count"][0] for p in vrr)  # its plane: the lower boundary plane


def test_sizes_the_tile_plan_declines(exe):
    def declined(nx, ny, nz):
        return vp.ask(exe, [f"sizes {nx} {ny} {nz}"])[0]["sizes"] == "1"

    assert not declined(2, 2, 2)
    assert declined(2, 2, 1) and declined(1, 2, 2) and declined(2, 1, 2)
    # plane = nx ny: 2^28 - 1 = 18705 x 14351 is taken, 2^28 is not
    assert 18705 * 14351 == 2 ** 28 - 1 and not declined(18705, 14351, 2)
    assert declined(16384, 16384, 2)
    # mask offsets (ny + 2) nsegx (nz + 6): 2^15 x 1 x 2^16 = 2^31 is declined, one plane less is taken
    assert declined(62, 2 ** 15 - 2, 2 ** 16 - 6) and not declined(62, 2 ** 15 - 2, 2 ** 16 - 7)
    assert declined(63, 2 ** 14 - 2, 2 ** 16 - 6) and not declined(63, 2 ** 14 - 2, 2 ** 16 - 7)  # two x segments
