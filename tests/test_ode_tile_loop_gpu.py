"""GPU: the ionic step kernel where ONE BLOCK WALKS SEVERAL TILES (ode_step_kernel's tile loop, csrc/beat_ode_kernel.h).  Models of
fewer than 12 states run capped, looping launches from 6.3 M nodes on and BEAT_ODE_GRID=<blocks> caps every model's launch
(ode_grid, csrc/beat_ode.hip), but the suite's arrays -- 79 tiles at the most, a block each -- never reached the loop's second trip:
the lane number taken afresh per tile, the kernel arguments re-read through an opaque pointer, the row bases formed from tile0, the
pending count taken from LDS, the class kernel's LDS slots reused without a barrier, the exits by break / continue.

tests/_ode_tile_loop_script.py runs every launch form on 2873 = 11 * 256 + 57 nodes (12 tiles; the state array's stride 3328 and
its offset differ from n and 0) in a fresh interpreter per launch shape, since the switches are read once per process:

    tile      BEAT_ODE_GRID=0                      12 blocks: one per tile, the baseline
    one       BEAT_ODE_GRID=1                       1 block walks all 12 (12 tiles per block > 8: the plain cap)
    balanced  BEAT_ODE_GRID=5                       4 blocks of 3 tiles
    capped    BEAT_ODE_GRID=5 BEAT_ODE_BALANCE=0    5 blocks; blocks 0 and 1 take a third tile, block 1 ends on the partial one

Each run reports beat_ode_launch_blocks for every (n, num_states) it launched and the fixture asserts those numbers before any
value is compared: a run that did not loop fails here.  Then (1) the three looping shapes equal the baseline in every stored array
bit for bit -- a node's arithmetic is the same instructions on the same inputs whichever block runs its tile --, (2) the baseline
meets the oracle at the tolerances the suite already asks of the same operation, and (3) a launch that applies a pending update
equals, bit for bit, the run that flushed the update in a pass of its own and then took a plain step.

The cases, and the line of the tile loop each is the first in the suite to execute on a second tile:
  A  TP06 uniform, v_copy, two steps; also n = 2048 (exit by tile * 256 >= n), 2049 (one node in a ninth tile), 63 (fewer tiles
     than the cap)                              -- NodeIO{states + tile0, ...}; `v_copy[i] = states[v_index * ldl + i]`; `if (i >= n) break`
  B  TP06, all 53 per-node rows                  -- `pl[k] = *beat_at(beat_row(ppn + tile0, k, pld), lane_off)`
  C  TP06, 1 and 4 varying rows, run-time-index kernel (the all-rows kernel's bits) and compiled instance
                                                 -- `vj = *beat_at(beat_row(ppn + tile0, j, pld), lane_off)`, `ij = sp.idx[j]` made opaque per tile;
                                                    `mp.v[j] = ...ppn + tile0...` of the compiled instance
  D  TP06 classes on the grid's nodes: class boundaries inside waves, a wave with three classes, runs of 255 (one across a tile
     boundary)                                   -- `mk.markers[i]`, the per-class pass over `NodeIOWithV{states + tile0, ..., v_copy + tile0}`, `continue`
  E  TP06 classes, compact layout with a node map (as DolfinMultiODESolver._setup_one_launch builds it), NaN in the padding
                                                 -- `cls_jn[tid] = (int)jn` reused tile after tile, `vbase[*jn_slot...]`
  F  pending update, count known to the host (ring of 6), guess order 2, four steps
                                                 -- `pendl.ring + (j * pendl.fld + tile0)`, `now.gt.d += tile0` (and e, dp[0], dp[1])
  G  behind an open solve (pending = -1)         -- `s_pend[1]` read per tile, `beat_pending_now(pendl, ...)` with dev_st
  H  class kernel with more than 6 pending directions (ring of 12), on the grid and in the compact layout
                                                 -- `pendl.ring + j * pendl.fld + jn` for j up to 11; the 255 lanes' `*vptr = v_now`
  I  the small models that loop by default at size: FHN, and the generated small_cell.ode uniform, per-node rows, classes, pending
  J  ToR-ORd uniform and classes (the register-tight instances): assertion (1) only, its accuracy is test_golden_gpu.py's

Wall time on an MI355X: 19 s for this file, 17 s of it the four script runs (6.3 s for the first, 3.5 s for each of the others:
about 2 s of interpreter and library start-up each; the first one also compiles, once per machine, the four instances of the generated
model -- 2.7 s -- and the two sparse-row instances of TP06 -- 1.1 s -- that the later runs take from the compile cache)."""
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SCRIPT = ROOT / "tests" / "_ode_tile_loop_script.py"
N = 2873
SMALL = ROOT / "tests" / "data" / "small_cell.ode"
SHAPES = {
    "tile": {"BEAT_ODE_GRID": "0"},
    "one": {"BEAT_ODE_GRID": "1"},
    "balanced": {"BEAT_ODE_GRID": "5"},
    "capped": {"BEAT_ODE_GRID": "5", "BEAT_ODE_BALANCE": "0"},
}
# blocks of a launch over n nodes, per shape (tests/test_ode_grid_cpu.py holds the arithmetic): 12, 8, 9 tiles, one tile, and the
# 11 tiles of the compact array
BLOCKS = {
    "tile": {2873: 12, 2048: 8, 2049: 9, 63: 1, 2816: 11},
    "one": {2873: 1, 2048: 1, 2049: 1, 63: 1, 2816: 1},
    "balanced": {2873: 4, 2048: 4, 2049: 5, 63: 1, 2816: 4},
    "capped": {2873: 5, 2048: 5, 2049: 5, 63: 1, 2816: 5},
}
LAUNCHED = {(2873, 19), (2048, 19), (2049, 19), (63, 19), (2816, 19), (2873, 2), (2873, 5), (2873, 45)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{shape: {name: array}}: the script once per launch shape, one after the other; the launch shape of each asserted here."""
    tmp = tmp_path_factory.mktemp("ode_tile_loop")
    out = {}
    for shape, switches in SHAPES.items():
        env = {k: v for k, v in os.environ.items() if k not in ("BEAT_ODE_GRID", "BEAT_ODE_BALANCE", "BEAT_ODE_TILE_MIN_STATES")}
        env.update(switches)
        path = tmp / f"{shape}.npz"
        t0 = time.perf_counter()
        proc = subprocess.run([sys.executable, str(SCRIPT), str(path)], env=env, capture_output=True, text=True, timeout=900)
        print(f"\n[{shape}] {time.perf_counter() - t0:.1f} s\n{proc.stdout}")
        assert proc.returncode == 0, f"{shape}: exit {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"
        with np.load(path) as z:
            out[shape] = {k: z[k] for k in z.files}
        got = {(int(n), int(ns)): int(b) for n, ns, b in out[shape]["blocks"]}
        assert set(got) == LAUNCHED, (shape, sorted(got))
        assert got == {(n, ns): BLOCKS[shape][n] for n, ns in LAUNCHED}, (shape, got)  # BEFORE any value is compared
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---- (1) the looping launches equal one block per tile, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one", "balanced", "capped"])
def test_looping_launch_equals_one_block_per_tile_bit_for_bit(runs, shape):
    base, other = runs["tile"], runs[shape]
    assert set(base) == set(other)
    differ = [k for k in sorted(base) if k != "blocks" and not _same_bits(base[k], other[k])]
    where = {}
    for k in differ[:8]:  # which nodes: the first tile a block takes is right, the later ones are the question
        if base[k].shape == other[k].shape:
            bad = np.nonzero((_bits(base[k]) != _bits(other[k])).reshape(base[k].shape))[-1]
            where[k] = (int(bad.min()), int(bad.max()), int(np.unique(bad // 256).size))
    assert not differ, (shape, differ, where)


# ---- (2) the baseline against the oracle ---------------------------------------------------------------------------------------------
def _tp06_step_matches_oracle(before, after, params, t, dt, what):
    """1e-11 of max(|ref|, 1e-3); nodes within 0.05 mV of i_CaL's removable singularity at V = 15 mV get 1e-8
    (tests/test_gpu_kernels.py: test_tp06_grl1_one_step_matches_oracle)."""
    from oracle import ionic

    ref = ionic.tp06_generalized_rush_larsen(before, t, dt, params)
    err = np.abs(after - ref) / np.maximum(np.abs(ref), 1e-3)
    assert np.isfinite(after).all(), what
    near = np.abs(before[17] - 15.0) < 0.05
    print(f"{what}: max err {err[:, ~near].max():.3e} ({int(near.sum())} nodes near V = 15: {err[:, near].max() if near.any() else 0.0:.3e})")
    assert err[:, ~near].max() < 1e-11, (what, err[:, ~near].max(), np.unravel_index(err.argmax(), err.shape))
    assert not near.any() or err[:, near].max() < 1e-8, what


def _class_step_matches_oracle(before, after, cls, sets, t, dt, what, v_before=None):
    """The nodes of class k against the oracle with parameter set k; class 255 (and 254): every row keeps its bits."""
    for k, p in enumerate(sets):
        sel = cls == k
        assert sel.any()
        b = before[:, sel].copy()
        if v_before is not None:
            b[17] = v_before[sel]
        _tp06_step_matches_oracle(b, after[:, sel], p, t, dt, f"{what} class {k}")
    idle = cls >= 254
    assert idle.any() and np.array_equal(_bits(after[:, idle]), _bits(before[:, idle])), what


def test_uniform_step_matches_oracle(runs):
    from oracle import ionic

    r = runs["tile"]
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    for n in (N, 2048, 2049, 63):
        for k in (1, 2):
            _tp06_step_matches_oracle(r[f"A{n}_s{k - 1}"], r[f"A{n}_s{k}"], P, 1.0 + (k - 1) * 0.05, 0.05, f"A n={n} step {k}")
            assert _same_bits(r[f"A{n}_vc{k}"], r[f"A{n}_s{k}"][17])


def test_per_node_and_sparse_rows_match_oracle_and_each_other(runs):
    r = runs["tile"]
    _tp06_step_matches_oracle(r["BC_s0"], r["B_s1"], r["B_P"], 1.0, 0.05, "B")
    assert _same_bits(r["B_vc1"], r["B_s1"][17])
    assert np.unique(r["B_P"], axis=1).shape[1] > 32  # (no class route could have taken these)
    for count in (1, 4):
        P = r[f"C{count}_P"]
        assert int((P != P[:, :1]).any(axis=1).sum()) == count
        _tp06_step_matches_oracle(r["BC_s0"], r[f"C{count}_all_s1"], P, 1.0, 0.05, f"C {count} rows")
        # the run-time-index kernel: the all-rows kernel's arithmetic, bit for bit (tests/_jit_fallback_script.py holds this at API level)
        assert _same_bits(r[f"C{count}_rt_s1"], r[f"C{count}_all_s1"]), count
        # the compiled instance takes the derived constants a varying parameter does not enter from the host's evaluation, the
        # all-rows kernel evaluates them per lane (last-bit differences, test_sparse_rows_run_on_an_instance_compiled_for_their_indices):
        # it is held to the oracle like the others
        _tp06_step_matches_oracle(r["BC_s0"], r[f"C{count}_jit_s1"], P, 1.0, 0.05, f"C {count} rows, compiled instance")
        for route in ("rt", "jit"):
            assert _same_bits(r[f"C{count}_{route}_vc1"], r[f"C{count}_{route}_s1"][17]), (count, route)


def test_class_steps_match_oracle_on_the_grid_and_in_the_compact_layout(runs):
    r = runs["tile"]
    m = r["D_markers"]
    assert {int(m[99]), int(m[100]), int(m[699]), int(m[700])} == {0, 1, 2} and len(set(m[1280:1344].tolist())) == 3
    assert (m[500:531] == 255).all() and (m[1010:1041] == 255).all() and m[499] != 255 and m[1041] != 255
    _class_step_matches_oracle(r["D_s0"], r["D_s1"], m, r["D_sets"], 1.0, 0.05, "D")
    assert _same_bits(r["D_vc1"], r["D_s1"][17])
    # E: the potential is read from the field at the mapped node and written to the row and the field; padding keeps its NaN
    cls, nmap, f0, f1 = r["E_cls"], r["E_map"], r["E_field0"], r["E_field1"]
    assert cls.size == 2816 < N and (cls == 254).sum() > 256 and np.isnan(r["E_s0"][:, cls == 254]).all()
    _class_step_matches_oracle(r["E_s0"], r["E_s1"], cls, r["E_sets"], 1.0, 0.05, "E")
    marked = cls < 254
    assert _same_bits(f1[nmap[marked]], r["E_s1"][17, marked])
    untouched = np.ones(N, dtype=bool)
    untouched[nmap[marked]] = False
    assert untouched.any() and _same_bits(f1[untouched], f0[untouched])


def _generated_step_matches(gen, before, after, params, t, dt, what):
    """tests/data/small_cell.ode against its generated NumPy evaluation: 1e-11 of max(|ref|, |y|) (tests/test_ode_file_gpu.py).
    From the second split step on, nodes whose random gates let the inward current run away (m and h both large, ca a thousand
    times its resting value) put a cancellation into dca_dt that the NumPy evaluation itself does not survive to 1e-11: measured
    on such a node against 60 digits, NumPy 7.0e-11 and the device 5.4e-11 off, the formula's running-error bound 4.1e-10.  An
    entry the NumPy evaluation does not confirm is therefore taken to the mpmath evaluation of the file (tests/_ode_mp.py), at
    the bound the expression-language tests hold the device to: 2 ulp of the running-error magnitude.  Returns how many nodes
    went there (a few; never one of the random initial states)."""
    import _ode_mp as M

    ref = gen.numpy_step(before, t, params, dt)
    err = np.abs(after - ref) / np.maximum(np.maximum(np.abs(ref), np.abs(before)), 1e-12)
    assert np.isfinite(after).all(), what
    nodes = np.unique(np.nonzero(err >= 1e-11)[1])
    print(f"{what}: max err {err.max():.3e}, {nodes.size} nodes taken to mpmath")
    assert nodes.size <= 32, (what, nodes.size, err.max())
    if nodes.size:
        p = params if params.ndim == 1 else params[:, nodes]
        mp_ref = M.reference(SMALL, before[:, nodes], p, t, dt, schemes=("generalized_rush_larsen",))["generalized_rush_larsen"]
        worst, leak = M.compare(after[:, nodes], mp_ref, gen.state_names)
        print(f"{what}: ulp of the running-error magnitude {worst}")
        assert max(worst.values()) <= 2.0 and not leak, (what, worst, leak)
    return int(nodes.size)


def test_small_models_match_their_references(runs):
    from beat.models import from_ode
    from oracle import ionic

    r = runs["tile"]
    ref = ionic.fhn_readme_forward_euler(r["Ifhn_s0"], 0.5, 0.01, r["Ifhn_P"])
    np.testing.assert_allclose(r["Ifhn_s1"], ref, rtol=1e-14, atol=1e-14)  # (test_simple_ode_and_fhn_match_oracle)
    assert _same_bits(r["Ifhn_vc1"], r["Ifhn_s1"][1])
    gen = from_ode(SMALL)
    y = r["Igen_s0"]
    for tag in ("uni", "rows", "cls"):
        assert _generated_step_matches(gen, y, r[f"Igen_{tag}_s1"], r[f"Igen_{tag}_P"], 0.3, 0.02, f"generated model, {tag}") == 0
        assert _same_bits(r[f"Igen_{tag}_vc1"], r[f"Igen_{tag}_s1"][0])
    for s in range(4):  # the flushed twin of the pending-update run
        _generated_step_matches(gen, r[f"Igenp_twin_pre{s}"], r[f"Igenp_twin_s{s}"], r["Igenp_P"], 1.0 + s * 0.05, 0.05, f"generated model, twin step {s}")


# ---- (3) a launch that applies the pending update = the flush pass and a plain step ------------------------------------------------------
def _pending_equals_twin(r, tag, steps, skip_v_of=None):
    keys = [k for k in r if k.startswith(f"{tag}_pend_")]
    assert any(k.endswith(f"_s{steps - 1}") for k in keys) and f"{tag}_pend_iters" in keys
    for k in keys:
        a, b = r[k], r[k.replace("_pend_", "_twin_")]
        if skip_v_of is not None and a.ndim == 2:  # (see the caller)
            a, b = a.copy(), b.copy()
            a[17, skip_v_of] = b[17, skip_v_of] = 0.0
        assert _same_bits(a, b), k
    assert (r[f"{tag}_pend_iters"] > 0).all()


def test_pending_update_in_the_launch_equals_flush_and_plain_step(runs):
    from oracle import ionic

    r = runs["tile"]
    P = ionic.tp06_init_parameter_values(stim_amplitude=0.0)
    for tag, steps in (("F", 4), ("G", 3)):
        _pending_equals_twin(r, tag, steps)
        assert f"{tag}_pend_guess_d" in r and r[f"{tag}_pend_guess_count"][0] >= 2  # the guess's fields were live
        for s in range(steps):
            _tp06_step_matches_oracle(r[f"{tag}_twin_pre{s}"], r[f"{tag}_twin_s{s}"], P, 1.0 + s * 0.05, 0.05, f"{tag} step {s}")
            for kind in ("pend", "twin"):
                assert _same_bits(r[f"{tag}_{kind}_vc{s}"], r[f"{tag}_{kind}_s{s}"][17]), (tag, kind, s)
                assert _same_bits(r[f"{tag}_{kind}_row{s}"], r[f"{tag}_{kind}_s{s}"][17]), (tag, kind, s)
    _pending_equals_twin(r, "Igenp", 4)


def test_class_kernel_with_a_long_ring_pending_equals_flush_and_plain_step(runs):
    r = runs["tile"]
    _pending_equals_twin(r, "H", 2)
    m = r["H_markers"]
    for s in range(2):
        # (class 255: the flush -- in the pending run the launch -- advanced the potential, the step then leaves every row alone)
        _class_step_matches_oracle(r[f"H_twin_pre{s}"], r[f"H_twin_s{s}"], m, r["H_sets"], 1.0 + s * 0.05, 0.05, f"H step {s}")
        assert _same_bits(r[f"H_pend_row{s}"], r[f"H_pend_s{s}"][17])
    assert not _same_bits(r["H_twin_pre0"][17, m == 255], r["H_s0"][17, m == 255])  # the update did move the nodes without a class
    # compact layout: the field is the potential's home.  The row of the state array mirrors it as of the last ionic LAUNCH, and only
    # a launch with a pending update writes the entries of class 255 (`states[V_INDEX * ld + i] = v_now`): in the twin they keep
    # their zeros, in the pending run they hold the field's value -- everything else is the same bits
    cls, nmap = r["Hm_cls"], r["Hm_map"]
    _pending_equals_twin(r, "Hm", 2, skip_v_of=cls == 255)
    for s in range(2):
        pre = r[f"Hm_twin_pre{s}"]
        _class_step_matches_oracle(pre, r[f"Hm_twin_s{s}"], cls, r["H_sets"], 1.0 + s * 0.05, 0.05, f"Hm step {s}",
                                   v_before=r[f"Hm_twin_prefield{s}"][nmap])
        for kind in ("pend", "twin"):
            assert _same_bits(r[f"Hm_{kind}_row{s}"][nmap[cls < 254]], r[f"Hm_{kind}_s{s}"][17, cls < 254]), (kind, s)
        assert _same_bits(r[f"Hm_pend_row{s}"][nmap[cls == 255]], r[f"Hm_pend_s{s}"][17, cls == 255])
        assert np.isnan(r[f"Hm_pend_s{s}"][:, cls == 254]).all()
