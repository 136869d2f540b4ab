"""NumPy restatement of the per-node event rule of beat_field_events (include/beat_hip.h), and the synthetic sequence of
potentials the kernel tests run it on.  The restatement always keeps every map (a selected subset is a subset of its result: a
map that is not kept does not change the others -- without ``act_last`` the first activation is the first step that finds the
node above the threshold, which is what ``act_first`` holds here too)."""

import numpy as np

TIME_MAPS = ("act_first", "act_last", "repol", "apd")
ALL_MAPS = TIME_MAPS + ("dvdt_max", "v_max")


def new_maps(n):
    m = {k: np.full(n, np.nan) for k in TIME_MAPS}
    m["dvdt_max"] = np.full(n, -np.inf)
    m["v_max"] = np.full(n, -np.inf)
    # start time of the step that wrote each entry of a time map (the tolerance of a linear time is relative to |t0| + dt)
    m.update({"t0_" + k: np.full(n, np.nan) for k in TIME_MAPS})
    return m


def _above(x, thr, strict):
    return x > thr if strict else x >= thr


def _cross_time(t0, t1, thr, vp, vn):
    with np.errstate(all="ignore"):
        return t0 + (t1 - t0) * (thr - vp) / (vn - vp)


def step(m, vp, vn, t0, t1, thr_up, thr_down, mode, strict):
    """One step (t0, t1) from potential ``vp`` to ``vn``; ``m`` is updated in place.  Returns the masks of the up and down events."""
    linear = mode == 1
    up = _above(vn, thr_up, strict) & (~_above(vp, thr_up, strict) | np.isnan(m["act_last"]))
    tu = np.where(vp < thr_up, _cross_time(t0, t1, thr_up, vp, vn), t0) if linear else np.full(vn.shape, t1)
    first = up & np.isnan(m["act_first"])
    m["act_last"][up] = tu[up]
    m["t0_act_last"][up] = t0
    m["act_first"][first] = tu[first]
    m["t0_act_first"][first] = t0
    down = ~np.isnan(m["act_last"]) & (vp >= thr_down) & (vn < thr_down)
    td = _cross_time(t0, t1, thr_down, vp, vn) if linear else np.full(vn.shape, t1)
    m["repol"][down] = td[down]
    m["apd"][down] = td[down] - m["act_last"][down]
    m["t0_repol"][down] = t0
    m["t0_apd"][down] = t0
    rate = (vn - vp) / (t1 - t0)
    m["dvdt_max"] = np.where(rate > m["dvdt_max"], rate, m["dvdt_max"])
    m["v_max"] = np.where(vn > m["v_max"], vn, m["v_max"])
    return up, down


THR_UP, THR_DOWN = -20.5, -60.25
NSTEPS, DT = 40, 0.05


def sequence(n, seed=11):
    """V_0 .. V_NSTEPS, shape (NSTEPS + 1, n): two plateau pulses with tanh flanks travel over the nodes one behind the other (every
    node they both pass is activated twice), a few per cent of noise on top; from 64 nodes on, four nodes carry hand-made courses:
    one that never leaves rest, one that sits EXACTLY on thr_up for two consecutive steps (vn == thr_up, then vp == thr_up), one
    that crosses thr_up and thr_down back and forth in consecutive steps, one that starts above thr_up and stays there."""
    rng = np.random.default_rng(seed)
    x = (np.arange(n) + 0.5) / n
    V = np.empty((NSTEPS + 1, n))
    for k in range(NSTEPS + 1):
        c1 = 0.15 + 1.9 * k / NSTEPS
        pulse = np.zeros(n)
        for c in (c1, c1 - 0.8):  # nodes in (c - 0.3, c) are on the plateau
            pulse += 0.5 * (np.tanh((c - x) / 0.04) - np.tanh((c - 0.3 - x) / 0.04))
        V[k] = -85.0 + 110.0 * pulse + 3.0 * rng.standard_normal(n)
    special = {}
    if n >= 64:
        special = {"never": n // 7, "exact": n // 3, "recross": n // 2, "stays": (4 * n) // 5}
        V[:, special["never"]] = -85.0 + 0.5 * rng.standard_normal(NSTEPS + 1)
        V[:, special["exact"]] = -85.0
        V[5:7, special["exact"]] = THR_UP
        V[7:20, special["exact"]] = 10.0
        V[:, special["recross"]] = np.where(np.arange(NSTEPS + 1) % 2 == 0, -70.0, 5.0)
        V[:, special["stays"]] = 20.0 + rng.standard_normal(NSTEPS + 1)
    return V, special


def run(V, mode, strict, thr_up=THR_UP, thr_down=THR_DOWN, t_start=0.0):
    """The maps after the whole sequence, and how many up / down events every node had."""
    n = V.shape[1]
    m = new_maps(n)
    ups, downs = np.zeros(n, dtype=int), np.zeros(n, dtype=int)
    for k in range(1, V.shape[0]):
        t0 = t_start + (k - 1) * DT
        up, down = step(m, V[k - 1], V[k], t0, t0 + DT, thr_up, thr_down, mode, strict)
        ups += up
        downs += down
    return m, ups, downs


def kinds(V, m, ups, downs, strict, thr_up=THR_UP):
    """Counts of the node kinds the kernel test wants in its sequence."""
    above0 = _above(V[0], thr_up, strict)
    recross = np.zeros(V.shape[1], dtype=bool)  # up, down through thr_up and up again within three consecutive steps
    a = _above(V, thr_up, strict)
    for k in range(1, V.shape[0] - 2):
        recross |= ~a[k - 1] & a[k] & ~a[k + 1] & a[k + 2]
    return {
        "start_above": int(above0.sum()),
        "never": int((ups == 0).sum()),
        "twice": int((m["act_last"] != m["act_first"])[ups > 0].sum()),
        "vn_on_threshold": int((V[1:] == thr_up).any(axis=0).sum()),
        "vp_on_threshold": int(((V[:-1] == thr_up) & (V[1:] != thr_up)).any(axis=0).sum()),
        "recross": int(recross.sum()),
        "repolarised": int((downs > 0).sum()),
    }
