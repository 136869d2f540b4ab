"""What a device solve of a case of tests/_pcg_ref.py is asked for, against the host's runs of the same case: the checks that
tests/test_rr_iterates_gpu.py (the register-row kernels) and tests/test_small_iterates_gpu.py (the one-launch solve) share.  Every
bound is the reference's own (FACTOR over the distance between its float64 and longdouble runs); none comes from a device."""
import numpy as np

import _pcg_ref as ref


class Check:
    """data: per case key, ``key|x`` (the solution) and ``key|rec`` (iterations, converged_reason, residual_norm, rhs_norm).
    Failures are collected, not raised: one run reports every case that misses."""

    def __init__(self, data):
        self.data, self.failures, self.worst, self.worst_norm = data, [], (0.0, None), (0.0, None)

    def that(self, ok, key, what):
        if not ok:
            self.failures.append(f"{key}: {what}")

    def rec(self, key):
        its, reason, rnorm, bnorm = self.data[f"{key}|rec"]
        return int(its), int(reason), float(rnorm), float(bnorm)

    def iterate(self, key, r, k):
        """x of the case against the longdouble iterate k of reference r."""
        x = self.data[f"{key}|x"]
        if not np.isfinite(x).all():
            self.that(False, key, "x is not finite")
            return
        err, bound = r.x_error(k, x), r.x_bound(k)
        ratio = err * ref.FACTOR / bound  # err / max(delta_k, floor)
        if ratio > self.worst[0]:
            self.worst = (ratio, key)
        self.that(err <= bound, key, f"max|x_dev - x_{k}| = {err:.3e} > {bound:.3e} = 16 max(delta {r.delta(k):.3e}, floor {r.x_floor(k):.3e})")

    def rhs_norm(self, key, r, bnorm):
        err, bound = abs(float(np.longdouble(bnorm) - r.bL)), r.rhs_norm_bound()
        self.worst_norm = max(self.worst_norm, (err * ref.FACTOR / bound, key))
        self.that(err <= bound, key, f"rhs_norm {bnorm!r} off ||b|| = {float(r.bL)!r} by {err:.3e} > {bound:.3e}")

    def cut(self, key, r, k):
        its, reason, rnorm, bnorm = self.rec(key)
        self.that(its == k and reason == -3, key, f"a solve cut at max_it = {k} reports iterations {its}, reason {reason}")
        self.iterate(key, r, k)
        self.rhs_norm(key, r, bnorm)
        err, bound = abs(float(np.longdouble(rnorm) - r.rL[k])), r.residual_bound(k)
        self.worst_norm = max(self.worst_norm, (err * ref.FACTOR / bound, key))
        self.that(err <= bound, key, f"residual_norm {rnorm!r} off ||r_{k}|| = {float(r.rL[k])!r} by {err:.3e} > {bound:.3e}")

    def uncut(self, key, r, rtol):
        its, reason, rnorm, bnorm = self.rec(key)
        k = r.stop(rtol)
        self.that(its == k and reason == 2, key, f"iterations {its}, reason {reason}; the host stops at {k} (||r||/||b|| = "
                  f"{float(r.rL[k] / r.bL):.3e} after {float(r.rL[max(k - 1, 1)] / r.bL):.3e})")
        if its == k:
            self.iterate(key, r, k)
            noise = ref.FACTOR * k * ref.U * float(r.bL)  # (the absolute floor of a cut solve's residual)
            if float(r.rL[k]) <= noise:  # CG on 8 unknowns ends with step 8: that residual is rounding error on both sides
                self.that(rnorm <= noise, key, f"residual_norm {rnorm!r} above the rounding level {noise:.3e} the host's {float(r.rL[k])!r} is below")
            else:
                self.that(abs(rnorm - float(r.rL[k])) <= 1e-6 * float(r.rL[k]), key, f"residual_norm {rnorm!r}, host {float(r.rL[k])!r}")
        self.rhs_norm(key, r, bnorm)

    def same_bits(self, key_a, key_b, iterations):
        xa, xb = self.data[f"{key_a}|x"], self.data[f"{key_b}|x"]
        self.that(np.array_equal(xa, xb), key_b, f"x differs from {key_a} in {int((xa != xb).sum())} nodes, by up to {np.abs(xa - xb).max():.3e}")
        if iterations:
            self.that(self.rec(key_a)[0] == self.rec(key_b)[0], key_b, f"iterations {self.rec(key_b)[0]}, {key_a} {self.rec(key_a)[0]}")
