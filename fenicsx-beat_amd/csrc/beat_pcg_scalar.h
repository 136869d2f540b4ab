// The scalar steps of the Jacobi-PCG: the start of a solve, the roll between iterations (beta, iteration count, convergence latch), the
// predicted stop and the step of the single-reduction iteration -- and the ONE stopping test all of them (and the one-workgroup solve
// and COCG, on their own state) decide with.  Plain C++17 without a HIP call: the kernels run it on the device (pcg_step_kernel and
// reduce_partials_kernel in beat_pde.hip), tests/pcg_scalar_harness.cpp on the host (tests/test_pcg_scalar_cpu.py).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BEAT_PCG_FN __device__ __forceinline__
#else
#define BEAT_PCG_FN inline
#endif

namespace beat_pde_detail {

// slots of the PCG scalar state `st` (device, caller-owned, >= 16 doubles)
enum St { BB = 0, RZ, RR, PQ, RZN, RRN, TOL2, BETA, STOP, ITERS, REASON, RTOL, ATOL, MAXIT, NUPD, RR0, ALPHA, PQS, RQ, QQ };  // RR0: r.r of the initial guess
// ALPHA: the step length of the single-reduction iteration (beat_pcg_merged_next); PQS, RQ, QQ: p.Ap, r.Ap and Ap.Ap of the pass that
// predicts the stop (beat_rr_pdot with a ring slot; PQS is copied to PQ).  Device side only: the host reads the first 16 entries.
// The operator's own scalar state (beat_pde::d_st) has BEAT_ST_DOUBLES entries.
constexpr int BEAT_ST_DOUBLES = 32;
static_assert(RR0 == 15 && QQ < BEAT_ST_DOUBLES, "BB .. RR0 are the 16 entries the host reads; the state holds every slot");

// The scalar step a launch runs (ScalarStep::kind in beat_pde_internal.h; the `then` of reduce_partials_kernel)
enum PcgStep { STEP_NONE = 0, STEP_ROLL, STEP_BEGIN, STEP_PREDICT, STEP_MERGED };

// The stopping test on r.r: 0 = go on, 2 = converged by rtol (tr = rtol^2 b.b), 3 = by atol (tol2 = max(tr, atol^2)).  False for a NaN.
BEAT_PCG_FN int beat_pcg_stop_reason(double rr, double tol2, double tr) { return rr <= tol2 ? (rr <= tr ? 2 : 3) : 0; }

// ... on the state, behind an iteration: convergence first, then max_it (-3).  True: latched.
BEAT_PCG_FN bool beat_pcg_latch(double* st, double rr) {
  int reason = beat_pcg_stop_reason(rr, st[TOL2], st[RTOL] * st[RTOL] * st[BB]);
  if (reason == 0 && st[ITERS] >= st[MAXIT]) reason = -3;
  if (reason == 0) return false;
  st[STOP] = 1.0;
  st[REASON] = (double)reason;
  return true;
}

BEAT_PCG_FN void beat_pcg_begin(double* st, double rtol, double atol, double max_it) {
  const double bb = st[BB], rr = st[RR];
  const double tr = rtol * rtol * bb, ta = atol * atol;
  const double tol2 = tr > ta ? tr : ta;
  st[TOL2] = tol2;
  st[ITERS] = 0.0;
  st[NUPD] = 0.0;
  st[RTOL] = rtol;
  st[ATOL] = atol;
  st[MAXIT] = max_it;
  st[BETA] = 0.0;
  st[RR0] = rr;
  const int reason = beat_pcg_stop_reason(rr, tol2, tr);  // (max_it does not latch here: a solve of no iterations reports 0)
  st[STOP] = reason != 0 ? 1.0 : 0.0;
  st[REASON] = (double)reason;
}

BEAT_PCG_FN void beat_pcg_roll(double* st) {
  st[BETA] = st[RZN] / st[RZ];
  st[RZ] = st[RZN];
  st[RR] = st[RRN];
  st[ITERS] += 1.0;
  beat_pcg_latch(st, st[RR]);
}

// The predicted stop behind PDOT (beat_rr_pdot with a ring slot), with st[PQS..QQ] = p.q, r.q, q.q just summed (q = A p_i, r = r_i):
//   r_{i+1} . r_{i+1} = RR - 2 alpha (r.q) + alpha^2 (q.q)   in exact arithmetic, alpha = RZ / PQ.
// The prediction rho feeds no iterate: it only gates the stop.  E = c (sqrt(RR) + |alpha| sqrt(QQ))^2 bounds |rho - what the residual
// update's reduction would compute| (c: beat_rr_predict_bound).  When rho + E settles the stopping test and its reason (and rho is
// accurate enough for the recorded residual norm) the solve is latched exactly as the update, its count and the roll would have left
// it -- same alpha bits in the ring slot, same ITERS, NUPD, STOP, REASON, RR = max(rho, 0) -- and the update's launches are the no-ops
// latched launches are.  Otherwise nothing changes but PQ: the update and the roll run and decide, max_it included.
BEAT_PCG_FN void beat_pcg_predict(double* st, double* alpha_slot, double c) {
  st[PQ] = st[PQS];
  const double alpha = st[RZ] / st[PQ];  // (the residual update's expression)
  const double rr = st[RR], rq = st[RQ], qq = st[QQ];
  const double rho = std::fma(alpha, std::fma(alpha, qq, -2.0 * rq), rr);
  const double m = std::sqrt(rr) + std::fabs(alpha) * std::sqrt(qq);
  const double e = c * m * m;
  const double tr = st[RTOL] * st[RTOL] * st[BB];
  // (a recorded norm within ~1e-6 of the explicit one: E <= 2^-20 rho; the comparisons are false for a NaN anywhere)
  const int reason = beat_pcg_stop_reason(rho + e, st[TOL2], tr);
  if (reason == 0 || !(e <= 0x1p-20 * rho)) return;
  if (reason == 3 && !(rho - e > tr)) return;  // by atol only when the whole of [rho - E, rho + E] says so
  *alpha_slot = alpha;
  st[RR] = rho > 0.0 ? rho : 0.0;
  st[ITERS] += 1.0;
  st[NUPD] += 1.0;
  st[REASON] = (double)reason;
  st[STOP] = 1.0;
}

// The scalar step of the single-reduction iteration (Chronopoulos & Gear 1989), after the ONE all-reduce of
//   st[PQ] = u . A u,  st[RZN] = r . u,  st[RRN] = r . r      (u = D^-1 r, r = r_i):
// the stopping test on r_i, then  beta_i = (r_i.u_i) / (r_{i-1}.u_{i-1}),  alpha_i = (r.u) / (u.Au - beta_i (r.u) / alpha_{i-1})
// -- the value p_i . A p_i has in exact arithmetic, without forming p_i first.  Counts the update that follows.
BEAT_PCG_FN void beat_pcg_merged_next(double* st, double* alpha_slot) {
  const double g = st[RZN], d = st[PQ], rr = st[RRN];
  st[RR] = rr;
  if (beat_pcg_latch(st, rr)) return;
  const bool first = st[ITERS] == 0.0;
  const double beta = first ? 0.0 : g / st[RZ];
  const double alpha = first ? g / d : g / (d - beta * g / st[ALPHA]);
  st[BETA] = beta;
  st[ALPHA] = alpha;
  st[RZ] = g;
  *alpha_slot = alpha;
  st[NUPD] += 1.0;
  st[ITERS] += 1.0;
}

// One scalar step on `st`.  A latched solve (st[STOP] != 0) is left as it is by every step but the start of the next one.
BEAT_PCG_FN void beat_pcg_step(int kind, double* st, double rtol, double atol, double max_it, double* alpha_slot, double bound_c) {
  if (kind == STEP_BEGIN) {
    beat_pcg_begin(st, rtol, atol, max_it);
    return;
  }
  if (kind == STEP_NONE || st[STOP] != 0.0) return;
  if (kind == STEP_ROLL) beat_pcg_roll(st);
  else if (kind == STEP_PREDICT) beat_pcg_predict(st, alpha_slot, bound_c);
  else beat_pcg_merged_next(st, alpha_slot);
}

}  // namespace beat_pde_detail
