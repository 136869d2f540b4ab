// Extrapolated initial guess (beat_pde_set_guess_order): what the kernels share (GuessTerms and what an x update does with them) and
// the host's bookkeeping in one object (beat_guess_state: the roles of the history fields, the coefficients of the next guess, when
// the history is dropped, what a deferring solve leaves to its caller, the adaptive choice of the order).  No HIP runtime calls: the
// library's translation units, the run-time compiler and the CPU test (tests/test_guess_policy_cpu.py, g++) read it from here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BEAT_GUESS_FN __device__ __forceinline__
#else
#define BEAT_GUESS_FN inline
#endif

namespace beat_pde_detail {
// The solve starts from x0 = v_ + e, where e was prepared by
// the previous solve's x update from the increments d = x - v_ of the last solves: polynomial extrapolation in time
// of degree m - 1 through the last m increments, e = sum_{i=1..m} (-1)^(i+1) C(m, i) d_i  (m = 1: d1; 2: 2 d1 - d2;
// 3: 3 d1 - 3 d2 + d3; 4: 4 d1 - 6 d2 + 4 d3 - d4).  e is never added to x by a pass of its own: it rides with the
// deferred update  x += inc, inc = e + sum alpha_j p_j,  which also records d <- inc (over the oldest increment kept)
// and prepares the next guess  e <- a inc + cd d_old + sum cp_j dp_j  in place.
constexpr int BEAT_GUESS_MAX_ORDER = 4;
struct GuessTerms {
  double* d = nullptr;   // in: the oldest increment kept, out: this solve's; nullptr: no guess in use
  const double* dp[BEAT_GUESS_MAX_ORDER - 2] = {nullptr, nullptr};  // the newer increments (d1, d2): read only
  double* e = nullptr;   // in: this solve's guess increment (if use_e), out: the next solve's
  double a = 1.0, cd = 0.0, cp[BEAT_GUESS_MAX_ORDER - 2] = {0.0, 0.0};
  int use_e = 0;
  // an x update of a later ring cycle of the same solve: e went to x with the first cycle, this one adds its
  // directions to x and to what the first cycle recorded (d += inc, e += a inc)
  int accumulate = 0;
};

// what an x update does to (d, e) once its increment is known -- one expression shared by the flush kernels and the
// ionic kernel's pending path, so that both leave the same bits behind.  d_old / dp_old / e_old: the values the
// fields held (read by the caller up front, together with its other loads; unused ones may be anything)
BEAT_GUESS_FN bool beat_guess_needs_d(const GuessTerms& gt) { return gt.accumulate || gt.cd != 0.0; }
BEAT_GUESS_FN bool beat_guess_needs_dp(const GuessTerms& gt, int j) { return !gt.accumulate && gt.cp[j] != 0.0; }
BEAT_GUESS_FN bool beat_guess_needs_e(const GuessTerms& gt) { return gt.accumulate || gt.use_e; }
BEAT_GUESS_FN void beat_guess_record(const GuessTerms& gt, double* d, double* e, double inc, double d_old,
                                     double dp0_old, double dp1_old, double e_old) {
  if (gt.accumulate) {
    *d = d_old + inc;
    *e = fma(gt.a, inc, e_old);
  } else {
    double en = gt.a * inc;
    if (gt.cp[0] != 0.0) en = fma(gt.cp[0], dp0_old, en);
    if (gt.cp[1] != 0.0) en = fma(gt.cp[1], dp1_old, en);
    if (gt.cd != 0.0) en = fma(gt.cd, d_old, en);
    *d = inc;
    *e = en;
  }
}
}  // namespace beat_pde_detail

// The host's side of the guess, one per operator (beat_pde::guess).  A solve path that supports the guess calls begin() before its
// right-hand side, passes terms(ring_base) to every x update and ends with observe() and end(); every other path calls skip() (the
// history does not survive a solve that did not record its increment).  The device memory behind the fields belongs to the
// operator (beat_pde_set_guess_order allocates what configure() asks for and hands it over with attach()).
struct beat_guess_state {
  using GuessTerms = beat_pde_detail::GuessTerms;
  static constexpr int MAX_ORDER = beat_pde_detail::BEAT_GUESS_MAX_ORDER;

  // initial guess from the previous solves' increments (0: x0 = v_; m: + the degree-(m-1) extrapolation of the last m), see GuessTerms
  int order = 0;  // as configured: 0..4, or -1 = choose per solve (below)
  // adaptive choice (order = -1).  No order is right everywhere: each recorded increment carries an rtol-sized
  // error, which an extrapolation of order m amplifies by the sum of its |coefficients| (1, 3, 7, 15) -- where the
  // increments are smooth in time (plateau, repolarisation, rest) that noise sets the initial residual and the lowest
  // order wins (0.3 iterations per step against 1.6), on a travelling front the truncation error does and the cubic
  // wins (3.6 against 8).  Hill climbing on the order: a running mean of the iteration count per order, the current
  // order used, one of its neighbours tried every 12th solve (up and down in turn), the move made when the neighbour
  // has been costing fewer iterations.  Iteration counts are global: every rank of a decomposed solve decides alike.
  int auto_cur = 3;      // order the policy currently favours
  int auto_next = 3;     // order of the guess the NEXT x update prepares (auto_cur or a probe)
  int auto_e_order = 0;  // order the guess now in e was built with (0: none / not adaptive)
  double auto_score[4] = {0.0, 0.0, 0.0, 0.0};  // running mean of the iterations per solve for orders 1..4
  int auto_seen[4] = {0, 0, 0, 0};
  int auto_since_probe = 0, auto_probe_up = 1;
  double* d_hist[3] = {nullptr, nullptr, nullptr};  // fields with ghost planes: the last increments, newest first
  double* d_guess = nullptr;  // the guess increment e prepared for the next solve
  double* alloc = nullptr;    // the device memory of hist_fields fields (allocated and freed by the operator)
  int hist_fields = 0;
  int hist_n = 0;             // solves recorded since the history was last dropped (capped at the maximal order)
  GuessTerms cur{};           // terms of the solve in progress (d == nullptr: not in use)
  bool pending = false;       // the last solve left x += e + sum alpha_j p_j to its caller ...
  GuessTerms guess_left{};    // ... with these terms
  bool applied_behind = false;  // that update was applied by the launch enqueued behind the open solve, with these terms (traffic)
  GuessTerms applied_terms{};

  int max_order() const { return order < 0 ? MAX_ORDER : order; }
  int kept() const { return std::max(1, max_order() - 1); }  // increments kept: order - 1 (at least one)
  int fields() const { return hist_fields; }

  // A new order: policy and history start over.  Returns the fields it needs: the max(order - 1, 1) increments kept + the guess
  // (1024^3: 8.6 GB each -- only what the order needs; adaptive: the fields the cubic needs)
  int configure(int new_order) {
    order = new_order;
    hist_n = 0;
    cur = GuessTerms{};
    auto_cur = auto_next = 3;
    auto_e_order = 0;
    for (int k = 0; k < 4; ++k) auto_seen[k] = 0;
    auto_since_probe = 0;
    return order != 0 ? kept() + 1 : 0;
  }
  // `n_fields` zeroed fields, `fld` doubles apart, each behind a ghost plane of `plane` doubles (mem == nullptr: none)
  void attach(double* mem, int n_fields, int64_t plane, int64_t fld) {
    alloc = mem;
    hist_fields = mem != nullptr ? n_fields : 0;
    d_hist[0] = d_hist[1] = d_hist[2] = d_guess = nullptr;
    if (mem == nullptr) return;
    for (int j = 0; j < n_fields - 1; ++j) d_hist[j] = mem + plane + (int64_t)j * fld;
    d_guess = mem + plane + (int64_t)(n_fields - 1) * fld;
  }
  void reset() { hist_n = 0, auto_e_order = 0; }  // increments of another problem (time step, state) say nothing about this one
  void skip() { reset(), cur = GuessTerms{}; }    // a solve that does not record its increment

  void begin() {
    cur = GuessTerms{};
    if (order == 0 || d_hist[0] == nullptr) return;
    GuessTerms& g = cur;
    // increments kept newest first in d_hist; the oldest one's storage takes this solve's
    const int nb = kept();
    g.d = d_hist[nb - 1];
    for (int j = 0; j + 1 < nb; ++j) g.dp[j] = d_hist[j];
    g.e = d_guess;
    g.use_e = hist_n >= 1;
    // the guess after this solve extrapolates through the m increments then on record (this one included):
    // e = sum_{i=0}^{m-1} (-1)^i C(m, i+1) D_i,  D_0 = this solve's, D_i = d_hist[i-1] as it is now
    const int want = order < 0 ? auto_next : order;
    const int m = std::min(want, hist_n + 1);
    static const double binom[5][5] = {{1, 0, 0, 0, 0}, {1, 1, 0, 0, 0}, {1, 2, 1, 0, 0}, {1, 3, 3, 1, 0}, {1, 4, 6, 4, 1}};
    g.a = binom[m][1];
    for (int i = 1; i < m; ++i) {
      const double c = ((i & 1) ? -1.0 : 1.0) * binom[m][i + 1];
      if (i - 1 == nb - 1)
        g.cd = c;
      else
        g.cp[i - 1] = c;
    }
  }

  // Terms of an x update for the ring cycle starting at iteration ring_base: the first cycle carries e and records the
  // increment, later ones add to it.
  GuessTerms terms(int ring_base) const {
    GuessTerms g = cur;
    if (g.d != nullptr && ring_base > 0) g.accumulate = 1;
    return g;
  }

  // this solve's increment has been recorded: it is the most recent one now
  void advance() {
    const int nb = kept();
    double* newest = d_hist[nb - 1];
    for (int j = nb - 1; j > 0; --j) d_hist[j] = d_hist[j - 1];
    d_hist[0] = newest;
    hist_n = std::min(MAX_ORDER, hist_n + 1);
  }

  // Adaptive order: observe() is called by the solve paths once the host has the scalar state of the solve that just ended, before
  // end() / advance().  Scores the order the guess was built with by what it is for -- the
  // iterations the solve took (the norm of the initial residual is a poor judge: the cubic's is smaller even where it
  // costs more iterations, because what is left is the amplified noise of the recorded increments, rough, and Jacobi-PCG
  // takes longer over it than over the smooth truncation error of the quadratic) -- and picks the order of the guess
  // after next (the next one is being prepared by this solve's x update, whose coefficients were fixed when it began).
  // policy() is the move itself (hill climbing over the orders 1..4, see above); returns the order to prepare next.
  int policy() {
    constexpr int LO = 1, HI = MAX_ORDER;
    int& at = auto_cur;
    // a neighbour that has been looked at and costs fewer iterations takes over (ties stay)
    for (int nb = at - 1; nb <= at + 1; nb += 2) {
      if (nb < LO || nb > HI || !auto_seen[nb - 1] || !auto_seen[at - 1]) continue;
      if (auto_score[nb - 1] < auto_score[at - 1] - 0.05) {
        at = nb;
        auto_since_probe = 0;  // look around from the new position soon
        break;
      }
    }
    int next = at;
    if (auto_seen[at - 1] && ++auto_since_probe >= 12) {
      auto_since_probe = 0;
      int nb = at + (auto_probe_up ? 1 : -1);
      if (nb < LO || nb > HI) nb = at - (auto_probe_up ? 1 : -1);
      auto_probe_up = !auto_probe_up;
      if (nb >= LO && nb <= HI) next = nb;
    }
    return next;
  }
  void score(int scored_order, double iterations) {
    const int k = scored_order - 1;
    auto_score[k] = auto_seen[k] ? 0.5 * auto_score[k] + 0.5 * iterations : iterations;
    auto_seen[k] = 1;
  }
  void observe(int iterations) {  // of the solve that just ended
    if (order >= 0) return;
    // the order behind the e this solve started from (0: none yet, or fewer increments)
    if (auto_e_order >= 1) score(auto_e_order, iterations);
    // the e the x update of THIS solve prepares has order min(auto_next, increments on record): remember it for the
    // next observation, then choose for the one after
    const int prepared = std::min(auto_next, hist_n + 1);
    auto_e_order = prepared == auto_next ? prepared : 0;
    auto_next = policy();
  }
  // A batch of one-launch solves (beat_split_steps) whose iteration counts iters[0], iters[stride], ... the host sees only now: the
  // whole batch ran with one order (its first solves on the guess the previous batch left); score it by the mean iteration count of
  // the later steps and let the policy move (here one "solve" is one batch).  The e the batch left is not scored by the next solve.
  void observe_batch(const double* iters, int stride, int n_steps) {
    auto_e_order = 0;
    if (order >= 0 || n_steps < 4) return;
    double sum = 0.0;
    for (int s = 2; s < n_steps; ++s) sum += iters[(int64_t)stride * s];
    score(auto_next, sum / (n_steps - 2));
    auto_since_probe += 5;  // (a batch stands for many solves: look at a neighbour every second batch)
    auto_next = policy();
  }

  // The end of a solve that executed nupd updates with a ring of `ring` directions; returns true when an application (e and/or the
  // last partial ring cycle) is still due.  deferred: it is left to the caller, who gets its terms from take_pending()
  bool end(int nupd, bool deferred, int ring) {
    const bool partial = nupd % ring != 0;
    if (cur.d == nullptr) return partial;
    const bool e_due = nupd == 0 && cur.use_e;  // no ring cycle carried e to x yet
    if (nupd == 0 && !e_due) {  // x = v_ is the answer and nothing was recorded: the history ends here
      skip();
      return false;
    }
    const bool due = partial || e_due;
    if (due && deferred) {
      guess_left = terms((nupd / ring) * ring);
      pending = true;
    }
    advance();
    return due;
  }
  // the terms of the application a deferring solve left to its caller, once (nothing pending: no guess terms)
  GuessTerms take_pending() {
    if (!pending) return GuessTerms{};
    pending = false;
    return guess_left;
  }
  // the launch enqueued behind the open solve has applied what that solve would have left pending
  void pending_applied_behind() {
    if (pending) {
      applied_terms = guess_left;
      applied_behind = true;
    }
    pending = false;
  }

  // a decomposed solve: the guess increment whose ghost planes travel with v_'s (nullptr: the next solve starts from x0 = v_)
  double* ghost_e() const { return order != 0 && hist_n >= 1 ? d_guess : nullptr; }

  // beat_pde_guess_history
  void history(double** dev_d, double** dev_e, int* count) const {
    if (dev_d) *dev_d = d_hist[0];
    if (dev_e) *dev_e = d_guess;
    if (count) *count = hist_n;
  }
  // beat_pde_guess_traffic: fields read, fields written, the order, who applies / applied the update
  void traffic(int out[4]) const {
    // (an update applied by a launch enqueued behind an open solve: its terms were kept when that solve was finished)
    const GuessTerms& g = pending ? guess_left : (applied_behind ? applied_terms : cur);
    int reads = 0, writes = 0;
    if (g.d != nullptr) {
      reads += (g.accumulate || g.use_e) ? 1 : 0;      // e
      reads += (g.accumulate || g.cd != 0.0) ? 1 : 0;  // the oldest increment kept
      for (int j = 0; j < MAX_ORDER - 2; ++j) reads += (!g.accumulate && g.cp[j] != 0.0) ? 1 : 0;
      writes = 2;  // d, e
    }
    out[0] = reads;
    out[1] = writes;
    out[2] = order < 0 ? auto_cur : order;
    out[3] = pending ? 1 : (applied_behind ? 2 : 0);  // 2: applied by the launch behind the open solve
  }
};
