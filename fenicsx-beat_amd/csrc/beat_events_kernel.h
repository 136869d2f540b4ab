// The event maps' kernel (see beat_events.hip, which launches it; include/beat_hip.h: beat_field_events has the rule).  In a header of
// its own so that the CPU test suite can build it for the host (tests/events_host_harness.cpp) and run it against the NumPy
// restatement of the rule without a device.
#pragma once
#include "beat_pde_internal.h"

namespace beat_events_detail {

using namespace beat_pde_detail;

struct FlushArgs {
  const double* st = nullptr;
  const double* ring = nullptr;
  int64_t fld = 0;
  const double* alphas = nullptr;
  int ring_base = 0;
  int R = 0;
  GuessTerms gt{};
};

__device__ __forceinline__ bool is_nan(double x) { return x != x; }

template <int FLUSH, bool VP>
__global__ __launch_bounds__(BEAT_BLOCK) void events_kernel(int64_t n, int shift, double* __restrict__ v, beat_event_maps m, double t0,
                                                            double t1, FlushArgs fa) {
  const double* __restrict__ ring = fa.ring;  // (as x_flush_kernel declares them: x, the directions and the maps do not overlap)
  int nvalid = 0;
  double a[PRING_MAX];
  if constexpr (FLUSH != 0) {
    nvalid = (int)fa.st[NUPD] - fa.ring_base;
    nvalid = nvalid < 0 ? 0 : (nvalid > fa.R ? fa.R : nvalid);
#pragma unroll
    for (int j = 0; j < PRING_MAX; ++j) a[j] = (j < nvalid) ? fa.alphas[j] : 0.0;
  }
  const double dt = t1 - t0;
  const bool strict = m.strict != 0, linear = m.mode == 1;
  const bool down = m.repol != nullptr || m.apd != nullptr;
  const int lane = threadIdx.x & 63;
  const int64_t npieces = (n + shift + 63) >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * (BEAT_BLOCK / 64);
  for (int64_t piece = (int64_t)blockIdx.x * (BEAT_BLOCK / 64) + (threadIdx.x >> 6); piece < npieces; piece += nwaves) {
    const int64_t i = piece * 64 + lane - shift;
    if (i < 0 || i >= n) continue;
    double vn;
    if constexpr (FLUSH == 2) {  // x_flush_kernel's guess branch
      const GuessTerms& gt = fa.gt;
      const double e_old = beat_guess_needs_e(gt) ? gt.e[i] : 0.0;
      const double d_old = beat_guess_needs_d(gt) ? gt.d[i] : 0.0;
      const double dp0 = beat_guess_needs_dp(gt, 0) ? gt.dp[0][i] : 0.0;
      const double dp1 = beat_guess_needs_dp(gt, 1) ? gt.dp[1][i] : 0.0;
      double inc = gt.accumulate ? 0.0 : e_old;
#pragma unroll
      for (int j = 0; j < PRING_MAX; ++j)
        if (j < nvalid) inc = fma(a[j], ring[(int64_t)j * fa.fld + i], inc);
      vn = v[i] + inc;
      v[i] = vn;
      beat_guess_record(gt, gt.d + i, gt.e + i, inc, d_old, dp0, dp1, e_old);
    } else if constexpr (FLUSH == 1) {  // its plain branch (which leaves x alone when nothing is pending)
      vn = v[i];
      if (nvalid > 0) {
#pragma unroll
        for (int j = 0; j < PRING_MAX; ++j)
          if (j < nvalid) vn = fma(a[j], ring[(int64_t)j * fa.fld + i], vn);
        v[i] = vn;
      }
    } else {
      vn = v[i];
    }

    const double vp = VP ? m.v_prev[i] : 0.0;
    const bool up_n = strict ? vn > m.thr_up : vn >= m.thr_up;
    // up event: above the threshold now and (below it a step ago, or never activated: the reference's rule, a node that is above
    // the threshold when first observed is activated at that step)
    bool fire = false;
    double al = 0.0;  // act_last[i] where it has been loaded or written
    bool al_known = false;
    if (m.act_last != nullptr) {  // (needs v_prev: the entry points see to it)
      const bool up_p = strict ? vp > m.thr_up : vp >= m.thr_up;
      fire = up_n && !up_p;
      if (up_n && up_p) {
        al = m.act_last[i];
        al_known = true;
        fire = is_nan(al);
      }
    } else if (m.act_first != nullptr) {  // the first event of a node is the first step that finds it above the threshold
      fire = up_n && is_nan(m.act_first[i]);
    }
    if (fire) {
      double tu = t1;
      if (linear) tu = vp < m.thr_up ? t0 + dt * (m.thr_up - vp) / (vn - vp) : t0;
      if (m.act_last != nullptr) {
        m.act_last[i] = tu;
        al = tu;
        al_known = true;
        if (m.act_first != nullptr && is_nan(m.act_first[i])) m.act_first[i] = tu;
      } else {
        m.act_first[i] = tu;
      }
    }
    // down event of an activated node
    if (down && vp >= m.thr_down && vn < m.thr_down) {
      if (!al_known) al = m.act_last[i];
      if (!is_nan(al)) {
        const double td = linear ? t0 + dt * (m.thr_down - vp) / (vn - vp) : t1;
        if (m.repol != nullptr) m.repol[i] = td;
        if (m.apd != nullptr) m.apd[i] = td - al;
      }
    }
    if (m.dvdt_max != nullptr) {
      const double rate = (vn - vp) / dt;
      if (rate > m.dvdt_max[i]) m.dvdt_max[i] = rate;
    }
    if (m.v_max != nullptr) {
      if (vn > m.v_max[i]) m.v_max[i] = vn;
    }
    if constexpr (VP) m.v_prev[i] = vn;
  }
}

}  // namespace beat_events_detail
