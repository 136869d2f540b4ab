// Host build of the event maps' kernel (csrc/beat_events_kernel.h) for the CPU test suite: the kernel's own source, compiled by g++
// and run "thread" by "thread" over a launch grid, so that the rule it implements -- and the deferred update of the potential
// it can carry, against x_flush_kernel's -- is checked on machines without a device (tests/test_events_cpu.py).  Set up as
// tests/ode_host_harness.cpp is.  Built as a shared library; the entry points take what the launches take.
#include <cmath>
#include <cstdint>
#include <cstring>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime.h>  // (host side of the HIP headers: g++ sees __global__ / __device__ / __forceinline__ as plain functions)

#ifndef __launch_bounds__
#define __launch_bounds__(...)
#endif
template <class T>
static inline T __shfl_down(T v, int, int) { return v; }
static inline void __syncthreads() {}
struct Dim3Stub { unsigned x = 0, y = 0, z = 0; };
static Dim3Stub threadIdx, blockIdx, blockDim, gridDim;

#include "../fenicsx-beat_amd/csrc/beat_events_kernel.h"

using namespace beat_events_detail;

namespace {
// x_flush_kernel's two branches (csrc/beat_pde.hip), restated for one node: what beat_pde_x_flush leaves in x, d and e
void flush_node(int64_t i, int nvalid, const double* a, double* x, const double* ring, int64_t fld, const GuessTerms& gt) {
  if (gt.d != nullptr) {
    const double e_old = beat_guess_needs_e(gt) ? gt.e[i] : 0.0;
    const double d_old = beat_guess_needs_d(gt) ? gt.d[i] : 0.0;
    const double dp0 = beat_guess_needs_dp(gt, 0) ? gt.dp[0][i] : 0.0;
    const double dp1 = beat_guess_needs_dp(gt, 1) ? gt.dp[1][i] : 0.0;
    double inc = gt.accumulate ? 0.0 : e_old;
    for (int j = 0; j < nvalid; ++j) inc = std::fma(a[j], ring[(int64_t)j * fld + i], inc);
    x[i] += inc;
    beat_guess_record(gt, gt.d + i, gt.e + i, inc, d_old, dp0, dp1, e_old);
  } else if (nvalid > 0) {
    double xi = x[i];
    for (int j = 0; j < nvalid; ++j) xi = std::fma(a[j], ring[(int64_t)j * fld + i], xi);
    x[i] = xi;
  }
}

template <int FLUSH>
void run(int64_t n, int shift, double* v, const beat_event_maps& m, double t0, double t1, const FlushArgs& fa, unsigned grid) {
  gridDim.x = grid;
  for (unsigned b = 0; b < grid; ++b)
    for (unsigned t = 0; t < BEAT_BLOCK; ++t) {
      blockIdx.x = b;
      threadIdx.x = t;
      if (m.v_prev != nullptr)
        events_kernel<FLUSH, true>(n, shift, v, m, t0, t1, fa);
      else
        events_kernel<FLUSH, false>(n, shift, v, m, t0, t1, fa);
    }
}
}  // namespace

// host_gt: {d, dp0, dp1, e} pointers (d = NULL: no guess), coef: {a, cd, cp0, cp1}, flags: {use_e, accumulate}
static GuessTerms terms(double* const* host_gt, const double* coef, const int* flags) {
  GuessTerms gt;
  gt.d = host_gt[0];
  gt.dp[0] = host_gt[1];
  gt.dp[1] = host_gt[2];
  gt.e = host_gt[3];
  gt.a = coef[0];
  gt.cd = coef[1];
  gt.cp[0] = coef[2];
  gt.cp[1] = coef[3];
  gt.use_e = flags[0];
  gt.accumulate = flags[1];
  return gt;
}

extern "C" void host_events(int64_t n, int shift, double* v, const beat_event_maps* m, double t0, double t1, unsigned grid) {
  run<0>(n, shift, v, *m, t0, t1, FlushArgs{}, grid);
}

extern "C" void host_flush(int64_t n, const double* st, double* x, const double* ring, int64_t fld, const double* alphas, int ring_base,
                           int R, double* const* host_gt, const double* coef, const int* flags) {
  const GuessTerms gt = terms(host_gt, coef, flags);
  int nvalid = (int)st[NUPD] - ring_base;
  nvalid = nvalid < 0 ? 0 : (nvalid > R ? R : nvalid);
  for (int64_t i = 0; i < n; ++i) flush_node(i, nvalid, alphas, x, ring, fld, gt);
}

extern "C" void host_flush_events(int64_t n, int shift, double* x, const beat_event_maps* m, double t0, double t1, const double* st,
                                  const double* ring, int64_t fld, const double* alphas, int ring_base, int R, double* const* host_gt,
                                  const double* coef, const int* flags, unsigned grid) {
  FlushArgs fa;
  fa.st = st;
  fa.ring = ring;
  fa.fld = fld;
  fa.alphas = alphas;
  fa.ring_base = ring_base;
  fa.R = R;
  fa.gt = terms(host_gt, coef, flags);
  if (fa.gt.d != nullptr)
    run<2>(n, shift, x, *m, t0, t1, fa, grid);
  else
    run<1>(n, shift, x, *m, t0, t1, fa, grid);
}
