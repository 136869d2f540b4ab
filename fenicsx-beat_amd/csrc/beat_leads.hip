// ECG lead traces on the device: several dot products with the potential in one pass.  The reference recovers the current density
// and integrates it once per electrode and sample
//   src/beat/ecg.py:282-298   ECGRecovery.solve (Mass Im = -(1/C_m) K v), eval(point) -> assemble_scalar of Im / (4 pi sigma_b |x - p|)
// Both steps are linear in v and both matrices are symmetric:  lead_l = w_l . Im = q_l . v  with  q_l = -(1/C_m) K Mass^-1 w_l,  a
// row that depends on the mesh, the tensor and the electrode only (beat.ecg.LeadRecorder makes it once).  A sample of L leads is
// then L dot products of stored rows with v: no solve, nothing returns to the host.
//
// The kernel.  One double per lane.  A wavefront walks over 512-byte pieces of v that are aligned in memory (as the event maps'
// pass, beat_events.hip: the first piece starts up to 63 nodes before the field and masks those lanes, the last one masks its
// tail), two pieces per trip, and reads the same nodes of R rows of q, R <= BEAT_LEADS_ROWS a compile-time count: R fp64
// accumulators per lane, v read once per group of R rows (nine rows: 8 + 1, two reads of v).  Traffic per sample and node:
// (L + ceil(L / 8)) x 8 bytes.  A lane adds its products in the order of its pieces with one fma each, the block sums the lanes with
// beat_block_sum, block b stores the partial of row l at partials[l * blocks + b] (scratch of the context, made with it), and a
// second launch of one block adds a row's partials in a fixed order and stores out[l] from a vector register.  No atomics.
//
// Bits.  The grid depends on n only and the pieces on n and on the address of v, so the partition of the nodes over lanes and
// blocks is the same for every row and every call: the same input gives the same bits, and row l comes out of a call with L rows
// as out of a call with that row alone (the unrolled trip issues its loads together and keeps the order of the fmas).
//
// Loads of q (BEAT_LEADS_Q_NT, default 0: plain).  NOT MEASURED YET, so the pass loads as every other pass of this library does.
// The rows are read once per sample and never written; on a grid of a user's size they are far larger than the caches (9 rows at
// 512^3: 9.7 GB against 256 MiB), so a line of q that stays in a cache only displaces v, which the launch before this one wrote
// and the next one reads: that speaks for non-temporal loads, and the library's streaming probe found read-only streams of
// 16-byte loads 5 - 10 % faster with them (profiles/r05_streaming.md).  Against: these are 8-byte loads, on a small grid the rows
// ARE cache-resident from one sample to the next, and the ionic kernel was slower with non-temporal rows in 8 of 8 pairs.  -D
// BEAT_LEADS_Q_NT=1 builds the other variant (make BUILD=build_nt LIBNAME=libbeat_hip_nt.so EXTRA=-DBEAT_LEADS_Q_NT=1); what to
// time is written down in profiles/lead_recorder.md.  v is loaded plainly either way.
#include "beat_common.h"

#include <algorithm>

#ifndef BEAT_LEADS_Q_NT
#define BEAT_LEADS_Q_NT 0
#endif

namespace {

constexpr int BEAT_LEADS_ROWS = 8;  // rows per pass over v

template <bool NT>
__device__ __forceinline__ double ld_q(const double* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

template <int R, bool NT>
__global__ __launch_bounds__(BEAT_BLOCK) void leads_partial_kernel(int64_t n, int shift, const double* __restrict__ v,
                                                                   const double* __restrict__ q, int64_t ldq,
                                                                   double* __restrict__ partials) {
  __shared__ double red[4];
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  const int lane = threadIdx.x & 63;
  const int64_t npieces = (n + shift + 63) >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * (BEAT_BLOCK / 64);
  for (int64_t piece = (int64_t)blockIdx.x * (BEAT_BLOCK / 64) + (threadIdx.x >> 6); piece < npieces; piece += 2 * nwaves) {
    // this wave's next two pieces: all loads first, then the fmas in the order of the pieces
    const int64_t i0 = piece * 64 + lane - shift, i1 = i0 + nwaves * 64;
    const bool ok0 = i0 >= 0 && i0 < n, ok1 = i1 < n;  // (i1 > i0 >= -63, and nwaves * 64 >= 256; past the last piece i1 >= n)
    const double v0 = ok0 ? v[i0] : 0.0, v1 = ok1 ? v[i1] : 0.0;
    double q0[R], q1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double* row = q + (int64_t)r * ldq;
      q0[r] = ok0 ? ld_q<NT>(row + i0) : 0.0;
      q1[r] = ok1 ? ld_q<NT>(row + i1) : 0.0;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = fma(q0[r], v0, acc[r]);  // (a masked lane adds 0 * 0: the sum keeps its bits)
      acc[r] = fma(q1[r], v1, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double s = beat_block_sum(acc[r], red);
    if (threadIdx.x == 0) partials[(int64_t)r * gridDim.x + blockIdx.x] = s;
  }
}

// one block: out[l] = sum of row l's block partials, each thread its share in the order of the blocks, then the block sum
__global__ __launch_bounds__(BEAT_BLOCK) void leads_final_kernel(const double* __restrict__ partials, int nblocks, int nleads,
                                                                 double* __restrict__ out) {
  __shared__ double red[4];
  for (int l = 0; l < nleads; ++l) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += BEAT_BLOCK) s += partials[(int64_t)l * nblocks + b];
    s = beat_block_sum(s, red);
    if (threadIdx.x == 0) out[l] = s;
  }
}

template <int R>
void launch_rows(beat_ctx* ctx, unsigned grid, int64_t n, int shift, const double* v, const double* q, int64_t ldq, double* partials) {
  BEAT_KERNEL((leads_partial_kernel<R, BEAT_LEADS_Q_NT != 0>), dim3(grid), dim3(BEAT_BLOCK), 0, ctx->stream, n, shift, v, q, ldq, partials);
}

}  // namespace

// src/beat/ecg.py:282-298: the recovery and the lead integrals of one sample, for all electrodes, as dot products with the potential
extern "C" int beat_field_leads(beat_ctx* ctx, const double* dev_v, int64_t n, const double* dev_q, int64_t ldq, int nleads,
                                double* dev_out) {
  BEAT_REQUIRE(ctx != nullptr && dev_v != nullptr && dev_q != nullptr && dev_out != nullptr, "null argument");
  BEAT_REQUIRE(n > 0, "n must be positive");
  BEAT_REQUIRE(nleads >= 1 && nleads <= BEAT_MAX_LEADS, "nleads must be 1..%d, got %d", BEAT_MAX_LEADS, nleads);
  BEAT_REQUIRE(ldq >= n, "ldq (%lld) is smaller than n (%lld)", (long long)ldq, (long long)n);
  BEAT_REQUIRE((((uintptr_t)dev_v | (uintptr_t)dev_q | (uintptr_t)dev_out) & 7) == 0, "dev_v, dev_q and dev_out must be 8-byte aligned");
  const int shift = (int)(((uintptr_t)dev_v >> 3) & 63);  // nodes between the 512-byte boundary below v and its first node
  // a function of n alone: the pieces of the longest walk (shift = 63), four per block
  const unsigned grid = (unsigned)std::min<int64_t>(BEAT_LEADS_MAX_BLOCKS, (((n + 126) >> 6) + BEAT_BLOCK / 64 - 1) / (BEAT_BLOCK / 64));
  double* partials = ctx->d_lead_partials;
  for (int l0 = 0; l0 < nleads; l0 += BEAT_LEADS_ROWS) {
    const double* q = dev_q + (int64_t)l0 * ldq;
    double* part = partials + (int64_t)l0 * grid;
    switch (std::min(BEAT_LEADS_ROWS, nleads - l0)) {
      case 1: launch_rows<1>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      case 2: launch_rows<2>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      case 3: launch_rows<3>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      case 4: launch_rows<4>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      case 5: launch_rows<5>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      case 6: launch_rows<6>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      case 7: launch_rows<7>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
      default: launch_rows<8>(ctx, grid, n, shift, dev_v, q, ldq, part); break;
    }
  }
  BEAT_KERNEL(leads_final_kernel, dim3(1), dim3(BEAT_BLOCK), 0, ctx->stream, (const double*)partials, (int)grid, nleads, dev_out);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}
