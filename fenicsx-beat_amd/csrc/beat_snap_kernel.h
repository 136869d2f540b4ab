// The field snapshots' sample lattice and pack kernel (see beat_snap.hip, which launches it; include/beat_hip.h: beat_snap_create has
// the rule).  The lattice half is plain C++17 without a HIP call: the kernel runs it on the device, tests/snap_host_harness.cpp on
// the host against NumPy slicing (tests/test_output_cpu.py).  The kernel half is compiled by hipcc only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BEAT_SNAP_FN __host__ __device__ __forceinline__
#else
#define BEAT_SNAP_FN inline
#endif

#ifndef BEAT_SNAP_MAX_FIELDS
#define BEAT_SNAP_MAX_FIELDS 8
#endif

namespace beat_snap_detail {

// The grid (n nodes per axis, x fastest), the box [lo, hi) of node indices and the stride per axis: the sampled nodes are
// lo + k * stride < hi, as the slice lo:hi:stride takes them.
struct SnapGeometry {
  int64_t n[3];
  int64_t lo[3];
  int64_t hi[3];
  int64_t stride[3];
};

// samples along one axis: len(range(lo, hi, stride))
BEAT_SNAP_FN int64_t snap_axis_count(int64_t lo, int64_t hi, int64_t stride) { return hi > lo ? (hi - lo + stride - 1) / stride : 0; }

// The sampled index of the node `rel` nodes above the box's low face (0 <= rel) along an axis of stride `stride`, -1 when the node
// is not on the lattice.  Indices below 2^32 take the 32-bit division (a handful of instructions on the device instead of a
// hundred); the result is the same.
BEAT_SNAP_FN int64_t snap_axis_sample(int64_t rel, int64_t stride) {
  if (stride == 1) return rel;
  if (((uint64_t)rel | (uint64_t)stride) >> 32 == 0) {
    const uint32_t r = (uint32_t)rel, s = (uint32_t)stride, q = r / s;
    return q * s == r ? (int64_t)q : -1;
  }
  const int64_t q = rel / stride;
  return q * stride == rel ? q : -1;
}

// Which sample the node (ix, iy, iz) of the grid is: its index in the frame (x fastest: xs + nxs * (ys + nys * zs)), or -1 for a node
// outside the box or off the lattice.
BEAT_SNAP_FN int64_t snap_node_sample(const SnapGeometry& g, int64_t ix, int64_t iy, int64_t iz) {
  const int64_t i[3] = {ix, iy, iz};
  int64_t s[3];
  for (int a = 0; a < 3; ++a) {
    if (i[a] < g.lo[a] || i[a] >= g.hi[a]) return -1;
    s[a] = snap_axis_sample(i[a] - g.lo[a], g.stride[a]);
    if (s[a] < 0) return -1;
  }
  const int64_t nxs = snap_axis_count(g.lo[0], g.hi[0], g.stride[0]), nys = snap_axis_count(g.lo[1], g.hi[1], g.stride[1]);
  return s[0] + nxs * (s[1] + nys * s[2]);
}

// nodes between the 512-byte boundary below an address and the address
BEAT_SNAP_FN int snap_row_shift(uint64_t address) { return (int)((address >> 3) & 63); }

}  // namespace beat_snap_detail

#if defined(__HIPCC__)
#include "beat_common.h"

namespace beat_snap_detail {

struct SnapFields {
  const double* f[BEAT_SNAP_MAX_FIELDS];
};

struct SnapLaunch {
  SnapGeometry g;
  int64_t ns[3];              // samples per axis
  int64_t frame_items;        // ns[0] * ns[1] * ns[2]
  int nfields;
  int stats;                  // 1: every row of the box is read, for min / max / nonfinite; 0: the lattice's rows only
  double fill;                // what a sample outside the tissue gets
  const unsigned char* mask;  // a byte per node of the grid, 0 = outside the tissue; null: all inside
};

// thread 0's (mn, mx, cnt) become those of the block; smem holds 12 doubles.  The order of the comparisons is fixed.
__device__ __forceinline__ void snap_block_reduce(double& mn, double& mx, double& cnt, double* smem) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    cnt += __shfl_down(cnt, off, 64);
    if (a < mn) mn = a;
    if (b > mx) mx = b;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (smem is reused from field to field)
  if (lane == 0) {
    smem[3 * wave] = mn;
    smem[3 * wave + 1] = mx;
    smem[3 * wave + 2] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BEAT_BLOCK / 64; ++w) {
      if (smem[3 * w] < mn) mn = smem[3 * w];
      if (smem[3 * w + 1] > mx) mx = smem[3 * w + 1];
      cnt += smem[3 * w + 2];
    }
  }
}

// One pass over the box of up to BEAT_SNAP_MAX_FIELDS fields.  blockIdx.x strides over the box's y rows, blockIdx.y over its z planes,
// blockIdx.z and the block's four waves over the 512-byte pieces of an x row; a piece is aligned in memory for the first field (the
// first piece of a row starts up to 63 nodes before the box and masks those lanes: no address is formed for them), so a wave reads
// whole coalesced rows whatever the stride.  Only lanes on the lattice store, one sample each, into the frame of their field
// (frames lie frame_items samples apart in `out`).  Every tissue node of the box enters the statistics; the block's partials go to
// partials[(field * nblocks + block) * 3 + {0 min, 1 max, 2 nonfinite}], no atomics.  NaN is counted and takes no part in min / max;
// an infinity is counted and does.  Plain loads, or non-temporal ones (NT): a choice to measure (tools/bench_output.py).  NF >= nfields
// is how many fields the instance keeps statistics registers for (1, 2, 4 or 8: six VGPRs per field decide how many waves a SIMD holds).
template <bool F32, bool NT, int NF>
__global__ __launch_bounds__(BEAT_BLOCK) void snap_pack_kernel(SnapLaunch a, SnapFields fields, void* __restrict__ out,
                                                                double* __restrict__ partials) {
  __shared__ double smem[3 * (BEAT_BLOCK / 64)];
  const SnapGeometry& g = a.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t len_x = g.hi[0] - g.lo[0];
  const bool stats = a.stats != 0;
  // rows walked: every row of the box with the statistics, the lattice's rows without
  const int64_t rows_y = stats ? g.hi[1] - g.lo[1] : a.ns[1], rows_z = stats ? g.hi[2] - g.lo[2] : a.ns[2];
  double mn[NF], mx[NF], cnt[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    mn[f] = __builtin_huge_val();
    mx[f] = -__builtin_huge_val();
    cnt[f] = 0.0;
  }
  for (int64_t jz = blockIdx.y; jz < rows_z; jz += gridDim.y) {
    const int64_t zb = stats ? jz : jz * g.stride[2];            // nodes above the box's low z face
    const int64_t zs = stats ? snap_axis_sample(zb, g.stride[2]) : jz;
    for (int64_t jy = blockIdx.x; jy < rows_y; jy += gridDim.x) {
      const int64_t yb = stats ? jy : jy * g.stride[1];
      const int64_t ys = stats ? snap_axis_sample(yb, g.stride[1]) : jy;
      const bool row_on = zs >= 0 && ys >= 0;
      const int64_t row0 = g.lo[0] + g.n[0] * ((g.lo[1] + yb) + g.n[1] * (g.lo[2] + zb));  // the row's first node in the box
      const int64_t out0 = a.ns[0] * (ys + a.ns[1] * zs);                                   // its first sample in a frame
      const int shift = snap_row_shift((uint64_t)(uintptr_t)(fields.f[0] + row0));
      const int64_t npieces = (len_x + shift + 63) >> 6;
      for (int64_t piece = (int64_t)blockIdx.z * (BEAT_BLOCK / 64) + wave; piece < npieces;
           piece += (int64_t)gridDim.z * (BEAT_BLOCK / 64)) {
        const int64_t xb = piece * 64 + lane - shift;  // nodes above the box's low x face
        if (xb < 0 || xb >= len_x) continue;
        const int64_t node = row0 + xb;
        const bool tissue = a.mask == nullptr || a.mask[node] != 0;
        const int64_t xs = row_on ? snap_axis_sample(xb, g.stride[0]) : -1;
        if (!tissue && xs < 0) continue;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          if (f < a.nfields) {
            double v = a.fill;
            if (tissue) {
              v = NT ? __builtin_nontemporal_load(fields.f[f] + node) : fields.f[f][node];
              if (stats) {
                if (v < mn[f]) mn[f] = v;
                if (v > mx[f]) mx[f] = v;
                if (!(fabs(v) <= 1.7976931348623157e308)) cnt[f] += 1.0;
              }
            }
            if (xs >= 0) {
              const int64_t o = (int64_t)f * a.frame_items + out0 + xs;
              if constexpr (F32)
                static_cast<float*>(out)[o] = static_cast<float>(v);
              else
                static_cast<double*>(out)[o] = v;
            }
          }
        }
      }
    }
  }
  if (!stats) return;  // (uniform over the launch)
  const int64_t nblocks = (int64_t)gridDim.x * gridDim.y * gridDim.z;
  const int64_t block = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (f < a.nfields) {
      snap_block_reduce(mn[f], mx[f], cnt[f], smem);
      if (threadIdx.x == 0) {
        double* p = partials + ((int64_t)f * nblocks + block) * 3;
        p[0] = mn[f];
        p[1] = mx[f];
        p[2] = cnt[f];
      }
    }
  }
}

}  // namespace beat_snap_detail
#endif  // __HIPCC__
