// Rule-based fibre, sheet and sheet-normal fields of a voxel geometry, from nodal harmonic fields that are already on the device.
// The reference's ventricular demos get theirs from a Laplace-Dirichlet rule-based generator over FEniCSx
//   demos/lv_endocardial.py, demos/biv_endocardial.py, demos/ukb_atlas.py   cardiac_geometries(create_fibers=True, fiber_angle_endo=60,
//                                                                           fiber_angle_epi=-60)
// and hand them to define_conductivity_tensor (src/beat/conductivities.py:107-118).  Here the two harmonic fields come from
// beat.utils.laplace_dirichlet; the step between them and the assembly (nodal fields -> per-voxel orthonormal frame -> per-voxel
// tensor) would otherwise be a NumPy pass over the whole box and a 72 bytes-per-voxel upload.
//
// The kernel.  One thread per voxel, x fastest, grid-stride, 64-bit voxel and node indices.  The eight corner rows of a wave are runs of
// consecutive nodes, so its loads are coalesced and overlap in cache; no LDS.  The rule itself is beat_fibres_kernel.h's, the same text
// the host harness runs.  Outputs are row-per-voxel ((nvoxels, 3) and (nvoxels, 9)): a wave's stores cover one contiguous range.
// Degenerate voxels are counted per thread, summed over the wave and added with one integer atomic per wave that has any (the count does
// not depend on the order).  A set-up kernel: nothing here has been tuned (one timing, as information: profiles/fibres_rule.md).
// Two ventricles (beat_fibres_biv_rule, Bayer's rule with bislerp) take the same walk over three transmural fields: fibres_biv_kernel.
#include <algorithm>

#include "beat_common.h"
#include "beat_fibres_kernel.h"

namespace {

using namespace beat_fibres_detail;

struct FibreArgs {
  int64_t cx, cy, cz;
  double h[3];
  double axis[3];
  const double* phi;
  const double* psi;  // null: axis
  const unsigned char* active;
  double alpha_endo, alpha_epi, beta_endo, beta_epi, s_l, s_t;
  double* f;
  double* s;
  double* n;
  double* M;
  unsigned long long* degenerate;
};

__global__ __launch_bounds__(BEAT_BLOCK) void fibres_kernel(FibreArgs a) {
  const int64_t nvox = a.cx * a.cy * a.cz;
  const int64_t nx = a.cx + 1, plane = nx * (a.cy + 1);
  const int64_t stride = (int64_t)gridDim.x * BEAT_BLOCK;
  unsigned long long mine = 0;
  const double h[3] = {a.h[0], a.h[1], a.h[2]}, axis[3] = {a.axis[0], a.axis[1], a.axis[2]};
  for (int64_t v = (int64_t)blockIdx.x * BEAT_BLOCK + threadIdx.x; v < nvox; v += stride) {
    double f[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0}, M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.active == nullptr || a.active[v] != 0) {
      const int64_t ix = v % a.cx, iy = (v / a.cx) % a.cy, iz = v / (a.cx * a.cy);
      const int64_t base = ix + nx * iy + plane * iz;  // corner c: base + (c & 1) + nx ((c >> 1) & 1) + plane ((c >> 2) & 1) < nodes
      double phi[8], psi[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int64_t node = base + (c & 1) + nx * ((c >> 1) & 1) + plane * ((c >> 2) & 1);
        phi[c] = a.phi[node];
        if (a.psi != nullptr) psi[c] = a.psi[node];
      }
      // (two call sites, each with its null pointer known at compile time, and the tensor always formed: no array is chosen through a
      // pointer at run time, which would put it into scratch memory)
      bool deg;
      if (a.psi != nullptr)
        deg = beat_fibres_voxel(phi, psi, h, nullptr, a.alpha_endo, a.alpha_epi, a.beta_endo, a.beta_epi, f, s, n, a.s_l, a.s_t, M);
      else
        deg = beat_fibres_voxel(phi, nullptr, h, axis, a.alpha_endo, a.alpha_epi, a.beta_endo, a.beta_epi, f, s, n, a.s_l, a.s_t, M);
      mine += deg ? 1u : 0u;
    }  // (an inactive voxel: zeros everywhere, the tensor included -- the assembly does not read it -- and not counted)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.f != nullptr) a.f[3 * v + k] = f[k];
      if (a.s != nullptr) a.s[3 * v + k] = s[k];
      if (a.n != nullptr) a.n[3 * v + k] = n[k];
    }
    if (a.M != nullptr) {
#pragma unroll
      for (int q = 0; q < 9; ++q) a.M[9 * v + q] = M[q];
    }
  }
  // every lane is back here: one add per wave that saw a degenerate voxel
  unsigned long long total = mine;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
  if ((threadIdx.x & 63) == 0 && total != 0) atomicAdd(a.degenerate, total);
}

// The bi-ventricular rule (beat_fibres_biv_rule): the same walk with three transmural fields, so 24 or 32 corner loads per voxel, and
// beat_fibres_biv_voxel in place of beat_fibres_voxel.  Three frames, two quaternion blends and some twenty sin / cos / atan2 per
// voxel: still a set-up kernel, timed once (profiles/fibres_biv.md).
struct FibreBivArgs {
  int64_t cx, cy, cz;
  double h[3];
  double axis[3];
  const double* phi_lv;
  const double* phi_rv;
  const double* phi_epi;
  const double* psi;  // null: axis
  const unsigned char* active;
  double alpha_endo, alpha_epi, beta_endo, beta_epi, s_l, s_t;
  double* f;
  double* s;
  double* n;
  double* M;
  unsigned long long* degenerate;
};

__global__ __launch_bounds__(BEAT_BLOCK) void fibres_biv_kernel(FibreBivArgs a) {
  const int64_t nvox = a.cx * a.cy * a.cz;
  const int64_t nx = a.cx + 1, plane = nx * (a.cy + 1);
  const int64_t stride = (int64_t)gridDim.x * BEAT_BLOCK;
  unsigned long long mine = 0;
  const double h[3] = {a.h[0], a.h[1], a.h[2]}, axis[3] = {a.axis[0], a.axis[1], a.axis[2]};
  for (int64_t v = (int64_t)blockIdx.x * BEAT_BLOCK + threadIdx.x; v < nvox; v += stride) {
    double f[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0}, M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.active == nullptr || a.active[v] != 0) {
      const int64_t ix = v % a.cx, iy = (v / a.cx) % a.cy, iz = v / (a.cx * a.cy);
      const int64_t base = ix + nx * iy + plane * iz;  // corner c: base + (c & 1) + nx ((c >> 1) & 1) + plane ((c >> 2) & 1) < nodes
      double lv[8], rv[8], epi[8], psi[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int64_t node = base + (c & 1) + nx * ((c >> 1) & 1) + plane * ((c >> 2) & 1);
        lv[c] = a.phi_lv[node];
        rv[c] = a.phi_rv[node];
        epi[c] = a.phi_epi[node];
        if (a.psi != nullptr) psi[c] = a.psi[node];
      }
      // (two call sites, as in fibres_kernel: each null pointer is known at compile time)
      bool deg;
      if (a.psi != nullptr)
        deg = beat_fibres_biv_voxel(lv, rv, epi, psi, h, nullptr, a.alpha_endo, a.alpha_epi, a.beta_endo, a.beta_epi, f, s, n, a.s_l,
                                    a.s_t, M);
      else
        deg = beat_fibres_biv_voxel(lv, rv, epi, nullptr, h, axis, a.alpha_endo, a.alpha_epi, a.beta_endo, a.beta_epi, f, s, n, a.s_l,
                                    a.s_t, M);
      mine += deg ? 1u : 0u;
    }  // (an inactive voxel: zeros everywhere and not counted)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.f != nullptr) a.f[3 * v + k] = f[k];
      if (a.s != nullptr) a.s[3 * v + k] = s[k];
      if (a.n != nullptr) a.n[3 * v + k] = n[k];
    }
    if (a.M != nullptr) {
#pragma unroll
      for (int q = 0; q < 9; ++q) a.M[9 * v + q] = M[q];
    }
  }
  // every lane is back here: one add per wave that saw a degenerate voxel
  unsigned long long total = mine;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
  if ((threadIdx.x & 63) == 0 && total != 0) atomicAdd(a.degenerate, total);
}

}  // namespace

extern "C" int beat_fibres_rule(beat_ctx* ctx, const int64_t cells[3], const double h[3], const double* dev_phi, const double* dev_psi,
                                const double axis[3], const unsigned char* dev_active, double alpha_endo, double alpha_epi,
                                double beta_endo, double beta_epi, double s_l, double s_t, double* dev_f, double* dev_s, double* dev_n,
                                double* dev_M, int64_t* dev_degenerate) {
  BEAT_REQUIRE(ctx != nullptr && cells != nullptr && h != nullptr && dev_phi != nullptr && dev_degenerate != nullptr, "null argument");
  BEAT_REQUIRE(dev_psi != nullptr || axis != nullptr, "no longitudinal input: neither dev_psi nor axis");
  BEAT_REQUIRE(dev_f != nullptr || dev_s != nullptr || dev_n != nullptr || dev_M != nullptr, "no output asked for");
  BEAT_REQUIRE(cells[0] >= 1 && cells[1] >= 1 && cells[2] >= 1, "cells must be positive, got (%lld, %lld, %lld)", (long long)cells[0],
               (long long)cells[1], (long long)cells[2]);
  BEAT_REQUIRE(cells[0] < ((int64_t)1 << 20) && cells[1] < ((int64_t)1 << 20) && cells[2] < ((int64_t)1 << 20) &&
                   (cells[0] + 1) * (cells[1] + 1) * (cells[2] + 1) < ((int64_t)1 << 40),
               "grid too large");
  BEAT_REQUIRE(h[0] > 0.0 && h[1] > 0.0 && h[2] > 0.0, "spacings must be positive");
  BEAT_REQUIRE((((uintptr_t)dev_phi | (uintptr_t)dev_psi | (uintptr_t)dev_f | (uintptr_t)dev_s | (uintptr_t)dev_n | (uintptr_t)dev_M |
                 (uintptr_t)dev_degenerate) & 7) == 0, "a pointer is not 8-byte aligned");
  FibreArgs a{};
  a.cx = cells[0];
  a.cy = cells[1];
  a.cz = cells[2];
  for (int k = 0; k < 3; ++k) {
    a.h[k] = h[k];
    a.axis[k] = (dev_psi == nullptr) ? axis[k] : 0.0;
  }
  a.phi = dev_phi;
  a.psi = dev_psi;
  a.active = dev_active;
  a.alpha_endo = alpha_endo;
  a.alpha_epi = alpha_epi;
  a.beta_endo = beta_endo;
  a.beta_epi = beta_epi;
  a.s_l = s_l;
  a.s_t = s_t;
  a.f = dev_f;
  a.s = dev_s;
  a.n = dev_n;
  a.M = dev_M;
  a.degenerate = reinterpret_cast<unsigned long long*>(dev_degenerate);
  const int64_t nvox = a.cx * a.cy * a.cz;
  const unsigned grid = (unsigned)std::min<int64_t>(2048, (nvox + BEAT_BLOCK - 1) / BEAT_BLOCK);
  BEAT_KERNEL(fibres_kernel, dim3(grid), dim3(BEAT_BLOCK), 0, ctx->stream, a);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}

extern "C" int beat_fibres_biv_rule(beat_ctx* ctx, const int64_t cells[3], const double h[3], const double* dev_phi_lv,
                                    const double* dev_phi_rv, const double* dev_phi_epi, const double* dev_psi, const double axis[3],
                                    const unsigned char* dev_active, double alpha_endo, double alpha_epi, double beta_endo,
                                    double beta_epi, double s_l, double s_t, double* dev_f, double* dev_s, double* dev_n, double* dev_M,
                                    int64_t* dev_degenerate) {
  BEAT_REQUIRE(ctx != nullptr && cells != nullptr && h != nullptr && dev_phi_lv != nullptr && dev_phi_rv != nullptr &&
                   dev_phi_epi != nullptr && dev_degenerate != nullptr, "null argument");
  BEAT_REQUIRE(dev_psi != nullptr || axis != nullptr, "no longitudinal input: neither dev_psi nor axis");
  BEAT_REQUIRE(dev_f != nullptr || dev_s != nullptr || dev_n != nullptr || dev_M != nullptr, "no output asked for");
  BEAT_REQUIRE(cells[0] >= 1 && cells[1] >= 1 && cells[2] >= 1, "cells must be positive, got (%lld, %lld, %lld)", (long long)cells[0],
               (long long)cells[1], (long long)cells[2]);
  BEAT_REQUIRE(cells[0] < ((int64_t)1 << 20) && cells[1] < ((int64_t)1 << 20) && cells[2] < ((int64_t)1 << 20) &&
                   (cells[0] + 1) * (cells[1] + 1) * (cells[2] + 1) < ((int64_t)1 << 40),
               "grid too large");
  BEAT_REQUIRE(h[0] > 0.0 && h[1] > 0.0 && h[2] > 0.0, "spacings must be positive");
  BEAT_REQUIRE((((uintptr_t)dev_phi_lv | (uintptr_t)dev_phi_rv | (uintptr_t)dev_phi_epi | (uintptr_t)dev_psi | (uintptr_t)dev_f |
                 (uintptr_t)dev_s | (uintptr_t)dev_n | (uintptr_t)dev_M | (uintptr_t)dev_degenerate) & 7) == 0,
               "a pointer is not 8-byte aligned");
  FibreBivArgs a{};
  a.cx = cells[0];
  a.cy = cells[1];
  a.cz = cells[2];
  for (int k = 0; k < 3; ++k) {
    a.h[k] = h[k];
    a.axis[k] = (dev_psi == nullptr) ? axis[k] : 0.0;
  }
  a.phi_lv = dev_phi_lv;
  a.phi_rv = dev_phi_rv;
  a.phi_epi = dev_phi_epi;
  a.psi = dev_psi;
  a.active = dev_active;
  a.alpha_endo = alpha_endo;
  a.alpha_epi = alpha_epi;
  a.beta_endo = beta_endo;
  a.beta_epi = beta_epi;
  a.s_l = s_l;
  a.s_t = s_t;
  a.f = dev_f;
  a.s = dev_s;
  a.n = dev_n;
  a.M = dev_M;
  a.degenerate = reinterpret_cast<unsigned long long*>(dev_degenerate);
  const int64_t nvox = a.cx * a.cy * a.cz;
  const unsigned grid = (unsigned)std::min<int64_t>(2048, (nvox + BEAT_BLOCK - 1) / BEAT_BLOCK);
  BEAT_KERNEL(fibres_biv_kernel, dim3(grid), dim3(BEAT_BLOCK), 0, ctx->stream, a);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}
