// Implicit Runge-Kutta stages of the monodomain PDE (beat.irksome_model): the complex-shifted solve of a fully implicit
// stage, its right-hand sides and the step's final update.  Replaces what Irksome's StageDerivativeTimeStepper hands to
// PETSc (src/beat/irksome_model.py:57-69, advance() at :96): one coupled solve of all stages, here diagonalised on the host
// (beat/butcher.py) into one shifted solve per eigenvalue of the Butcher matrix.
//
// Operator of a stage: S = a Mass + (b + i c) K on the constant-coefficient tables of the operator (27 node types).  For
// c != 0 it is complex symmetric with an SPD real part (a, b > 0): Jacobi-preconditioned COCG, i.e. CG with the unconjugated
// bilinear form p^T q; stopping test ||r||_2 <= max(rtol ||b||_2, atol) with the conjugated norm, as PETSc's KSP reports it.
// For c == 0 and a real right-hand side the same kernels run their real instantiation: plain Jacobi-PCG.
//
// Split-complex layout: the real and the imaginary part are two ordinary fields (one ghost plane on either side,
// include/beat_hip.h), so every field of the operator's geometry can be an operand.  Single slab (physical z faces) only.
//
// Traffic per COCG iteration: apply 32 B/node (p in, q out), update 96 (x, r, p, q in; x, r out), direction 48 (r, p in; p
// out): 176 B/node, twice the 88 of the real iteration.  The stencil reads its 15 neighbours straight from global memory
// (x-neighbours from the same cache lines, the y / z rows from L2): no LDS staging.
#include "beat_pde_internal.h"
#include "beat_pde_device.h"

#include <cmath>
#include <vector>

namespace {
using namespace beat_pde_detail;

// (dx, dy, dz) of the 15 stencil points (kOffsets of beat_pde.hip, which device code cannot read)
constexpr int kOff[45] = {0, 0, 0,  1, 0, 0,  -1, 0, 0,  0, 1, 0,  0, -1, 0,  0, 0, 1,  0, 0, -1,
                          1, 1, 0,  -1, -1, 0,  0, 1, 1,  0, -1, -1,  1, 0, 1,  -1, 0, -1,
                          1, 1, 1,  -1, -1, -1};

// slots of the COCG scalar state (device, 32 doubles at the end of the work array)
enum Z {
  Z_BB = 0, Z_RZ_RE, Z_RZ_IM, Z_RR, Z_PQ_RE, Z_PQ_IM, Z_RZN_RE, Z_RZN_IM, Z_RRN, Z_TOL2, Z_BETA_RE, Z_BETA_IM,
  Z_STOP, Z_ITERS, Z_REASON, Z_RTOL, Z_MAXIT, Z_ALPHA_RE, Z_ALPHA_IM, Z_SLOTS = 32
};

// The shifted operator: interior coefficients by value (SGPRs), the 26 boundary rows from the operator's padded device tables.
struct ZOp {
  double re[15], im[15];       // interior row: a M + b K, c K
  double dre, dim;             // interior 1 / diag (complex)
  const double* tm;            // Mass table (27 x TABW)
  const double* tk;            // K table
  double a, b, c;
};

// 1 / diag(S) of a node type
__device__ __forceinline__ void zdinv(const ZOp& op, int type, double& dr, double& di) {
  if (type == 13) {
    dr = op.dre;
    di = op.dim;
    return;
  }
  const double m0 = op.tm[type * TABW], k0 = op.tk[type * TABW];
  const double xr = op.a * m0 + op.b * k0, xi = op.c * k0;
  const double den = xr * xr + xi * xi;
  dr = den != 0.0 ? xr / den : 0.0;
  di = den != 0.0 ? -xi / den : 0.0;
}

// Gather the 15 neighbours of node (ix, iy, iz) of field f; 0 outside the box.
__device__ __forceinline__ void gather15(const double* __restrict__ f, const Geom& g, int ix, int iy, int iz, int64_t i,
                                         double (&v)[15]) {
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    const int dx = kOff[3 * k], dy = kOff[3 * k + 1], dz = kOff[3 * k + 2];
    const bool in = (unsigned)(ix + dx) < (unsigned)g.nx && (unsigned)(iy + dy) < (unsigned)g.ny &&
                    (unsigned)(iz + dz) < (unsigned)g.nz;
    v[k] = in ? f[i + dx + (int64_t)dy * g.nx + (int64_t)dz * g.plane] : 0.0;
  }
}

// q = S p; partials of the unconjugated p^T q (re, im) when `partials` is set.  Latched: nothing to do.
template <bool CPLX>
__global__ __launch_bounds__(BEAT_BLOCK) void zapply_kernel(Geom g, ZOp op, const double* __restrict__ st,
                                                            const double* __restrict__ pre, const double* __restrict__ pim,
                                                            double* __restrict__ qre, double* __restrict__ qim,
                                                            double* __restrict__ partials) {
  __shared__ double red[4];
  if (st != nullptr && st[Z_STOP] != 0.0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrows = g.ny * g.nz;
  double s_re = 0.0, s_im = 0.0;
  for (int row = blockIdx.x * 4 + wave; row < nrows; row += gridDim.x * 4) {
    const int iz = row / g.ny, iy = row - iz * g.ny;
    const int tyz = 3 * axis_type(iy, g.ny, 1, 1) + 9 * axis_type(iz, g.nz, 1, 1);
    const int64_t base = (int64_t)row * g.nx;
    for (int ix = lane; ix < g.nx; ix += 64) {
      const int type = axis_type(ix, g.nx, 1, 1) + tyz;
      const int64_t i = base + ix;
      double vr[15], vi[15];
      gather15(pre, g, ix, iy, iz, i, vr);
      if (CPLX) gather15(pim, g, ix, iy, iz, i, vi);
      double ar = 0.0, ai = 0.0;
      if (type == 13) {
#pragma unroll
        for (int k = 0; k < 15; ++k) {
          ar = fma(op.re[k], vr[k], ar);
          if (CPLX) {
            ar = fma(-op.im[k], vi[k], ar);
            ai = fma(op.re[k], vi[k], ai);
            ai = fma(op.im[k], vr[k], ai);
          }
        }
      } else {
        const double* __restrict__ rm = op.tm + type * TABW;
        const double* __restrict__ rk = op.tk + type * TABW;
#pragma unroll
        for (int k = 0; k < 15; ++k) {
          const double cr = op.a * rm[k] + op.b * rk[k];
          ar = fma(cr, vr[k], ar);
          if (CPLX) {
            const double ci = op.c * rk[k];
            ar = fma(-ci, vi[k], ar);
            ai = fma(cr, vi[k], ai);
            ai = fma(ci, vr[k], ai);
          }
        }
      }
      qre[i] = ar;
      if (CPLX) qim[i] = ai;
      s_re = fma(vr[0], ar, s_re);
      if (CPLX) {
        s_re = fma(-vi[0], ai, s_re);
        s_im = fma(vr[0], ai, s_im);
        s_im = fma(vi[0], ar, s_im);
      }
    }
  }
  if (partials != nullptr) {
    const double a0 = beat_block_sum(s_re, red);
    const double a1 = CPLX ? beat_block_sum(s_im, red) : 0.0;
    if (threadIdx.x == 0) {
      partials[blockIdx.x] = a0;
      partials[BEAT_MAX_PARTIALS + blockIdx.x] = a1;
    }
  }
}

// Start of a solve from x = 0: r = rhs, p = D^-1 r; partials of r^T D^-1 r (re, im) and ||r||^2.
template <bool CPLX>
__global__ __launch_bounds__(BEAT_BLOCK) void zbegin_kernel(Geom g, ZOp op, const double* __restrict__ bre,
                                                            const double* __restrict__ bim, double* __restrict__ xre,
                                                            double* __restrict__ xim, double* __restrict__ rre,
                                                            double* __restrict__ rim, double* __restrict__ pre,
                                                            double* __restrict__ pim, double* __restrict__ partials) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrows = g.ny * g.nz;
  double s_zr = 0.0, s_zi = 0.0, s_rr = 0.0;
  for (int row = blockIdx.x * 4 + wave; row < nrows; row += gridDim.x * 4) {
    const int iz = row / g.ny, iy = row - iz * g.ny;
    const int tyz = 3 * axis_type(iy, g.ny, 1, 1) + 9 * axis_type(iz, g.nz, 1, 1);
    const int64_t base = (int64_t)row * g.nx;
    for (int ix = lane; ix < g.nx; ix += 64) {
      const int type = axis_type(ix, g.nx, 1, 1) + tyz;
      const int64_t i = base + ix;
      double dr, di;
      zdinv(op, type, dr, di);
      const double r0 = bre[i], r1 = CPLX ? bim[i] : 0.0;
      const double z0 = dr * r0 - di * r1, z1 = dr * r1 + di * r0;
      xre[i] = 0.0;
      rre[i] = r0;
      pre[i] = CPLX ? z0 : dr * r0;
      if (CPLX) {
        xim[i] = 0.0;
        rim[i] = r1;
        pim[i] = z1;
        s_zr = fma(r0, z0, fma(-r1, z1, s_zr));
        s_zi = fma(r0, z1, fma(r1, z0, s_zi));
        s_rr = fma(r0, r0, fma(r1, r1, s_rr));
      } else {
        s_zr = fma(r0, dr * r0, s_zr);
        s_rr = fma(r0, r0, s_rr);
      }
    }
  }
  const double a0 = beat_block_sum(s_zr, red);
  const double a1 = beat_block_sum(s_zi, red);
  const double a2 = beat_block_sum(s_rr, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = a0;
    partials[BEAT_MAX_PARTIALS + blockIdx.x] = a1;
    partials[2 * BEAT_MAX_PARTIALS + blockIdx.x] = a2;
  }
}

// alpha = rz / pq; x += alpha p; r -= alpha q; partials of r^T D^-1 r (re, im) and ||r||^2.
template <bool CPLX>
__global__ __launch_bounds__(BEAT_BLOCK) void zupdate_kernel(Geom g, ZOp op, const double* __restrict__ st,
                                                             double* __restrict__ xre, double* __restrict__ xim,
                                                             double* __restrict__ rre, double* __restrict__ rim,
                                                             const double* __restrict__ pre, const double* __restrict__ pim,
                                                             const double* __restrict__ qre, const double* __restrict__ qim,
                                                             double* __restrict__ partials) {
  __shared__ double red[4];
  if (st[Z_STOP] != 0.0) return;
  const double alr = st[Z_ALPHA_RE], ali = st[Z_ALPHA_IM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrows = g.ny * g.nz;
  double s_zr = 0.0, s_zi = 0.0, s_rr = 0.0;
  for (int row = blockIdx.x * 4 + wave; row < nrows; row += gridDim.x * 4) {
    const int iz = row / g.ny, iy = row - iz * g.ny;
    const int tyz = 3 * axis_type(iy, g.ny, 1, 1) + 9 * axis_type(iz, g.nz, 1, 1);
    const int64_t base = (int64_t)row * g.nx;
    for (int ix = lane; ix < g.nx; ix += 64) {
      const int type = axis_type(ix, g.nx, 1, 1) + tyz;
      const int64_t i = base + ix;
      double dr, di;
      zdinv(op, type, dr, di);
      if (CPLX) {
        const double p0 = pre[i], p1 = pim[i], q0 = qre[i], q1 = qim[i];
        xre[i] = xre[i] + (alr * p0 - ali * p1);
        xim[i] = xim[i] + (alr * p1 + ali * p0);
        const double r0 = rre[i] - (alr * q0 - ali * q1);
        const double r1 = rim[i] - (alr * q1 + ali * q0);
        rre[i] = r0;
        rim[i] = r1;
        const double z0 = dr * r0 - di * r1, z1 = dr * r1 + di * r0;
        s_zr = fma(r0, z0, fma(-r1, z1, s_zr));
        s_zi = fma(r0, z1, fma(r1, z0, s_zi));
        s_rr = fma(r0, r0, fma(r1, r1, s_rr));
      } else {
        xre[i] = fma(alr, pre[i], xre[i]);
        const double r0 = fma(-alr, qre[i], rre[i]);
        rre[i] = r0;
        s_zr = fma(r0 * dr, r0, s_zr);
        s_rr = fma(r0, r0, s_rr);
      }
    }
  }
  const double a0 = beat_block_sum(s_zr, red);
  const double a1 = beat_block_sum(s_zi, red);
  const double a2 = beat_block_sum(s_rr, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = a0;
    partials[BEAT_MAX_PARTIALS + blockIdx.x] = a1;
    partials[2 * BEAT_MAX_PARTIALS + blockIdx.x] = a2;
  }
}

// p = D^-1 r + beta p
template <bool CPLX>
__global__ __launch_bounds__(BEAT_BLOCK) void zdirection_kernel(Geom g, ZOp op, const double* __restrict__ st,
                                                                const double* __restrict__ rre, const double* __restrict__ rim,
                                                                double* __restrict__ pre, double* __restrict__ pim) {
  if (st[Z_STOP] != 0.0) return;
  const double br = st[Z_BETA_RE], bi = st[Z_BETA_IM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrows = g.ny * g.nz;
  for (int row = blockIdx.x * 4 + wave; row < nrows; row += gridDim.x * 4) {
    const int iz = row / g.ny, iy = row - iz * g.ny;
    const int tyz = 3 * axis_type(iy, g.ny, 1, 1) + 9 * axis_type(iz, g.nz, 1, 1);
    const int64_t base = (int64_t)row * g.nx;
    for (int ix = lane; ix < g.nx; ix += 64) {
      const int type = axis_type(ix, g.nx, 1, 1) + tyz;
      const int64_t i = base + ix;
      double dr, di;
      zdinv(op, type, dr, di);
      if (CPLX) {
        const double r0 = rre[i], r1 = rim[i], p0 = pre[i], p1 = pim[i];
        pre[i] = (dr * r0 - di * r1) + (br * p0 - bi * p1);
        pim[i] = (dr * r1 + di * r0) + (br * p1 + bi * p0);
      } else {
        pre[i] = fma(br, pre[i], dr * rre[i]);
      }
    }
  }
}

// (ar + i ai) / (br + i bi) by Smith's scaling: |b|^2 is never formed, so the quotient of two dot products stays finite
// wherever both are (|b| below 1e-154 or above 1e154 under- / overflows |b|^2); for bi = 0 it is the plain real division.
__device__ __forceinline__ void zdiv(double ar, double ai, double br, double bi, double& cr, double& ci) {
  if (fabs(bi) <= fabs(br)) {
    const double t = bi / br, den = br + bi * t;
    cr = (ar + ai * t) / den;
    ci = (ai - ar * t) / den;
  } else {
    const double t = br / bi, den = br * t + bi;
    cr = (ar * t + ai) / den;
    ci = (ai * t - ar) / den;
  }
}

// Fixed-order sum of `nsum` block partials, then the scalar step of the stage that produced them:
//  0 start (sums r^T z, ||r||^2): tolerance, latch;  1 after the apply (sums p^T q): alpha, breakdown latch;
//  2 after the update (sums r^T z, ||r||^2): beta, roll, iteration count, latch.
__global__ __launch_bounds__(BEAT_BLOCK) void zscalar_kernel(const double* __restrict__ partials, int count, int step,
                                                             double* st, double rtol, double atol, double max_it) {
  __shared__ double red[4];
  if (step != 0 && st[Z_STOP] != 0.0) return;
  const int nsum = step == 1 ? 2 : 3;
  double s[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < nsum; ++k) {
    double v = 0.0;
    for (int i = threadIdx.x; i < count; i += BEAT_BLOCK) v += partials[(int64_t)k * BEAT_MAX_PARTIALS + i];
    s[k] = beat_block_sum(v, red);
  }
  if (threadIdx.x != 0) return;
  if (step == 0) {
    const double rr = s[2];
    const double tr = rtol * rtol * rr, ta = atol * atol;  // x0 = 0: b = r
    st[Z_BB] = rr;
    st[Z_RR] = rr;
    st[Z_RZ_RE] = s[0];
    st[Z_RZ_IM] = s[1];
    st[Z_TOL2] = tr > ta ? tr : ta;
    st[Z_RTOL] = rtol;
    st[Z_MAXIT] = max_it;
    st[Z_ITERS] = 0.0;
    st[Z_BETA_RE] = st[Z_BETA_IM] = 0.0;
    const int reason = beat_pcg_stop_reason(rr, st[Z_TOL2], tr);
    st[Z_STOP] = reason != 0 ? 1.0 : 0.0;
    st[Z_REASON] = (double)reason;
  } else if (step == 1) {
    st[Z_PQ_RE] = s[0];
    st[Z_PQ_IM] = s[1];
    if (s[0] == 0.0 && s[1] == 0.0) {  // p^T q = 0 with r != 0: the bilinear form broke down
      st[Z_STOP] = 1.0;
      st[Z_REASON] = -5.0;  // KSP_DIVERGED_BREAKDOWN
      return;
    }
    zdiv(st[Z_RZ_RE], st[Z_RZ_IM], s[0], s[1], st[Z_ALPHA_RE], st[Z_ALPHA_IM]);
  } else {
    st[Z_RZN_RE] = s[0];
    st[Z_RZN_IM] = s[1];
    st[Z_RRN] = s[2];
    zdiv(s[0], s[1], st[Z_RZ_RE], st[Z_RZ_IM], st[Z_BETA_RE], st[Z_BETA_IM]);
    st[Z_RZ_RE] = s[0];
    st[Z_RZ_IM] = s[1];
    st[Z_RR] = s[2];
    st[Z_ITERS] += 1.0;
    const double tr = st[Z_RTOL] * st[Z_RTOL] * st[Z_BB];
    if (const int reason = beat_pcg_stop_reason(st[Z_RR], st[Z_TOL2], tr)) {
      st[Z_STOP] = 1.0;
      st[Z_REASON] = (double)reason;
    } else if (st[Z_ITERS] >= st[Z_MAXIT]) {
      st[Z_STOP] = 1.0;
      st[Z_REASON] = -3.0;
    } else if (s[0] == 0.0 && s[1] == 0.0) {
      st[Z_STOP] = 1.0;
      st[Z_REASON] = -5.0;
    }
  }
}

// Right-hand side of a stage: r = sum_m gamma_m w_m - K (sum_j s_j y_j), gamma and s complex, w and y real fields.
struct RkRhsArgs {
  const double* w[BEAT_MAX_STIM];
  double gre[BEAT_MAX_STIM], gim[BEAT_MAX_STIM];
  int nw;
  const double* y[BEAT_MAX_STIM];
  double sre[BEAT_MAX_STIM], sim[BEAT_MAX_STIM];
  int ny;
  double kint[15];
  const double* tk;
};

template <bool CPLX>
__global__ __launch_bounds__(BEAT_BLOCK) void rk_rhs_kernel(Geom g, RkRhsArgs a, double* __restrict__ rre,
                                                            double* __restrict__ rim) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrows = g.ny * g.nz;
  for (int row = blockIdx.x * 4 + wave; row < nrows; row += gridDim.x * 4) {
    const int iz = row / g.ny, iy = row - iz * g.ny;
    const int tyz = 3 * axis_type(iy, g.ny, 1, 1) + 9 * axis_type(iz, g.nz, 1, 1);
    const int64_t base = (int64_t)row * g.nx;
    for (int ix = lane; ix < g.nx; ix += 64) {
      const int type = axis_type(ix, g.nx, 1, 1) + tyz;
      const int64_t i = base + ix;
      double kr = 0.0, ki = 0.0;
      const double* __restrict__ rk = a.tk + type * TABW;
      for (int j = 0; j < a.ny; ++j) {
        double v[15];
        gather15(a.y[j], g, ix, iy, iz, i, v);
        double s = 0.0;
        if (type == 13) {
#pragma unroll
          for (int k = 0; k < 15; ++k) s = fma(a.kint[k], v[k], s);
        } else {
#pragma unroll
          for (int k = 0; k < 15; ++k) s = fma(rk[k], v[k], s);
        }
        kr = fma(a.sre[j], s, kr);
        if (CPLX) ki = fma(a.sim[j], s, ki);
      }
      double gr = 0.0, gi = 0.0;
      for (int m = 0; m < a.nw; ++m) {
        const double wv = a.w[m][i];
        gr = fma(a.gre[m], wv, gr);
        if (CPLX) gi = fma(a.gim[m], wv, gi);
      }
      rre[i] = gr - kr;
      if (CPLX) rim[i] = gi - ki;
    }
  }
}

// v += sum_i Re(d_i u_i) = sum_i (dre_i ure_i - dim_i uim_i)
struct RkUpdArgs {
  const double* ure[BEAT_MAX_STIM];
  const double* uim[BEAT_MAX_STIM];
  double dre[BEAT_MAX_STIM], dim[BEAT_MAX_STIM];
  int nu;
};

__global__ __launch_bounds__(BEAT_BLOCK) void rk_update_kernel(int64_t n, RkUpdArgs a, double* __restrict__ v) {
  for (int64_t i = (int64_t)blockIdx.x * BEAT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BEAT_BLOCK) {
    double s = v[i];
    for (int k = 0; k < a.nu; ++k) {
      s = fma(a.dre[k], a.ure[k][i], s);
      if (a.uim[k] != nullptr) s = fma(-a.dim[k], a.uim[k][i], s);
    }
    v[i] = s;
  }
}

ZOp make_op(const beat_pde* pde, double a, double b, double c) {
  ZOp op{};
  for (int k = 0; k < 15; ++k) {
    const double m = pde->h_mass[13 * 15 + k], s = pde->h_stiff[13 * 15 + k];
    op.re[k] = a * m + b * s;
    op.im[k] = c * s;
  }
  const double xr = op.re[0], xi = op.im[0], den = xr * xr + xi * xi;
  op.dre = den != 0.0 ? xr / den : 0.0;
  op.dim = den != 0.0 ? -xi / den : 0.0;
  op.tm = pde->d_tab(2);
  op.tk = pde->d_tab(3);
  op.a = a;
  op.b = b;
  op.c = c;
  return op;
}

int require_tables(const beat_pde* pde) {
  BEAT_REQUIRE(pde != nullptr, "null pde");
  BEAT_REQUIRE(!pde->var, "the Runge-Kutta stage kernels need constant-coefficient tables (no per-node rows)");
  BEAT_REQUIRE(pde->g.z_lo_phys && pde->g.z_hi_phys, "the Runge-Kutta stage kernels run on an undivided grid only");
  BEAT_REQUIRE(!pde->open.on, "the operator has an open solve: finish it first (beat_pde_solve_end)");
  return BEAT_OK;
}

}  // namespace

extern "C" int64_t beat_pde_zwork_doubles(const beat_pde* pde) {
  if (pde == nullptr) return 0;
  return 6 * (pde->n + 2 * pde->g.plane) + Z_SLOTS;
}

extern "C" int beat_pde_zapply(beat_pde* pde, double a, double b, double c, const double* dev_x_re, const double* dev_x_im,
                               double* dev_y_re, double* dev_y_im) {
  if (int rc = require_tables(pde)) return rc;
  BEAT_REQUIRE(dev_x_re && dev_x_im && dev_y_re && dev_y_im, "null field");
  BEAT_REQUIRE(dev_x_re != dev_y_re && dev_x_im != dev_y_im && dev_x_re != dev_y_im && dev_x_im != dev_y_re,
               "in-place apply is not supported");
  const ZOp op = make_op(pde, a, b, c);
  BEAT_KERNEL(zapply_kernel<true>, dim3(pde->vec_grid), dim3(BEAT_BLOCK), 0, pde->ctx->stream, pde->g, op, (const double*)nullptr,
              dev_x_re, dev_x_im, dev_y_re, dev_y_im, (double*)nullptr);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}

extern "C" int beat_pde_zsolve(beat_pde* pde, double a, double b, double c, const double* dev_rhs_re, const double* dev_rhs_im,
                               double* dev_x_re, double* dev_x_im, double* dev_work, double rtol, double atol, int max_it,
                               beat_ksp_info* info) {
  if (int rc = require_tables(pde)) return rc;
  BEAT_REQUIRE(dev_rhs_re && dev_x_re && dev_work && info, "null argument");
  BEAT_REQUIRE(max_it >= 1, "max_it must be >= 1");
  const bool cplx = dev_x_im != nullptr;
  BEAT_REQUIRE(cplx || (c == 0.0 && dev_rhs_im == nullptr), "a complex shift or right-hand side needs dev_x_im");
  BEAT_REQUIRE(!cplx || dev_rhs_im != nullptr, "dev_x_im given without dev_rhs_im");
  const Geom& g = pde->g;
  const int64_t fld = pde->n + 2 * g.plane;
  double* f[6];
  for (int j = 0; j < 6; ++j) f[j] = dev_work + g.plane + j * fld;
  double *rre = f[0], *rim = f[1], *pre = f[2], *pim = f[3], *qre = f[4], *qim = f[5];
  double* st = dev_work + 6 * fld;
  double* part = pde->ctx->d_partials;
  hipStream_t s = pde->ctx->stream;
  const ZOp op = make_op(pde, a, b, c);
  const dim3 grid(pde->vec_grid), block(BEAT_BLOCK);
  const int count = (int)pde->vec_grid;
  if (cplx) {
    BEAT_KERNEL(zbegin_kernel<true>, grid, block, 0, s, g, op, dev_rhs_re, dev_rhs_im, dev_x_re, dev_x_im, rre, rim, pre, pim, part);
  } else {
    BEAT_KERNEL(zbegin_kernel<false>, grid, block, 0, s, g, op, dev_rhs_re, (const double*)nullptr, dev_x_re, (double*)nullptr, rre,
                (double*)nullptr, pre, (double*)nullptr, part);
  }
  BEAT_KERNEL(zscalar_kernel, dim3(1), block, 0, s, (const double*)part, count, 0, st, rtol, atol, (double)max_it);
  BEAT_LAUNCH_CHECK();
  // iterations are enqueued in chunks; the latch makes the surplus of the last chunk empty launches
  int chunk = pde->z_last_iters > 0 ? pde->z_last_iters + 1 : 16;
  int launched = 0;
  double* h = pde->ctx->h_pinned;
  while (true) {
    const int todo = std::min(chunk, max_it - launched);
    for (int it = 0; it < todo; ++it) {
      if (cplx) {
        BEAT_KERNEL(zapply_kernel<true>, grid, block, 0, s, g, op, (const double*)st, (const double*)pre, (const double*)pim, qre, qim,
                    part);
      } else {
        BEAT_KERNEL(zapply_kernel<false>, grid, block, 0, s, g, op, (const double*)st, (const double*)pre, (const double*)nullptr, qre,
                    (double*)nullptr, part);
      }
      BEAT_KERNEL(zscalar_kernel, dim3(1), block, 0, s, (const double*)part, count, 1, st, rtol, atol, (double)max_it);
      if (cplx) {
        BEAT_KERNEL(zupdate_kernel<true>, grid, block, 0, s, g, op, (const double*)st, dev_x_re, dev_x_im, rre, rim, (const double*)pre,
                    (const double*)pim, (const double*)qre, (const double*)qim, part);
      } else {
        BEAT_KERNEL(zupdate_kernel<false>, grid, block, 0, s, g, op, (const double*)st, dev_x_re, (double*)nullptr, rre, (double*)nullptr,
                    (const double*)pre, (const double*)nullptr, (const double*)qre, (const double*)nullptr, part);
      }
      BEAT_KERNEL(zscalar_kernel, dim3(1), block, 0, s, (const double*)part, count, 2, st, rtol, atol, (double)max_it);
      if (cplx) {
        BEAT_KERNEL(zdirection_kernel<true>, grid, block, 0, s, g, op, (const double*)st, (const double*)rre, (const double*)rim, pre, pim);
      } else {
        BEAT_KERNEL(zdirection_kernel<false>, grid, block, 0, s, g, op, (const double*)st, (const double*)rre, (const double*)nullptr, pre,
                    (double*)nullptr);
      }
      BEAT_LAUNCH_CHECK();
    }
    launched += todo;
    BEAT_HIP_CHECK(hipMemcpyAsync(h, st, sizeof(double) * 16, hipMemcpyDeviceToHost, s));
    BEAT_HIP_CHECK(hipStreamSynchronize(s));
    if (h[Z_STOP] != 0.0 || launched >= max_it) break;
    chunk = std::max(4, chunk / 2);
  }
  info->iterations = (int)h[Z_ITERS];
  info->converged_reason = h[Z_STOP] != 0.0 ? (int)h[Z_REASON] : -3;
  info->residual_norm = std::sqrt(h[Z_RR]);
  info->rhs_norm = std::sqrt(h[Z_BB]);
  pde->z_last_iters = info->iterations;
  return info->converged_reason < 0 ? BEAT_ENOTCONV : BEAT_OK;
}

extern "C" int beat_pde_rk_rhs(beat_pde* pde, const double* const* host_dev_w, const double* host_gamma_re,
                               const double* host_gamma_im, int n_w, const double* const* host_dev_y, const double* host_s_re,
                               const double* host_s_im, int n_y, double* dev_r_re, double* dev_r_im) {
  if (int rc = require_tables(pde)) return rc;
  BEAT_REQUIRE(n_w >= 0 && n_w <= BEAT_MAX_STIM && n_y >= 0 && n_y <= BEAT_MAX_STIM, "at most %d fields of each kind",
               BEAT_MAX_STIM);
  BEAT_REQUIRE(dev_r_re != nullptr, "null output");
  BEAT_REQUIRE((n_w == 0 || (host_dev_w && host_gamma_re)) && (n_y == 0 || (host_dev_y && host_s_re)), "null coefficients");
  const bool cplx = dev_r_im != nullptr;
  RkRhsArgs a{};
  for (int m = 0; m < n_w; ++m) {
    BEAT_REQUIRE(host_dev_w[m] != nullptr, "null weight field %d", m);
    a.w[m] = host_dev_w[m];
    a.gre[m] = host_gamma_re[m];
    a.gim[m] = host_gamma_im ? host_gamma_im[m] : 0.0;
    BEAT_REQUIRE(cplx || a.gim[m] == 0.0, "a complex coefficient needs dev_r_im");
  }
  for (int j = 0; j < n_y; ++j) {
    BEAT_REQUIRE(host_dev_y[j] != nullptr, "null field %d", j);
    a.y[j] = host_dev_y[j];
    a.sre[j] = host_s_re[j];
    a.sim[j] = host_s_im ? host_s_im[j] : 0.0;
    BEAT_REQUIRE(cplx || a.sim[j] == 0.0, "a complex coefficient needs dev_r_im");
  }
  a.nw = n_w;
  a.ny = n_y;
  for (int k = 0; k < 15; ++k) a.kint[k] = pde->h_stiff[13 * 15 + k];
  a.tk = pde->d_tab(3);
  if (cplx) {
    BEAT_KERNEL(rk_rhs_kernel<true>, dim3(pde->vec_grid), dim3(BEAT_BLOCK), 0, pde->ctx->stream, pde->g, a, dev_r_re, dev_r_im);
  } else {
    BEAT_KERNEL(rk_rhs_kernel<false>, dim3(pde->vec_grid), dim3(BEAT_BLOCK), 0, pde->ctx->stream, pde->g, a, dev_r_re, (double*)nullptr);
  }
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}

extern "C" int beat_pde_rk_update(beat_pde* pde, double* dev_v, const double* const* host_dev_u_re, const double* const* host_dev_u_im,
                                  const double* host_d_re, const double* host_d_im, int n_u) {
  if (int rc = require_tables(pde)) return rc;
  BEAT_REQUIRE(dev_v != nullptr && n_u >= 0 && n_u <= BEAT_MAX_STIM, "null field or more than %d stage fields", BEAT_MAX_STIM);
  BEAT_REQUIRE(n_u == 0 || (host_dev_u_re && host_d_re), "null stage fields");
  RkUpdArgs a{};
  for (int k = 0; k < n_u; ++k) {
    BEAT_REQUIRE(host_dev_u_re[k] != nullptr, "null stage field %d", k);
    a.ure[k] = host_dev_u_re[k];
    a.uim[k] = host_dev_u_im ? host_dev_u_im[k] : nullptr;
    a.dre[k] = host_d_re[k];
    a.dim[k] = (host_d_im && a.uim[k]) ? host_d_im[k] : 0.0;
  }
  a.nu = n_u;
  const int64_t n = pde->n;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, (n + BEAT_BLOCK - 1) / BEAT_BLOCK));
  BEAT_KERNEL(rk_update_kernel, dim3(grid), dim3(BEAT_BLOCK), 0, pde->ctx->stream, n, a, dev_v);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}
