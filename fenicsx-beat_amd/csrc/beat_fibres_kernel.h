// The rule-based fibre / sheet / sheet-normal frame of ONE voxel (include/beat_hip.h: beat_fibres_rule has the rule).  Plain C++17
// without a HIP call: the kernel runs it on the device (beat_fibres.hip), tests/fibres_host_harness.cpp on the host against the
// NumPy restatement of the rule (tests/test_fibres_cpu.py).  Built with -ffp-contract=off on both sides.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BEAT_FIBRES_FN __host__ __device__ __forceinline__
#else
#define BEAT_FIBRES_FN inline
#endif

namespace beat_fibres_detail {

// |r| at or below which the transmural direction has no part across the longitudinal one
constexpr double BEAT_FIBRES_RMIN = 1e-12;

// Gradient at the voxel centre of the trilinear field with corner values v (corner c at offsets (c & 1, (c >> 1) & 1, (c >> 2) & 1)):
// per axis the mean of the four edge differences along it, over the spacing
BEAT_FIBRES_FN void beat_fibres_gradient(const double v[8], const double h[3], double g[3]) {
  g[0] = 0.25 * (((v[1] - v[0]) + (v[3] - v[2])) + ((v[5] - v[4]) + (v[7] - v[6]))) / h[0];
  g[1] = 0.25 * (((v[2] - v[0]) + (v[3] - v[1])) + ((v[6] - v[4]) + (v[7] - v[5]))) / h[1];
  g[2] = 0.25 * (((v[4] - v[0]) + (v[5] - v[1])) + ((v[6] - v[2]) + (v[7] - v[3]))) / h[2];
}

BEAT_FIBRES_FN double beat_fibres_norm(const double a[3]) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// s_t delta_ij + (s_l - s_t) f_i f_j, row-major: the (nvoxels, 9) layout beat_pde_assemble_rows reads.  f = 0 gives the isotropic s_t I.
BEAT_FIBRES_FN void beat_fibres_tensor(const double f[3], double s_l, double s_t, double M[9]) {
  const double d = s_l - s_t;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[3 * i + j] = (i == j ? s_t : 0.0) + d * f[i] * f[j];
}

// One voxel.  phi: the transmural field at its 8 corners (0 endocardium, 1 epicardium); psi: the longitudinal field there, or null
// for the constant direction `axis`; angles in radians.  Returns true and f = s = n = 0 for a degenerate voxel: grad phi = 0,
// grad psi = 0 (axis = 0), or the two parallel (|r| <= BEAT_FIBRES_RMIN).  M (null: not wanted) gets the tensor of f either way.
BEAT_FIBRES_FN bool beat_fibres_voxel(const double phi[8], const double* psi, const double h[3], const double* axis, double alpha_endo,
                                      double alpha_epi, double beta_endo, double beta_epi, double f[3], double s[3], double n[3],
                                      double s_l, double s_t, double* M) {
  double gphi[3], el[3];
  beat_fibres_gradient(phi, h, gphi);
  if (psi != nullptr) {
    beat_fibres_gradient(psi, h, el);
  } else {
    for (int k = 0; k < 3; ++k) el[k] = axis[k];
  }
  const double nphi = beat_fibres_norm(gphi), nl = beat_fibres_norm(el);
  bool degenerate = !(nphi > 0.0) || !(nl > 0.0);  // (a NaN in the input counts as degenerate)
  double et[3] = {0.0, 0.0, 0.0}, ec[3];
  if (!degenerate) {
    double t[3];
    for (int k = 0; k < 3; ++k) {
      el[k] /= nl;
      t[k] = gphi[k] / nphi;
    }
    const double lt = el[0] * t[0] + el[1] * t[1] + el[2] * t[2];
    for (int k = 0; k < 3; ++k) et[k] = t[k] - lt * el[k];
    const double nr = beat_fibres_norm(et);
    degenerate = !(nr > BEAT_FIBRES_RMIN);
    if (!degenerate)
      for (int k = 0; k < 3; ++k) et[k] /= nr;
  }
  if (degenerate) {
    for (int k = 0; k < 3; ++k) f[k] = s[k] = n[k] = 0.0;
  } else {
    ec[0] = el[1] * et[2] - el[2] * et[1];
    ec[1] = el[2] * et[0] - el[0] * et[2];
    ec[2] = el[0] * et[1] - el[1] * et[0];
    double pc = 0.125 * (((phi[0] + phi[1]) + (phi[2] + phi[3])) + ((phi[4] + phi[5]) + (phi[6] + phi[7])));
    pc = pc < 0.0 ? 0.0 : (pc > 1.0 ? 1.0 : pc);
    const double alpha = alpha_endo * (1.0 - pc) + alpha_epi * pc;
    const double beta = beta_endo * (1.0 - pc) + beta_epi * pc;
    const double ca = std::cos(alpha), sa = std::sin(alpha), cb = std::cos(beta), sb = std::sin(beta);
    for (int k = 0; k < 3; ++k) {
      const double g = -sa * ec[k] + ca * el[k];
      f[k] = ca * ec[k] + sa * el[k];
      s[k] = sb * g + cb * et[k];
      n[k] = cb * g - sb * et[k];
    }
  }
  if (M != nullptr) beat_fibres_tensor(f, s_l, s_t, M);
  return degenerate;
}

}  // namespace beat_fibres_detail
