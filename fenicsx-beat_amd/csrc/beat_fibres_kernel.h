// The rule-based fibre / sheet / sheet-normal frame of ONE voxel (include/beat_hip.h: beat_fibres_rule has the rule).  Plain C++17
// without a HIP call: the kernel runs it on the device (beat_fibres.hip), tests/fibres_host_harness.cpp on the host against the
// NumPy restatement of the rule (tests/test_fibres_cpu.py).  Built with -ffp-contract=off on both sides.  The second half is the
// bi-ventricular rule (beat_fibres_biv_rule): one frame per surface family, quaternions, Bayer's bislerp, and the voxel; on the host
// through tests/fibres_biv_host_harness.cpp (tests/test_fibres_biv_cpu.py).
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

// ---- the bi-ventricular rule (include/beat_hip.h: beat_fibres_biv_rule has the rule) ----------------------------------------------------
// Quaternions are held in named scalars and every choice below is a select on scalars: nothing is indexed at run time, which would put
// an array into scratch memory on the device.

struct beat_fibres_quat {
  double w, x, y, z;
};

// Step 1.  The frame of the longitudinal direction l and the transmural direction t, turned by alpha and beta (radians): the rule of
// beat_fibres_voxel with its inputs made explicit.  Returns false and leaves f, s, n alone where the frame is undefined: |l| = 0,
// |t| = 0, |r| <= BEAT_FIBRES_RMIN, or a NaN in l or t.
BEAT_FIBRES_FN bool beat_fibres_frame(const double l[3], const double t[3], double alpha, double beta, double f[3], double s[3],
                                      double n[3]) {
  const double nl = beat_fibres_norm(l), nt = beat_fibres_norm(t);
  if (!(nl > 0.0) || !(nt > 0.0)) return false;
  double el[3], tn[3], et[3], ec[3];
  for (int k = 0; k < 3; ++k) {
    el[k] = l[k] / nl;
    tn[k] = t[k] / nt;
  }
  const double lt = el[0] * tn[0] + el[1] * tn[1] + el[2] * tn[2];
  for (int k = 0; k < 3; ++k) et[k] = tn[k] - lt * el[k];
  const double nr = beat_fibres_norm(et);
  if (!(nr > BEAT_FIBRES_RMIN)) return false;
  for (int k = 0; k < 3; ++k) et[k] /= nr;
  ec[0] = el[1] * et[2] - el[2] * et[1];
  ec[1] = el[2] * et[0] - el[0] * et[2];
  ec[2] = el[0] * et[1] - el[1] * et[0];
  const double ca = std::cos(alpha), sa = std::sin(alpha), cb = std::cos(beta), sb = std::sin(beta);
  for (int k = 0; k < 3; ++k) {
    const double g = -sa * ec[k] + ca * el[k];
    f[k] = ca * ec[k] + sa * el[k];
    s[k] = sb * g + cb * et[k];
    n[k] = cb * g - sb * et[k];
  }
  return true;
}

// Step 2.  The rotation R = [f | n | s] (columns) as a unit quaternion, by Shepperd's method: the largest of the trace and the three
// diagonal entries decides which component comes from the square root, so the divisor is at least 2.
BEAT_FIBRES_FN beat_fibres_quat beat_fibres_frame_to_quat(const double f[3], const double s[3], const double n[3]) {
  const double r00 = f[0], r10 = f[1], r20 = f[2], r01 = n[0], r11 = n[1], r21 = n[2], r02 = s[0], r12 = s[1], r22 = s[2];
  const double tr = r00 + r11 + r22;
  beat_fibres_quat q;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    const double S = 2.0 * std::sqrt(1.0 + tr);
    q.w = 0.25 * S;
    q.x = (r21 - r12) / S;
    q.y = (r02 - r20) / S;
    q.z = (r10 - r01) / S;
  } else if (r00 >= r11 && r00 >= r22) {
    const double S = 2.0 * std::sqrt(1.0 + r00 - r11 - r22);
    q.w = (r21 - r12) / S;
    q.x = 0.25 * S;
    q.y = (r01 + r10) / S;
    q.z = (r02 + r20) / S;
  } else if (r11 >= r22) {
    const double S = 2.0 * std::sqrt(1.0 + r11 - r00 - r22);
    q.w = (r02 - r20) / S;
    q.x = (r01 + r10) / S;
    q.y = 0.25 * S;
    q.z = (r12 + r21) / S;
  } else {
    const double S = 2.0 * std::sqrt(1.0 + r22 - r00 - r11);
    q.w = (r10 - r01) / S;
    q.x = (r02 + r20) / S;
    q.y = (r12 + r21) / S;
    q.z = 0.25 * S;
  }
  return q;
}

// ... and back; the quaternion is normalised first.
BEAT_FIBRES_FN void beat_fibres_quat_to_frame(beat_fibres_quat q, double f[3], double s[3], double n[3]) {
  const double nq = std::sqrt((q.w * q.w + q.x * q.x) + (q.y * q.y + q.z * q.z));
  const double w = q.w / nq, x = q.x / nq, y = q.y / nq, z = q.z / nq;
  f[0] = 1.0 - 2.0 * (y * y + z * z);
  f[1] = 2.0 * (x * y + w * z);
  f[2] = 2.0 * (x * z - w * y);
  n[0] = 2.0 * (x * y - w * z);
  n[1] = 1.0 - 2.0 * (x * x + z * z);
  n[2] = 2.0 * (y * z + w * x);
  s[0] = 2.0 * (x * z + w * y);
  s[1] = 2.0 * (y * z - w * x);
  s[2] = 1.0 - 2.0 * (x * x + y * y);
}

// Step 3.  Of a, a i, a j, a k -- the frames (f, n, s), (f, -n, -s), (-f, n, -s), (-f, -n, s) of a -- the one nearest to b or to -b
// (the earliest wins a tie), with the sign that brings it to b's side, turned towards b by the share t of the angle between them.
// c >= 1/2 (the four are an orthonormal basis of R^4), so there is no acos and no division by a sine: w / sigma is a unit vector
// whatever sigma > 0 is, and it is multiplied by sin(t theta) <= sigma.
BEAT_FIBRES_FN beat_fibres_quat beat_fibres_bislerp(beat_fibres_quat a, beat_fibres_quat b, double t) {
  const double c0 = (a.w * b.w + a.x * b.x) + (a.y * b.y + a.z * b.z);   // a   = ( w,  x,  y,  z)
  const double c1 = (-a.x * b.w + a.w * b.x) + (a.z * b.y - a.y * b.z);  // a i = (-x,  w,  z, -y)
  const double c2 = (-a.y * b.w - a.z * b.x) + (a.w * b.y + a.x * b.z);  // a j = (-y, -z,  w,  x)
  const double c3 = (-a.z * b.w + a.y * b.x) + (-a.x * b.y + a.w * b.z); // a k = (-z,  y, -x,  w)
  beat_fibres_quat q = a;
  double c = c0;
  if (std::fabs(c1) > std::fabs(c)) {
    c = c1;
    q.w = -a.x, q.x = a.w, q.y = a.z, q.z = -a.y;
  }
  if (std::fabs(c2) > std::fabs(c)) {
    c = c2;
    q.w = -a.y, q.x = -a.z, q.y = a.w, q.z = a.x;
  }
  if (std::fabs(c3) > std::fabs(c)) {
    c = c3;
    q.w = -a.z, q.x = a.y, q.y = -a.x, q.z = a.w;
  }
  if (c < 0.0) {
    c = -c;
    q.w = -q.w, q.x = -q.x, q.y = -q.y, q.z = -q.z;
  }
  const double ww = b.w - c * q.w, wx = b.x - c * q.x, wy = b.y - c * q.y, wz = b.z - c * q.z;
  const double sigma = std::sqrt((ww * ww + wx * wx) + (wy * wy + wz * wz));
  if (sigma > 0.0) {
    const double angle = t * std::atan2(sigma, c);
    const double ct = std::cos(angle), st = std::sin(angle) / sigma;
    q.w = ct * q.w + st * ww;
    q.x = ct * q.x + st * wx;
    q.y = ct * q.y + st * wy;
    q.z = ct * q.z + st * wz;
  }
  return q;
}

// The mean of the 8 corner values, clipped to [0, 1]
BEAT_FIBRES_FN double beat_fibres_centre(const double v[8]) {
  const double c = 0.125 * (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
  return c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
}

// Step 4.  One voxel of two ventricles.  phi_lv, phi_rv, phi_epi: the three transmural fields at its 8 corners (each 1 on its own
// surface, 0 on the other two); psi, axis, the angles, M and the result as for beat_fibres_voxel.  Degenerate (true, f = s = n = 0)
// where none of the three frames is defined.
BEAT_FIBRES_FN bool beat_fibres_biv_voxel(const double phi_lv[8], const double phi_rv[8], const double phi_epi[8], const double* psi,
                                          const double h[3], const double* axis, double alpha_endo, double alpha_epi, double beta_endo,
                                          double beta_epi, double f[3], double s[3], double n[3], double s_l, double s_t, double* M) {
  double l[3], mglv[3], grv[3], gepi[3];
  if (psi != nullptr) {
    beat_fibres_gradient(psi, h, l);
  } else {
    for (int k = 0; k < 3; ++k) l[k] = axis[k];
  }
  beat_fibres_gradient(phi_lv, h, mglv);
  for (int k = 0; k < 3; ++k) mglv[k] = -mglv[k];
  beat_fibres_gradient(phi_rv, h, grv);
  beat_fibres_gradient(phi_epi, h, gepi);
  const double clv = beat_fibres_centre(phi_lv), crv = beat_fibres_centre(phi_rv), cepi = beat_fibres_centre(phi_epi);
  const double d = (clv + crv > 0.0) ? crv / (clv + crv) : 0.0;
  const double alpha_s = alpha_endo * (1.0 - 2.0 * d), beta_s = beta_endo * (1.0 - 2.0 * d);
  const double alpha_w = alpha_endo * (1.0 - cepi) + alpha_epi * cepi, beta_w = beta_endo * (1.0 - cepi) + beta_epi * cepi;

  beat_fibres_quat q = {1.0, 0.0, 0.0, 0.0};
  double ff[3], fs[3], fn[3];  // one frame at a time
  bool defined = beat_fibres_frame(l, mglv, alpha_s, beta_s, ff, fs, fn);
  if (defined) q = beat_fibres_frame_to_quat(ff, fs, fn);
  if (beat_fibres_frame(l, grv, alpha_s, beta_s, ff, fs, fn)) {
    const beat_fibres_quat qrv = beat_fibres_frame_to_quat(ff, fs, fn);
    q = defined ? beat_fibres_bislerp(q, qrv, d) : qrv;
    defined = true;
  }
  if (beat_fibres_frame(l, gepi, alpha_w, beta_w, ff, fs, fn)) {
    const beat_fibres_quat qepi = beat_fibres_frame_to_quat(ff, fs, fn);
    q = defined ? beat_fibres_bislerp(q, qepi, cepi) : qepi;
    defined = true;
  }
  // (q is the identity where nothing is defined; selects, not a branch that stores zeros: the compiler merges equal stores of two
  // branches into one store through a chosen address, and what is stored through such an address stays in scratch memory)
  beat_fibres_quat_to_frame(q, ff, fs, fn);
  for (int k = 0; k < 3; ++k) {
    f[k] = defined ? ff[k] : 0.0;
    s[k] = defined ? fs[k] : 0.0;
    n[k] = defined ? fn[k] : 0.0;
  }
  if (M != nullptr) beat_fibres_tensor(f, s_l, s_t, M);
  return !defined;
}

}  // namespace beat_fibres_detail
