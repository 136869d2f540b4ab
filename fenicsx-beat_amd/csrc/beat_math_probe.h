// The ionic kernels' math layer one helper at a time: beat_math_probe (beat_probe.hip) evaluates these on the device, and
// tests/math_host_harness.cpp builds the same function for the host with g++ -- the CPU suite holds the exp / log / phi sources,
// the GPU suite the device's results (and that both are the same bits).  Each entry reads BEAT_MATH_IN[fn] values of one column
// and writes BEAT_MATH_OUT[fn]; the composites take (y, f or inf, J or rate, dt).
#pragma once

#include "ionic_models.h"
#include "torord_dyncl.h"

enum BeatMathFn {
  BEAT_MATH_EXP = 0,       // FastMath::exp (v_ldexp_f64 scaling: ToR-ORd, TP06, the generated models)
  BEAT_MATH_EXP_INT,       // FastMathT<true>::exp (integer add into the exponent field; no model uses it)
  BEAT_MATH_LOG,           // FastMath::log
  BEAT_MATH_LOG_INT,       // FastMathT<true>::log
  BEAT_MATH_RCP,           // beat_rcp
  BEAT_MATH_RSQRT,         // beat_rsqrt
  BEAT_MATH_TP06_RCP2,     // Tp06Grl1::rcp2 / 3 / 4: (a, b[, c[, d]]) -> their reciprocals
  BEAT_MATH_TP06_RCP3,
  BEAT_MATH_TP06_RCP4,
  BEAT_MATH_TORORD_RCP2,   // torord_detail::rcp2 / 3 / 4
  BEAT_MATH_TORORD_RCP3,
  BEAT_MATH_TORORD_RCP4,
  BEAT_MATH_TP06_PHI_SMALL,
  BEAT_MATH_TP06_PHI7,
  BEAT_MATH_TORORD_PHI_SMALL,
  BEAT_MATH_TORORD_PHI7,
  BEAT_MATH_TP06_GRL1,     // Tp06Grl1::grl1 (y, f, J, dt)
  BEAT_MATH_TP06_ADVANCE,  // Tp06Grl1::advance (y, f, J, dt)
  BEAT_MATH_TP06_GATE,     // Tp06Grl1::gate (y, inf, 1/tau, dt)
  BEAT_MATH_TORORD_ADVANCE,  // TorordDynClGrl1::advance (y, f, J, dt)
  BEAT_MATH_TORORD_GATE,     // TorordDynClGrl1::gate (y, inf, rate, dt)
  BEAT_MATH_TORORD_GATE_B,   // TorordDynClGrl1::gate_b (y, inf, rate, dt, small = true)
  BEAT_MATH_COUNT
};
constexpr int BEAT_MATH_IN[BEAT_MATH_COUNT] = {1, 1, 1, 1, 1, 1, 2, 3, 4, 2, 3, 4, 1, 1, 1, 1, 4, 4, 4, 4, 4, 4};
constexpr int BEAT_MATH_OUT[BEAT_MATH_COUNT] = {1, 1, 1, 1, 1, 1, 2, 3, 4, 2, 3, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

// fm: the flavour TP06 and ToR-ORd use (FastMath), fmi: FastMathT<true>
template <class FM, class FMI>
__device__ __forceinline__ void beat_math_eval(int fn, const FM& fm, const FMI& fmi, const double* a, double* o) {
  using T = Tp06Grl1;
  using R = TorordDynClGrl1;
  static_assert(std::is_same<typename T::FM, FM>::value, "TP06 takes the flavour the probe stages as fm");
  switch (fn) {
    case BEAT_MATH_EXP: o[0] = fm.exp(a[0]); break;
    case BEAT_MATH_EXP_INT: o[0] = fmi.exp(a[0]); break;
    case BEAT_MATH_LOG: o[0] = fm.log(a[0]); break;
    case BEAT_MATH_LOG_INT: o[0] = fmi.log(a[0]); break;
    case BEAT_MATH_RCP: o[0] = beat_rcp(a[0]); break;
    case BEAT_MATH_RSQRT: o[0] = beat_rsqrt(a[0]); break;
    case BEAT_MATH_TP06_RCP2: T::rcp2(a[0], a[1], o[0], o[1]); break;
    case BEAT_MATH_TP06_RCP3: T::rcp3(a[0], a[1], a[2], o[0], o[1], o[2]); break;
    case BEAT_MATH_TP06_RCP4: T::rcp4(a[0], a[1], a[2], a[3], o[0], o[1], o[2], o[3]); break;
    case BEAT_MATH_TORORD_RCP2: torord_detail::rcp2(a[0], a[1], o[0], o[1]); break;
    case BEAT_MATH_TORORD_RCP3: torord_detail::rcp3(a[0], a[1], a[2], o[0], o[1], o[2]); break;
    case BEAT_MATH_TORORD_RCP4: torord_detail::rcp4(a[0], a[1], a[2], a[3], o[0], o[1], o[2], o[3]); break;
    case BEAT_MATH_TP06_PHI_SMALL: o[0] = T::phi_small(a[0]); break;
    case BEAT_MATH_TP06_PHI7: o[0] = T::phi7(a[0]); break;
    case BEAT_MATH_TORORD_PHI_SMALL: o[0] = R::phi_small(a[0]); break;
    case BEAT_MATH_TORORD_PHI7: o[0] = R::phi7(a[0]); break;
    case BEAT_MATH_TP06_GRL1: o[0] = T::grl1(fm, a[0], a[1], a[2], a[3]); break;
    case BEAT_MATH_TP06_ADVANCE: o[0] = T::advance(fm, a[0], a[1], a[2], a[3]); break;
    case BEAT_MATH_TP06_GATE: o[0] = T::gate(fm, a[0], a[1], a[2], a[3]); break;
    case BEAT_MATH_TORORD_ADVANCE: o[0] = R::advance(fm, a[0], a[1], a[2], a[3]); break;
    case BEAT_MATH_TORORD_GATE: o[0] = R::gate(fm, a[0], a[1], a[2], a[3]); break;
    case BEAT_MATH_TORORD_GATE_B: o[0] = R::gate_b(fm, a[0], a[1], a[2], a[3], true); break;
  }
}
