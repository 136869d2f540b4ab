// How an instance compiled at run time is held against a reference instance (beat_ode_jit.h: a sparse-row instance against the
// run-time-index kernel; beat_ode_jit.hip: a variant step or monitor instance of a generated model against its plain instance):
// the switch that turns the checks off and the comparison of the two results, row by row.  No HIP: the library and the CPU test
// (tests/test_jit_check_cpu.py, g++) read it from here.  Tolerances and message texts are the callers'.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdlib>

// BEAT_JIT_SELF_CHECK=0 (set, first character '0') turns every check of a run-time compiled instance off
inline bool beat_jit_checks_off() {
  const char* e = std::getenv("BEAT_JIT_SELF_CHECK");
  return e != nullptr && e[0] == '0';
}

struct BeatJitMismatch {
  size_t row = 0, node = 0;
  double x = 0.0, y = 0.0;  // the instance's value, the reference's
};

// a (the instance under test) against b (the reference), both rows x nc and row-major: |x - y| <= rtol |y| + atol S, S the
// largest finite |b| below 1e300 of the value's row.  true when every pair agrees; else *bad is the first one, in row-major order,
// that does not.
inline bool beat_jit_rows_agree(const double* a, const double* b, size_t rows, size_t nc, double rtol, double atol, BeatJitMismatch* bad) {
  for (size_t k = 0; k < rows; ++k) {
    double scale = 0.0;
    for (size_t i = 0; i < nc; ++i) {
      const double v = std::fabs(b[k * nc + i]);
      if (v == v && v > scale && v < 1e300) scale = v;
    }
    for (size_t i = 0; i < nc; ++i) {
      const double x = a[k * nc + i], y = b[k * nc + i];
      if (x != x && y != y) continue;  // both NaN (a caller's garbage in, the same garbage out)
      if (!(std::fabs(x - y) <= rtol * std::fabs(y) + atol * scale)) {  // (written so that NaN against a number fails)
        *bad = BeatJitMismatch{k, i, x, y};
        return false;
      }
    }
  }
  return true;
}
