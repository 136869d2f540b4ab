// Host build of the ionic kernels' math layer (fenicsx-beat_amd/csrc/beat_math_probe.h -> ionic_models.h, torord_dyncl.h) for
// tests/test_device_math_host.py and the host / device comparison of tests/test_device_math_gpu.py: the same source the device
// probe (beat_math_probe) compiles, with the device intrinsics replaced as tests/tp06_host_harness.cpp replaces them (the
// reciprocal and rsqrt estimates become 1/x and 1/sqrt(x): the rcp rows are not comparable).
//   math_host <fn> <in.bin> <out.bin> n     (in: (BEAT_MATH_IN[fn], n) doubles row-major, out: (BEAT_MATH_OUT[fn], n))
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime.h>  // (host side of the HIP headers: g++ sees __device__ / __forceinline__ as plain inline)

template <class T>
static inline T __shfl_down(T v, int, int) { return v; }
static inline void __syncthreads() {}
struct Dim3Stub { unsigned x = 0, y = 0, z = 0; };
static Dim3Stub threadIdx, blockIdx, blockDim, gridDim;
static inline int __double2hiint(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return (int)(uint32_t)(b >> 32);
}
static inline int __double2loint(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return (int)(uint32_t)(b & 0xffffffffu);
}
static inline double __hiloint2double(int hi, int lo) {
  const uint64_t b = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double x;
  std::memcpy(&x, &b, 8);
  return x;
}
static inline double __builtin_amdgcn_rcp(double x) { return 1.0 / x; }
static inline double __builtin_amdgcn_rsq(double x) { return 1.0 / std::sqrt(x); }
static inline void __builtin_amdgcn_sched_barrier(int) {}
#include "../fenicsx-beat_amd/csrc/beat_math_probe.h"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int fn = std::atoi(argv[1]);
  const long n = std::atol(argv[4]);
  if (fn < 0 || fn >= BEAT_MATH_COUNT || n <= 0) return 2;
  const int k = BEAT_MATH_IN[fn], m = BEAT_MATH_OUT[fn];
  std::vector<double> in((size_t)k * n), out((size_t)m * n);
  FILE* f = std::fopen(argv[2], "rb");
  if (!f || std::fread(in.data(), 8, in.size(), f) != in.size()) return 3;
  std::fclose(f);
  const FastMath fm{kExp2Tab, kLogTab};  // (on the host both flavours scale by ldexp and read the plain table)
  const FastMathT<true> fmi{kExp2Tab, kLogTab};
  for (long i = 0; i < n; ++i) {
    double a[4], o[4];
    for (int r = 0; r < k; ++r) a[r] = in[(size_t)r * n + i];
    beat_math_eval(fn, fm, fmi, a, o);
    for (int r = 0; r < m; ++r) out[(size_t)r * n + i] = o[r];
  }
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 4;
  std::fclose(f);
  return 0;
}
