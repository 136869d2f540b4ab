// Small device helpers the diffusion kernels share: the node type along an axis, the XCD block mapping, the DPP lane shifts and the
// raw-buffer 64-bit load.  Device code only (gfx950 builtins); each kernel file includes it beside beat_pde_internal.h.
#pragma once

namespace beat_pde_detail {

// node type along an axis of n nodes: 0 low face, 1 interior, 2 high face; lo_phys / hi_phys: that end is a face of the whole grid
__device__ __forceinline__ int axis_type(int i, int n, int lo_phys, int hi_phys) {
  if (n == 1 && lo_phys && hi_phys) return 1;  // collapsed axis: no coupling along it
  if (i == 0 && lo_phys) return 0;
  if (i == n - 1 && hi_phys) return 2;
  return 1;
}

// Blocks are dealt round-robin to the 8 XCDs; give each XCD a contiguous run of tiles so that
// tiles sharing a halo share an L2.  Pure performance heuristic (placement is not relied upon).
__device__ __forceinline__ int xcd_block(int b, int total) {
  const int per = (total + 7) >> 3;
  return (b & 7) * per + (b >> 3);
}

// lane i <- lane i-1 (lane 0 <- 0) / lane i <- lane i+1 (lane 63 <- 0); all 64 lanes must be active
__device__ __forceinline__ double from_left(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, true);  // wave_shr:1
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double from_right(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true);  // wave_shl:1
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// One plane of a field (or of a coefficient row) as a raw buffer of `bytes` bytes: a lane that wants nothing passes BUF_OOB, an offset
// beyond the buffer's end -- its load returns 0 and fetches nothing -- so it needs neither a branch nor a change of the exec mask.
// AUX: the cache-policy operand of the load (0 default, 2 non-temporal).
typedef int buf_v2i __attribute__((ext_vector_type(2)));
constexpr unsigned BUF_OOB = 0x80000000u;
template <int AUX = 0>
__device__ __forceinline__ double buf_load(const double* base, unsigned bytes, unsigned off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
  const buf_v2i v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, AUX);
  return __hiloint2double(v.y, v.x);
}

}  // namespace beat_pde_detail
