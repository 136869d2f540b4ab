// How a slab of nz planes is cut for the passes that overlap a halo exchange.  Plain C++: the host code of every pass family and the
// CPU test (tests/test_slab_parts_cpu.py) read the split from here.
//   part -1: the whole slab in one range
//   part  0: the planes whose stencil needs no ghost plane -- enqueued while the ghost planes travel
//   part  1: the one or two slab-boundary planes, lower first; the pass then sums the block partials of both parts
// A face is "physical" when it is a face of the whole grid (no neighbour, no ghost plane behind it), otherwise live.
#pragma once

namespace beat_pde_detail {

struct PlaneRange {
  int z_lo, z_hi;  // planes [z_lo, z_hi)
};
struct SlabPart {
  int count;  // ranges in use, in launch (= partial-slot) order
  PlaneRange range[2];
};

inline SlabPart beat_slab_part(int nz, bool z_lo_phys, bool z_hi_phys, int part) {
  if (part < 0) return {1, {{0, nz}, {0, 0}}};
  if (part == 0) {
    const int lo = z_lo_phys ? 0 : 1, hi = nz - (z_hi_phys ? 0 : 1);
    return {1, {{lo, hi > lo ? hi : lo}, {0, 0}}};
  }
  SlabPart p{0, {{0, 0}, {0, 0}}};
  if (!z_lo_phys) p.range[p.count++] = {0, 1};
  // (a one-plane slab with two live faces: its plane is the lower boundary plane, launched once)
  if (!z_hi_phys && (nz > 1 || z_lo_phys)) p.range[p.count++] = {nz - 1, nz};
  return p;
}

}  // namespace beat_pde_detail
