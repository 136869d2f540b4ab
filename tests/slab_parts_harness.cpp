// Prints what csrc/beat_slab_parts.h yields, one line per (nz, z_lo_phys, z_hi_phys, part):  nz lo hi part count z_lo z_hi [z_lo z_hi]
// (tests/test_slab_parts_cpu.py)
#include <cstdio>

#include "beat_slab_parts.h"

int main() {
  for (int nz = 1; nz <= 5; ++nz)
    for (int lo = 0; lo < 2; ++lo)
      for (int hi = 0; hi < 2; ++hi)
        for (int part = -1; part <= 1; ++part) {
          const beat_pde_detail::SlabPart p = beat_pde_detail::beat_slab_part(nz, lo != 0, hi != 0, part);
          std::printf("%d %d %d %d %d", nz, lo, hi, part, p.count);
          for (int k = 0; k < p.count; ++k) std::printf(" %d %d", p.range[k].z_lo, p.range[k].z_hi);
          std::printf("\n");
        }
  return 0;
}
