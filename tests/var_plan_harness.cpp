// Prints the work plans of csrc/beat_var_plan.h (tests/_var_plan.py, tests/test_var_plan_cpu.py).  Commands on stdin, one per line; every
// answer ends with a line "end".  Integers in decimal, flag and mask words in hex.
//   case nx ny nz z_lo_phys z_hi_phys nwords w ...   the grid, its faces and the tissue bits every later command works on
//   seg T                 -> seg n i ... | segmask n w ... | tiled n i ... | tiledmask n w ...   (T = 0: the tiled lists are empty)
//   vtl ry max_run aligned max_items want_mask
//                         -> vtl declined   or   vtl nsegx nzp run | lists base count (x 3) | first (27) | items n seg rb zb ze ... |
//                            mask n hash [| maskwords w ...]
//   vrr ry max_run        -> vrr first count (x 3) | items n seg rb zb ze ...
//   parts                 -> part0 n z_lo z_hi ... | part1 n z_lo z_hi ...   (beat_slab_part: the planes of the second and third list)
//   sizes nx ny nz        -> sizes 0|1   (vtl_sizes_declined)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "beat_var_plan.h"

using namespace beat_pde_detail;

static void print_ints(const char* name, const std::vector<int>& v) {
  std::printf("%s %zu", name, v.size());
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}
static void print_words(const char* name, const std::vector<u64>& v) {
  std::printf("%s %zu", name, v.size());
  for (u64 x : v) std::printf(" %llx", x);
  std::printf("\n");
}
static void print_items(const std::vector<PlaneRun>& v) {
  std::printf("items %zu", v.size());
  for (const PlaneRun& r : v) std::printf(" %d %d %d %d", r.seg, r.rb, r.zb, r.ze);
  std::printf("\n");
}
static u64 fnv(const std::vector<u64>& v) {
  u64 h = 1469598103934665603ull;
  for (u64 x : v)
    for (int b = 0; b < 8; ++b) h = (h ^ ((x >> (8 * b)) & 255ull)) * 1099511628211ull;
  return h;
}

int main() {
  int nx = 0, ny = 0, nz = 0, lo = 1, hi = 1;
  std::vector<u64> flags;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "case") {
      size_t nwords = 0;
      in >> nx >> ny >> nz >> lo >> hi >> nwords;
      flags.assign(nwords, 0ull);
      for (u64& w : flags) in >> std::hex >> w;
      if (!in || nwords != (size_t)(((int64_t)nx * ny * nz + VAR_SEG - 1) / VAR_SEG)) return 2;
      continue;  // (no answer)
    } else if (cmd == "seg") {
      int T = 0;
      in >> T;
      const SegList s = var_segments(flags);
      const SegList t = T > 0 ? var_segments_tiled(s, nx, ny, (int64_t)nx * ny, T) : SegList{};
      print_ints("seg", s.seg);
      print_words("segmask", s.mask);
      print_ints("tiled", t.seg);
      print_words("tiledmask", t.mask);
    } else if (cmd == "vtl") {
      VtlPlanOptions o;
      int want_mask = 0;
      in >> o.ry >> o.max_run >> o.aligned >> o.max_items >> want_mask;
      if (!in) return 2;
      const VtlPlan p = vtl_plan(nx, ny, nz, lo != 0, hi != 0, flags, o);
      if (p.declined) {
        std::printf("vtl declined\n");
      } else {
        std::printf("vtl %d %d %d\n", p.nsegx, p.nzp, p.run);
        std::printf("lists");
        for (int k = 0; k < 3; ++k) std::printf(" %d %d", p.list_base[k], p.list_count[k]);
        std::printf("\nfirst");
        for (int k = 0; k < 3; ++k)
          for (int x = 0; x < 9; ++x) std::printf(" %d", p.first[k][x]);
        std::printf("\n");
        print_items(p.items);
        std::printf("mask %zu %llx\n", p.mask.size(), fnv(p.mask));
        if (want_mask) print_words("maskwords", p.mask);
      }
    } else if (cmd == "vrr") {
      VrrPlanOptions o;
      in >> o.ry >> o.max_run;
      if (!in) return 2;
      const VrrPlan p = vrr_plan(nx, ny, nz, lo != 0, hi != 0, flags, o);
      std::printf("vrr");
      for (int k = 0; k < 3; ++k) std::printf(" %d %d", p.first[k], p.count[k]);
      std::printf("\n");
      print_items(p.items);
    } else if (cmd == "parts") {
      for (int part = 0; part < 2; ++part) {
        const SlabPart sp = beat_slab_part(nz, lo != 0, hi != 0, part);
        std::printf("part%d %d", part, 2 * sp.count);
        for (int k = 0; k < sp.count; ++k) std::printf(" %d %d", sp.range[k].z_lo, sp.range[k].z_hi);
        std::printf("\n");
      }
    } else if (cmd == "sizes") {
      int sx = 0, sy = 0, sz = 0;
      in >> sx >> sy >> sz;
      if (!in) return 2;
      std::printf("sizes %d\n", vtl_sizes_declined(sx, sy, sz) ? 1 : 0);
    } else {
      return 2;
    }
    std::printf("end\n");
  }
  return 0;
}
