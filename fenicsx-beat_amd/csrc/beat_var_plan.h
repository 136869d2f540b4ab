// The host-built work plans of the per-node-coefficient diffusion path, all derived from one array of tissue bits (bit l of flags[s]:
// node 64 s + l is a tissue node; nodes numbered x fastest, then y, then z):
//   * the list of the 64-node segments that hold tissue and its tile-ordered copy (var_spmv_kernel and the vector kernels,
//     beat_pde_var.hip);
//   * the lane masks, the three tile lists and their eight parts of vtl_spmv_kernel (beat_pde_vtl.hip);
//   * the three lists of column runs of the opt-in vrr_spmv_kernel (beat_pde_vrr.hip).
// Plain C++: integer geometry only, no device calls, no switches, no I/O.  The set-up functions read their switches, call a planner
// and upload what it returns; tests/var_plan_harness.cpp prints the plans and tests/test_var_plan_cpu.py holds them to the tissue
// bits.  A face is physical or live as in beat_slab_parts.h, which also cuts the slab for the second and third list.
#pragma once
#include "beat_slab_parts.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace beat_pde_detail {

using u64 = unsigned long long;

constexpr int SEG = 62;      // x-nodes computed per wave and row by the tile and the column kernels (lanes 1..62; 0 and 63: the x-halo)
constexpr int VAR_SEG = 64;  // granularity of the tissue bookkeeping: one wavefront's worth of consecutive nodes
constexpr int MAX_RUN = 48;  // planes per column run of vrr_spmv_kernel at most, by default (longer runs of tissue are cut)

// A column (x segment, row block) of the wave decomposition and the planes [zb, ze) of it that one work item computes: a tile of
// vtl_spmv_kernel (RY rows, one per wave) or a run of vrr_spmv_kernel (RY rows per wave)
struct PlaneRun {
  int seg, rb, zb, ze;
};

// the tissue bits of the nodes [i, i + n), 1 <= n <= 64, in bits 0 .. n-1
inline u64 tissue_bits(const std::vector<u64>& flags, int64_t i, int n) {
  const size_t w = (size_t)(i >> 6);
  const int off = (int)(i & 63);
  u64 v = flags[w] >> off;
  if (off + n > 64) v |= flags[w + 1] << (64 - off);
  return n < 64 ? v & ((1ull << n) - 1ull) : v;
}

// ---- the segment list -------------------------------------------------------------------------------------------------------------
struct SegList {
  std::vector<int> seg;   // indices of the 64-node segments that hold tissue nodes
  std::vector<u64> mask;  // per entry: bit l set = node 64 seg + l is a tissue node
};

// the segments that hold tissue, ascending
inline SegList var_segments(const std::vector<u64>& flags) {
  SegList s;
  for (size_t k = 0; k < flags.size(); ++k)
    if (flags[k]) {
      s.seg.push_back((int)k);
      s.mask.push_back(flags[k]);
    }
  return s;
}

// the same list in tile order: tiles of T rows x T planes (keyed by the segment's first node), node order inside
inline SegList var_segments_tiled(const SegList& s, int nx, int ny, int64_t plane, int T) {
  const int64_t nyb = (ny + T - 1) / T;
  std::vector<int64_t> key(s.seg.size());
  std::vector<int> order(s.seg.size());
  for (size_t k = 0; k < s.seg.size(); ++k) {
    const int64_t i0 = (int64_t)s.seg[k] * VAR_SEG;
    const int64_t z = i0 / plane, y = (i0 % plane) / nx;
    key[k] = (z / T) * nyb + y / T;
    order[k] = (int)k;
  }
  std::stable_sort(order.begin(), order.end(), [&](int u, int v) { return key[(size_t)u] < key[(size_t)v]; });
  SegList t;
  t.seg.resize(order.size());
  t.mask.resize(order.size());
  for (size_t k = 0; k < order.size(); ++k) {
    t.seg[k] = s.seg[(size_t)order[k]];
    t.mask[k] = s.mask[(size_t)order[k]];
  }
  return t;
}

// ---- columns: which planes hold tissue, and the runs of planes over them ----------------------------------------------------------
struct PlanGrid {
  int nx, ny, nz;
  int64_t plane() const { return (int64_t)nx * ny; }
  int nsegx() const { return (nx + SEG - 1) / SEG; }
};

// act[z] = column (seg, rb) of ry rows holds a tissue node on plane z, for z in [z_lo, z_hi); returns whether any plane does.  One
// definition serves both kernels: the x-nodes 62 seg .. 62 seg + 61 inside the box are the lanes 1..62 of the tile kernel's masks.
inline bool column_activity(const PlanGrid& g, const std::vector<u64>& flags, int seg, int rb, int ry, int z_lo, int z_hi,
                            std::vector<char>& act) {
  const int x0 = seg * SEG, x1 = std::min(g.nx, x0 + SEG), ya = rb * ry, yb = std::min(g.ny, ya + ry);
  bool any = false;
  for (int z = z_lo; z < z_hi; ++z) {
    u64 m = 0ull;
    for (int y = ya; y < yb; ++y) m |= tissue_bits(flags, (int64_t)z * g.plane() + (int64_t)y * g.nx + x0, x1 - x0);
    act[(size_t)z] = m != 0ull;
    any |= m != 0ull;
  }
  return any;
}

// The runs of column (seg, rb) over the planes [z_lo, z_hi): a run starts on a plane with tissue, grows over gaps of up to two planes
// and ends behind its last plane with tissue, before limit(its first plane) at the latest
template <class Limit>
void grow_runs(const std::vector<char>& act, int seg, int rb, int z_lo, int z_hi, Limit limit, std::vector<PlaneRun>& out) {
  int z = z_lo;
  while (z < z_hi) {
    if (!act[(size_t)z]) {
      ++z;
      continue;
    }
    const int stop = (int)std::min<int64_t>(z_hi, limit(z));
    int e = z + 1, last = z + 1;
    while (e < stop && (act[(size_t)e] || e - last < 2)) {
      if (act[(size_t)e]) last = e + 1;
      ++e;
    }
    out.push_back(PlaneRun{seg, rb, z, last});
    z = last;
  }
}

// ---- the tile plan of vtl_spmv_kernel ---------------------------------------------------------------------------------------------
struct VtlPlanOptions {
  int ry = 8;         // rows per tile: 4 or 8
  int max_run = 16;   // planes per tile at most; doubled until the tiles fit max_items
  int aligned = 0;    // 0: tiles trimmed to their own tissue | 1: to the tissue range of their z block | 2: whole z blocks
  int max_items = 0;  // tiles per list at most (one partial sum per tile: the library passes its number of partial slots)
};

struct VtlPlan {
  bool declined = true;  // the segment-list kernels serve the operator; nothing below is filled
  int nsegx = 0;         // x segments per row
  int nzp = 0;           // entries per (row, x segment) of the mask table: planes -1 .. nz, and what the march reads ahead
  int run = 0;           // the run finally used
  // mask[(y + 1) nsegx + seg][z + 1]: bit l = node (62 seg - 1 + l, y, z) is a tissue node of this slab; on a ghost plane that another
  // rank owns: the node is inside the box (its p is live; which of them are tissue is not known here).  Rows -1 and ny: all zero
  std::vector<u64> mask;
  // tile lists, back to back: [0] the whole slab, [1] the planes that need no ghost data, [2] the one or two that do (decomposed
  // grids; empty on a slab with two physical faces), each in (z block, row block, x segment) order
  std::vector<PlaneRun> items;
  int list_base[3] = {0, 0, 0}, list_count[3] = {0, 0, 0};
  int first[3][9] = {};  // per list: its eight contiguous, equally heavy parts (one per XCD), as indices into items
};

// what the tile kernel cannot take, from the sizes alone
inline bool vtl_sizes_declined(int nx, int ny, int nz) {
  if (nz < 2 || nx < 2 || ny < 2) return true;                   // 1-D / 2-D grids and single planes: the segment list
  if ((int64_t)nx * ny >= ((int64_t)1 << 28)) return true;       // 32-bit byte offsets inside a plane
  return (int64_t)(ny + 2) * ((nx + SEG - 1) / SEG) * (nz + 6) >= ((int64_t)1 << 31);  // 32-bit mask offsets
}

inline std::vector<u64> vtl_masks(const PlanGrid& g, bool z_lo_phys, bool z_hi_phys, const std::vector<u64>& flags) {
  const int nsegx = g.nsegx(), nzp = g.nz + 6;
  std::vector<u64> mask((size_t)(g.ny + 2) * nsegx * nzp, 0ull);
  for (int y = 0; y < g.ny; ++y)
    for (int s = 0; s < nsegx; ++s) {
      u64* row = mask.data() + ((size_t)(y + 1) * nsegx + s) * nzp + 1;
      // the lanes [l0, l1) whose node 62 s - 1 + l lies inside the box
      const int l0 = s == 0 ? 1 : 0, l1 = std::min(64, g.nx - (s * SEG - 1));
      const u64 box = (l1 - l0 < 64 ? (1ull << (l1 - l0)) - 1ull : ~0ull) << l0;
      if (!z_lo_phys) row[-1] = box;
      if (!z_hi_phys) row[g.nz] = box;
      for (int z = 0; z < g.nz; ++z)
        row[z] = tissue_bits(flags, (int64_t)z * g.plane() + (int64_t)y * g.nx + (int64_t)s * SEG - 1 + l0, l1 - l0) << l0;
    }
  return mask;
}

// the tiles of the planes [z_lo, z_hi), in (z block, row block, x segment) order; false if there are more than max_items
inline bool vtl_tiles(const PlanGrid& g, const std::vector<u64>& flags, const VtlPlanOptions& o, int z_lo, int z_hi, int run,
                      std::vector<PlaneRun>& items) {
  items.clear();
  if (z_hi <= z_lo) return true;
  const int nrb = (g.ny + o.ry - 1) / o.ry;
  std::vector<char> act((size_t)g.nz);
  for (int rb = 0; rb < nrb; ++rb)
    for (int seg = 0; seg < g.nsegx(); ++seg) {
      if (!column_activity(g, flags, seg, rb, o.ry, z_lo, z_hi, act)) continue;
      if (o.aligned) {
        // every tile of a z block covers the block's tissue range as a whole (aligned 2: the whole block)
        for (int b0 = (z_lo / run) * run; b0 < z_hi; b0 += run) {
          const int c0 = std::max(b0, z_lo), c1 = std::min(z_hi, b0 + run);
          int lo = c1, hi = c0;
          for (int z = c0; z < c1; ++z)
            if (act[(size_t)z]) {
              lo = std::min(lo, z);
              hi = std::max(hi, z + 1);
            }
          if (lo >= hi) continue;
          items.push_back(o.aligned == 2 ? PlaneRun{seg, rb, c0, c1} : PlaneRun{seg, rb, lo, hi});
        }
        continue;
      }
      // a run never crosses a multiple of `run`: tiles of one z block are neighbours in the list
      grow_runs(act, seg, rb, z_lo, z_hi, [run](int z) { return ((int64_t)(z / run) + 1) * run; }, items);
    }
  std::stable_sort(items.begin(), items.end(), [&](const PlaneRun& p, const PlaneRun& q) {
    const int zp = p.zb / run, zq = q.zb / run;
    if (zp != zq) return zp < zq;
    if (p.rb != q.rb) return p.rb < q.rb;
    return p.seg < q.seg;
  });
  return (int64_t)items.size() <= o.max_items;
}

// eight contiguous parts of equal weight (planes + a prologue's worth per tile); indices into the concatenated array
inline void vtl_parts(const std::vector<PlaneRun>& items, int base, int (&first)[9]) {
  std::vector<int64_t> cum(items.size() + 1, 0);
  for (size_t k = 0; k < items.size(); ++k) cum[k + 1] = cum[k] + (items[k].ze - items[k].zb) + 2;
  first[0] = 0;
  for (int x = 1; x < 8; ++x) {
    const int64_t want = cum.back() * x / 8;
    first[x] = (int)(std::lower_bound(cum.begin(), cum.end(), want) - cum.begin());
    first[x] = std::max(first[x - 1], std::min(first[x], (int)items.size()));
  }
  first[8] = (int)items.size();
  for (int x = 0; x < 9; ++x) first[x] += base;
}

inline VtlPlan vtl_plan(int nx, int ny, int nz, bool z_lo_phys, bool z_hi_phys, const std::vector<u64>& flags, const VtlPlanOptions& o) {
  VtlPlan p;
  if (vtl_sizes_declined(nx, ny, nz)) return p;
  const PlanGrid g{nx, ny, nz};
  // (one partial sum of p.q per tile: longer runs if there would be more tiles than partial slots)
  int run = o.max_run;
  bool fits = false;
  for (; !(fits = vtl_tiles(g, flags, o, 0, nz, run, p.items)) && run < nz; run *= 2) {
  }
  if (!fits) {  // (a plane of more than max_items tiles: the segment-list kernel)
    p.items.clear();
    return p;
  }
  p.declined = false;
  p.nsegx = g.nsegx();
  p.nzp = nz + 6;
  p.run = run;
  p.mask = vtl_masks(g, z_lo_phys, z_hi_phys, flags);
  std::vector<PlaneRun> part_items[2];
  if (!(z_lo_phys && z_hi_phys)) {
    // a decomposed grid: the planes that need no ghost plane of p (their launch overlaps the exchange), then the one or two
    // slab-boundary planes (beat_slab_part)
    const SlabPart inner = beat_slab_part(nz, z_lo_phys, z_hi_phys, 0), boundary = beat_slab_part(nz, z_lo_phys, z_hi_phys, 1);
    std::vector<PlaneRun> plane_items;
    bool ok = vtl_tiles(g, flags, o, inner.range[0].z_lo, inner.range[0].z_hi, run, part_items[0]);
    for (int k = 0; k < boundary.count; ++k) {
      ok = vtl_tiles(g, flags, o, boundary.range[k].z_lo, boundary.range[k].z_hi, run, plane_items) && ok;
      part_items[1].insert(part_items[1].end(), plane_items.begin(), plane_items.end());
    }
    if (!ok || (int64_t)part_items[0].size() + (int64_t)part_items[1].size() > o.max_items) {
      part_items[0].clear();  // (the split launches keep the segment-list kernel)
      part_items[1].clear();
    }
  }
  p.list_count[0] = (int)p.items.size();
  vtl_parts(p.items, 0, p.first[0]);
  for (int k = 0; k < 2; ++k) {
    p.list_base[k + 1] = (int)p.items.size();
    p.list_count[k + 1] = (int)part_items[k].size();
    vtl_parts(part_items[k], p.list_base[k + 1], p.first[k + 1]);
    p.items.insert(p.items.end(), part_items[k].begin(), part_items[k].end());
  }
  return p;
}

// ---- the column runs of vrr_spmv_kernel -------------------------------------------------------------------------------------------
struct VrrPlanOptions {
  int ry = 2;  // rows per wave: 2 or 4
  int max_run = MAX_RUN;
};

struct VrrPlan {
  std::vector<PlaneRun> items;  // [whole | interior | boundary] lists, back to back, each sorted long runs first
  int first[3] = {0, 0, 0}, count[3] = {0, 0, 0};
};

inline VrrPlan vrr_plan(int nx, int ny, int nz, bool z_lo_phys, bool z_hi_phys, const std::vector<u64>& flags, const VrrPlanOptions& o) {
  const PlanGrid g{nx, ny, nz};
  const int nrb = (ny + o.ry - 1) / o.ry;
  const SlabPart inner = beat_slab_part(nz, z_lo_phys, z_hi_phys, 0), boundary = beat_slab_part(nz, z_lo_phys, z_hi_phys, 1);
  const auto limit = [&o](int z) { return (int64_t)z + o.max_run; };
  std::vector<PlaneRun> lists[3];
  std::vector<char> act((size_t)nz);
  for (int rb = 0; rb < nrb; ++rb)
    for (int seg = 0; seg < g.nsegx(); ++seg) {
      if (!column_activity(g, flags, seg, rb, o.ry, 0, nz, act)) continue;
      grow_runs(act, seg, rb, 0, nz, limit, lists[0]);
      grow_runs(act, seg, rb, inner.range[0].z_lo, inner.range[0].z_hi, limit, lists[1]);
      for (int k = 0; k < boundary.count; ++k) grow_runs(act, seg, rb, boundary.range[k].z_lo, boundary.range[k].z_hi, limit, lists[2]);
    }
  VrrPlan p;
  for (int k = 0; k < 3; ++k) {
    // long runs first: the tail of the launch is made of short ones
    std::stable_sort(lists[k].begin(), lists[k].end(), [](const PlaneRun& a, const PlaneRun& b) { return a.ze - a.zb > b.ze - b.zb; });
    p.first[k] = (int)p.items.size();
    p.count[k] = (int)lists[k].size();
    p.items.insert(p.items.end(), lists[k].begin(), lists[k].end());
  }
  return p;
}

}  // namespace beat_pde_detail
