// Per-node-coefficient SpMV of the PCG on workgroup tiles: q = A p with every stored forward coefficient and every row
// of p loaded ONCE per tile, the rest shared on chip.
//
// The segment-list kernel (var_spmv_kernel, beat_pde_var.hip) issues 23 wave-level loads per 64 nodes -- 8 forward
// coefficients, 7 backward ones read as the neighbours' forward coefficients a row or a plane away, 7 rows of p, the
// segment's edge values -- and moves 121 B per tissue node from beyond the L2 on the 401^3 shell (PMC, round 3) against
// the 80 B a node owns (8 coefficients, p, q).  The z-marching kernel of round 3 (beat_pde_vrr.hip) loads the forward
// half only but keeps RY rows x 3 planes of p and two sets of coefficients per WAVE (180-240 VGPRs), loads its whole
// footprint whether tissue or not, and reads the tissue bits with a vector load inside the march (a vmcnt(0) per plane
// that drains its prefetch).  Here:
//   * a WORKGROUP owns a tile of 62 x-nodes (lanes 1..62 of a wave; lanes 0 and 63 carry the x-halo) x RY rows, one row
//     per wave, and marches along z over a run of planes that hold tissue;
//   * per plane a wave loads its row's 8 forward coefficients and ONE row of p (the plane after next; both one step ahead
//     of their use); its own row's three planes of p and the four slots that point to the plane above stay in registers;
//   * what a row needs from the rows next to it -- p of the rows above and below, the four forward slots of the row
//     below that point up (+y, +x+y, +y+z, +x+y+z: its backward -y, -x-y, -y-z, -x-y-z) -- goes through LDS: every wave
//     publishes its row once per plane, one barrier per plane, two buffers; the two halo rows of the tile (p above and
//     below, the four slots of the row below) are six more loads per plane, dealt to the waves;
//   * x-neighbours by DPP wave shifts; lanes on nodes outside the tissue issue no loads (per-row 64-bit masks, a table
//     laid out along z and read with scalar loads two steps ahead), so lines without tissue are never fetched.
// Per plane and tile: 9 RY + 6 wave loads for 62 RY nodes (RY = 8: 9.75 per 62 nodes instead of 23 per 64).  The values
// of q are those of var_spmv_kernel bit for bit (same coefficients, the same 15 fused multiply-adds in slot order);
// p.q is summed per TILE and the tiles in list order (the same bits whoever computed what).
// Inside the solver the same pass also FORMS the search direction (PDOT = true, beat_vtl_pdot): it reads r and the previous
// direction instead of p, builds p = D^-1 r + beta p_old wherever the product needs it (own row, rows above and below, halo
// lanes; D^-1 = 1 / the row's own centre coefficient), stores it and computes q = A p -- var_pupdate_oop_kernel's pass over
// r, p_old and 1/diag is gone from the iteration.  Three tile lists per operator: the whole slab, and for decomposed
// grids the planes that need no ghost plane of p and the one or two that do (beat_vtl_spmv_dot_part).
// Measured (profiles/r04_shell400.md, r04_var_resources.md): SpMV 529-543 -> 403-427 us on an 18.6 M-node shell, 121 -> 105
// B/node from beyond the L2; the fused pass 475 us against 375 + 125; 119-125 VGPRs, no scratch, no spilled SGPR.
//
// Replaces, like beat_pde_var.hip, PETSc's MatMult inside KSP.solve (src/beat/base_model.py:236) for operators assembled
// from per-cell conductivity tensors (src/beat/conductivities.py:101-118, demos/biv_endocardial.py:187-282).
#include "beat_pde_internal.h"
#include "beat_pde_device.h"
#include "beat_var_plan.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace {
using namespace beat_pde_detail;

// (SEG = 62, the x-nodes computed per wave (lanes 1..62), and u64: beat_var_plan.h)
using VtlItem = PlaneRun;  // tile column (x segment, row block) and the planes [zb, ze) it computes

struct VtlArgs {
  int64_t ld;
  int nx, ny, nz;
  int64_t plane;
  int nsegx;  // x segments per row
  int nzp;    // entries per (row, x segment) of the mask table: planes -1 .. nz + padding
  double* partials;
  int part_off;
  const double* st;
  const double* x;         // p
  double* y;               // q
  const double* rows;      // (15, ld) coefficient rows of A
  const unsigned long long* mask;  // lane masks per (row, x segment) along z
  const VtlItem* items;
  const int* xcd_first;    // 9 entries: the part of the tile list each XCD walks
  int* next;               // 8 counters (next tile of each part) + the number of workgroups done
  // PDOT (the solver's iteration): x = the PREVIOUS search direction, the new one is formed while loading --
  // p = D^-1 r + beta p_old, D^-1 = 1 / the row's own centre coefficient -- and stored to pnew
  const double* r;
  double* pnew;
  int first;               // bit 0: iteration 0, p = D^-1 r (beta = 0, p_old not read); bit 1: keep the direction on the lower ghost plane
  // PDOT on a slab with live neighbours (beat_vtl_pdot_part): the centre coefficients of the NEIGHBOURS' boundary planes (one
  // plane each, exchanged once per operator) -- the direction is formed on the ghost planes too, from the exchanged r, the
  // previous direction kept there and these, and stored there, so that p itself is never exchanged.  nullptr: a physical face.
  const double* gc0_lo;
  const double* gc0_hi;
  // The right-hand side of a step in two single-window passes (round 5; the constant-coefficient kernels' formulation,
  // beat_pde_rr.hip: b = B v_ + dt stim, r = b - A x0):
  //   BV  (mode 2): rows = the rows of B, x = v_, y = b (stored), per-tile partials of b.b
  //   RES (mode 4): rows = A, x = the guess increment e (or nullptr), r = v_ -- the window holds x0 = v_ + e, formed while loading
  //                 as PDOT forms the direction --, t = b, y = the residual b - A x0, pnew = D^-1 r (or nullptr: not wanted),
  //                 per-tile partials of r.z and r.r (slots 1 and 2)
  const double* t;
  double dt;
  const double* w[BEAT_MAX_STIM];
  double amp[BEAT_MAX_STIM];
  int nstim;
  int ignore_stop;         // launches outside the iteration (the latch of the previous solve is still set)
};

// One plane of a field (or of a coefficient row) as a raw buffer: a lane that wants nothing passes an offset beyond the
// buffer's end -- its load returns 0 and fetches nothing, its store is dropped -- so neither needs a branch or a change
// of the exec mask, and the compiler can count what is outstanding at every point of the march.
// (-DBEAT_VTL_NT, an experiment of round 5: bit 0 = the coefficient loads non-temporal -- every coefficient is read once per pass
// and should not push the vector rows the neighbouring tiles share out of the L2 --, bit 1 = the stores of p and q; measured in
// profiles/r05_shell400.md; default 0)
#ifndef BEAT_VTL_NT
#define BEAT_VTL_NT 0
#endif
__device__ __forceinline__ void vtl_buf_store(double* base, unsigned bytes, unsigned off, double val) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
  buf_v2i v;
  v.x = __double2loint(val);
  v.y = __double2hiint(val);
  __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)off, 0, (BEAT_VTL_NT & 2) ? 2 : 0);
}

// forward slots of the 15-point stencil (beat_stencil_offsets): 0 centre, 1 +x, 3 +y, 5 +z, 7 +x+y, 9 +y+z, 11 +x+z,
// 13 +x+y+z; the backward slot k+1 pairs with the forward slot k.  F[] below holds them in that order.
template <int RY, bool DYN, int MODE>
__global__ __launch_bounds__(RY * 64, 4) void vtl_spmv_kernel(VtlArgs a_) {  // MODE: 0 q = A p | 1 PDOT | 2 BV | 3 PDOT, live neighbours | 4 RES
  constexpr bool PDOT = MODE == 1 || MODE == 3, BV = MODE == 2, RES = MODE == 4;
  constexpr bool FORMED = PDOT || RES;  // the window's values are formed from several loads (PDOT: r, p_old, c0; RES: v_, e)
  constexpr bool GHOST = MODE == 3;  // PDOT on a slab with live neighbours: the direction is formed and kept on the ghost planes too
  constexpr int NPE = 2;  // halo entries that are rows of a vector: p below / above
  // one LDS array: p of plane z+1 for rows y0-1 .. y0+RY of the tile (two buffers), slots 3, 7, 9, 13 of plane z for rows
  // y0-1 .. y0+RY-2 (two buffers), and a row per wave that absorbs the stores of a wave without a (second) halo load
  constexpr int P_PAR = (RY + 2) * 64, C_PAR = RY * 4 * 64;
  constexpr int P_BASE = 0, C_BASE = 2 * P_PAR, DUMMY = C_BASE + 2 * C_PAR;
  constexpr bool TWO = RY < NPE + 4;  // NPE + 4 halo loads per plane: two per wave when a tile has fewer rows than that
  static_assert(!(RES || BV) || !TWO, "the right-hand side passes are built for tiles of 8 rows");
  __shared__ double lds[DUMMY + RY * 64];
  __shared__ double red[3 * RY];
  __shared__ int next_item;
  if (a_.st[STOP] != 0.0 && !a_.ignore_stop) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 lanebit = 1ull << lane;
  // Every XCD (blocks b with b % 8 == x) walks one contiguous, equally heavy part of the tile list, front to back: the
  // tiles its workgroups have in flight are neighbours, the halo rows and lanes they share are lines its L2 holds.  A
  // workgroup that is done takes the part's next tile (one counter per XCD; tiles differ by a factor of ten in tissue,
  // dealt round-robin the average wave was alive 75 % of the launch), and helps the other XCDs out once its own part is
  // exhausted.  p.q is summed per TILE, the reduction adds the tiles in list order: the same bits whoever computed what.
  // DYN = false (the default, see beat_vtl_setup): the tiles of a part dealt round-robin to the XCD's workgroups.
  const int xcd = blockIdx.x & 7;
  int static_it = a_.xcd_first[xcd] + (int)(blockIdx.x >> 3);
  for (;;) {
    // (taken by wave 0 as a whole, uniformly; only the atomic itself is one lane's.  Written as `if (threadIdx.x == 0)` at
    // the head of the loop, the compiler split the loop by lanes and wave 0 executed the barrier below twice per round.)
    if (w == 0) {
      int got = -1;
      if (DYN) {
        for (int k = 0; k < 8 && got < 0; ++k) {
          const int x = (xcd + k) & 7;
          const int first = a_.xcd_first[x], end = a_.xcd_first[x + 1];
          if (first < end) {
            int n = 0;
            if (lane == 0) n = atomicAdd(a_.next + x, 1);
            n = __builtin_amdgcn_readfirstlane(n);
            if (n < end - first) got = first + n;
          }
        }
      } else {
        if (static_it < a_.xcd_first[xcd + 1]) got = static_it;
        static_it += (int)(gridDim.x >> 3);
      }
      if (lane == 0) next_item = got;
    }
    __syncthreads();  // (also: the previous tile's last reads of the LDS buffers are done)
    const int it = __builtin_amdgcn_readfirstlane(next_item);
    if (it < 0) break;
    double acc = 0.0;
    // the kernel arguments through a pointer the optimiser cannot see through, per tile: read where a tile needs them
    // instead of being held in SGPRs from the top of the kernel on (the kernel has none to spare)
    typedef const __attribute__((address_space(4))) char* KArgPtr;
    KArgPtr ka = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const VtlArgs& a = *(const VtlArgs*)ka;
    const double* __restrict__ X = a.x;
    const double* __restrict__ A = a.rows;
    const u64* __restrict__ MASK = a.mask;
    const VtlItem item = a.items[it];  // wave-uniform
    const int y0 = item.rb * RY, zb = item.zb, ze = item.ze;
    const int gy = y0 + w;
    const int gx = item.seg * SEG - 1 + lane;
    const int cx = min(max(gx, 0), a.nx - 1);
    // rows of the mask table: index y + 1 for y = -1 .. ny (both ends all zero); z + 1 for z = -1 .. nz
    // (32-bit offsets into the table: the set-up refuses grids whose table has 2^31 entries)
    const int ty = min(gy, a.ny), tyu = min(gy + 1, a.ny), tyd = min(gy - 1, a.ny);
    const int mo_own = ((ty + 1) * a.nsegx + item.seg) * a.nzp + 1;
    const unsigned roff = (unsigned)(min(gy, a.ny - 1) * a.nx + cx);
    // Everything inside the march is data, not control flow: a load that is not wanted (a lane outside the tissue, a plane
    // beyond the run, a halo load this wave does not have) gets an empty mask, i.e. out-of-range offsets in every lane.
    // With branches around the loads and the store the compiler cannot count what is outstanding where the paths join
    // and waits for everything (vmcnt(0) right behind the store of q, every plane).
    const unsigned pbytes = (unsigned)a.plane * 8u;
    auto lane_off = [&](u64 mk, unsigned ro) -> unsigned { return (mk & lanebit) ? ro * 8u : BUF_OOB; };
    auto ldp = [&](u64 mk, int z, unsigned ro) -> double { return buf_load(X + (int64_t)z * a.plane, pbytes, lane_off(mk, ro)); };
    auto ldc = [&](u64 mk, int slot, int z, unsigned ro) -> double {
      return buf_load(A + (int64_t)slot * a.ld + (int64_t)z * a.plane, pbytes, lane_off(mk, ro));
    };
    // PDOT: a value of p is formed from three loads -- the residual, the previous direction and the row's centre coefficient
    // c0 (D^-1 = 1 / c0, rounded as var_form_A_kernel rounds the stored 1/diag; p = fma(beta, p_old, D^-1 r): the very
    // expression of var_pupdate_oop_kernel, so the same bits) -- wherever the SpMV needs it: the own row, the rows above and
    // below, the halo lanes.  Redundant arithmetic on the halo, no second pass over r, p_old and 1/diag (32 B/node).
    const double beta = PDOT ? a.st[BETA] : 0.0;
    const bool first = PDOT && (a.first & 1) != 0;
    struct Trio {
      double r, q, c0;
    };
    auto form = [&](const Trio& t) -> double {
      if constexpr (RES) {
        return t.r + t.q;  // x0 = v_ + e (a lane that loaded nothing: 0 + 0; without a guess e is not read: + 0)
      } else {
        const double di = 1.0 / t.c0;
        const double zz = di * t.r;
        const double pv = first ? zz : fma(beta, t.q, zz);
        return t.c0 != 0.0 ? pv : 0.0;  // (a lane that loaded nothing: c0 = 0)
      }
    };
    // RES: the second operand of a formed value is the guess increment; nullptr (no guess on record): never read
    const bool no_second = RES ? X == nullptr : first;
    // centre coefficients of plane z: slot 0 of the rows, or the neighbour's plane on a ghost plane
    auto c0_of = [&](int z) -> const double* {
      if constexpr (GHOST) {
        KArgPtr kg = ka;
        asm volatile("" : "+s"(kg));
        const VtlArgs& ag = *(const VtlArgs*)kg;
        return z < 0 ? ag.gc0_lo : (z >= a.nz ? ag.gc0_hi : A + (int64_t)z * a.plane);
      } else {
        return A + (int64_t)z * a.plane;
      }
    };
    auto ld3 = [&](u64 mk, int z, unsigned ro) -> Trio {
      const unsigned off = lane_off(mk, ro);
      KArgPtr kr = ka;
      asm volatile("" : "+s"(kr));
      const double* Rr = ((const VtlArgs*)kr)->r;
      Trio t;
      t.r = buf_load(Rr + (int64_t)z * a.plane, pbytes, off);
      t.q = buf_load(X + (int64_t)z * a.plane, pbytes, no_second ? BUF_OOB : off);
      t.c0 = RES ? 0.0 : buf_load(c0_of(z), pbytes, off);
      return t;
    };
    // (a ghost plane of a physical face: its mask is empty, nothing is loaded, p = 0; the decomposed solve does not come here)
    auto ldpv = [&](u64 mk, int z, unsigned ro) -> double {  // p at (row ro, plane z), straight from memory
      if constexpr (FORMED) {
        return form(ld3(mk, z, ro));
      } else {
        return ldp(mk, z, ro);
      }
    };
    // the halo rows of the tile: p of rows y0-1 and y0+RY (consumed like the waves' own p: loaded for plane z+2 at step
    // z), slots 3, 7, 9, 13 of row y0-1 (like the own coefficients: plane z+1 at step z); wave w takes halo loads w and
    // w + RY of the six (e: 0 = p below, 1 = p above, 2..5 = slot 3 / 7 / 9 / 13 of the row below).  What a halo load
    // needs is re-derived from its number where it is used (a handful of scalar instructions per plane): kept as
    // pointers, the descriptors cost the SGPRs the kernel does not have
    const int ea = w, eb = w + RY;
    auto halo_row = [&](int e) -> int { return (e < NPE && (e & 1)) ? y0 + RY : y0 - 1; };
    const unsigned roff_a = (unsigned)(min(max(halo_row(ea), 0), a.ny - 1) * a.nx + cx);
    const unsigned roff_b = (unsigned)(min(max(halo_row(eb), 0), a.ny - 1) * a.nx + cx);
    const int moff_a = ((min(max(halo_row(ea), -1), a.ny) + 1) * a.nsegx + item.seg) * a.nzp + 1;
    const int moff_b = ((min(max(halo_row(eb), -1), a.ny) + 1) * a.nsegx + item.seg) * a.nzp + 1;
    auto halo_plane = [&](int e, int z) -> int { return z + (e < NPE ? 2 : 1); };  // what step z loads (step z+1 publishes)
    auto halo_mask = [&](int e, int moff, int z) -> u64 { return MASK[moff + halo_plane(e, z)]; };
    auto halo_load = [&](int e, u64 mk, unsigned ro, int z) -> Trio {
      const bool is_p = e < NPE;
      const int zz = halo_plane(e, z);
      const bool want = e < NPE + 4 && zz <= (is_p ? ze : ze - 1);
      const u64 m = want ? mk : 0ull;
      int64_t ld = a.ld;
      asm volatile("" : "+s"(ld));
      const int slot = (0xD973 >> (4 * ((e - NPE) & 3))) & 15;  // 3, 7, 9, 13
      Trio t{0.0, 0.0, 0.0};
      if constexpr (FORMED) {
        // a p entry is three loads (r, p_old, c0; RES: v_, e), a coefficient entry one: the others run with every lane out of range
        KArgPtr kr = ka;
        asm volatile("" : "+s"(kr));
        const double* base = is_p ? ((const VtlArgs*)kr)->r : A + slot * ld;
        const unsigned off = lane_off(m, ro), offp = is_p ? off : BUF_OOB;
        t.r = buf_load(base + (int64_t)zz * a.plane, pbytes, off);
        t.q = buf_load(X + (int64_t)zz * a.plane, pbytes, no_second ? BUF_OOB : offp);
        t.c0 = RES ? 0.0 : buf_load(c0_of(zz), pbytes, offp);
      } else {
        const double* base = is_p ? X : A + slot * ld;
        t.r = buf_load(base + (int64_t)zz * a.plane, pbytes, lane_off(m, ro));
      }
      return t;
    };
    auto halo_value = [&](int e, const Trio& t) -> double {  // what is published: p of the halo row, or the coefficient
      if constexpr (FORMED) {
        return e < 2 ? form(t) : t.r;
      } else {
        return t.r;
      }
    };
    auto halo_lds = [&](int e, int z) -> int {  // where step z publishes it
      const int par = (e < NPE ? z + 1 : z) & 1;
      const int p_at = P_BASE + par * P_PAR + (e & 1) * (RY + 1) * 64, c_at = C_BASE + par * C_PAR + (e - NPE) * 64;
      const int at = e < NPE ? p_at : c_at;
      return e >= NPE + 4 ? DUMMY + w * 64 : at;
    };

    // ---- prologue: the planes below the run, straight from memory ------------------------------------------------------
    u64 M0 = MASK[mo_own + zb], M1 = MASK[mo_own + zb + 1], M2 = MASK[mo_own + zb + 2];
    double Pm, P0, U0, D0, Dm, K5, K9, K11, K13;
    double C0keep = 0.0;  // PDOT: the centre coefficient of the plane after this one's p was formed from, until it is F[0]
    double acc1 = 0.0, acc2 = 0.0;  // RES: the partials of r.z and r.r
    const u64 out_lanes = ((1ull << SEG) - 1ull) << 1;
    bool direct = zb == 0;
    {
      const int mo_up = ((tyu + 1) * a.nsegx + item.seg) * a.nzp + 1;
      const int mo_dn = ((tyd + 1) * a.nsegx + item.seg) * a.nzp + 1;
      const unsigned roff_up = (unsigned)(min(gy + 1, a.ny - 1) * a.nx + cx);
      const unsigned roff_dn = (unsigned)(max(gy - 1, 0) * a.nx + cx);
      const u64 mo = MASK[mo_own + zb - 1], md = MASK[mo_dn + zb - 1];
      Pm = ldpv(mo, zb - 1, roff);
      if constexpr (RES) {
        P0 = form(ld3(M0, zb, roff));
      } else if constexpr (PDOT) {

        const Trio t0 = ld3(M0, zb, roff);
        P0 = form(t0);
        C0keep = t0.c0;
        // this tile's first plane of the new direction (the later ones are stored as they are formed, one plane ahead) and -- on
        // plane 0 of a slab with a live lower neighbour, bit 1 of `first` -- the direction on the ghost plane below it, kept for
        // the next iteration: the two planes as ONE buffer (a second descriptor costs the SGPRs the kernel does not have)
        if constexpr (GHOST) {
          double* const two = a.pnew + (int64_t)(zb - 1) * a.plane;
          vtl_buf_store(two, 2u * pbytes, (zb == 0 && (a.first & 2) && (mo & lanebit & out_lanes)) ? roff * 8u : BUF_OOB, Pm);
          vtl_buf_store(two, 2u * pbytes, (M0 & lanebit & out_lanes) ? pbytes + roff * 8u : BUF_OOB, P0);
        } else {
          vtl_buf_store(a.pnew + (int64_t)zb * a.plane, pbytes, (M0 & lanebit & out_lanes) ? roff * 8u : BUF_OOB, P0);
        }
      } else {
        P0 = ldp(M0, zb, roff);
      }
      U0 = ldpv(MASK[mo_up + zb], zb, roff_up);
      D0 = ldpv(MASK[mo_dn + zb], zb, roff_dn);
      Dm = ldpv(md, zb - 1, roff_dn);
      // coefficients of the plane below towards this one: slots 5 / 11 of the own row, 9 / 13 of the row below.  Plane 0
      // of a slab has no stored plane below it: its own backward slots 6, 10, 12, 14 are used as they are (what
      // var_spmv_kernel does; zero on a physical face)
      const int zc = direct ? 0 : zb - 1;
      const u64 mk_o = direct ? M0 : mo, mk_d = direct ? M0 : md;
      const unsigned ro_d = direct ? roff : roff_dn;
      K5 = ldc(mk_o, direct ? 6 : 5, zc, roff);
      K11 = ldc(mk_o, direct ? 12 : 11, zc, roff);
      K9 = ldc(mk_d, direct ? 10 : 9, zc, ro_d);
      K13 = ldc(mk_d, direct ? 14 : 13, zc, ro_d);
    }
    // in flight for the first step: this plane's coefficients, p of the next plane, the halo rows' share
    double Fn[8];
    auto load_coefs = [&](u64 mk, int z) {
      const unsigned off = lane_off(mk & ~(1ull << 63), roff);  // lane 63 is the +x halo: nobody needs its coefficients
      // the row stride opaque per plane: otherwise the seven products k ld are loop invariants, hoisted into SGPR pairs
      // the kernel does not have (31 spilled to VGPR lanes)
      int64_t ld = a.ld;
      asm volatile("" : "+s"(ld));
      const double* bc = A + (int64_t)z * a.plane;
      constexpr int CNT = (BEAT_VTL_NT & 1) ? 2 : 0;
      Fn[0] = PDOT ? 0.0 : buf_load<CNT>(bc, pbytes, off);  // (PDOT: the centre coefficient comes with r and p_old, a plane earlier)
      bc += ld;
      Fn[1] = buf_load<CNT>(bc, pbytes, off);
      ld += ld;
#pragma unroll
      for (int k = 2; k < 8; ++k) {
        bc += ld;
        Fn[k] = buf_load<CNT>(bc, pbytes, off);
      }
    };
    load_coefs(M0, zb);
    double Pn = 0.0, Bn = 0.0;
    Trio Tn{0.0, 0.0, 0.0};
    if constexpr (FORMED) {
      Tn = ld3(M1, zb + 1, roff);
    } else {
      Pn = ldp(M1, zb + 1, roff);
    }
    if constexpr (RES) Bn = buf_load(a.t + (int64_t)zb * a.plane, pbytes, lane_off(M0, roff));  // b of this plane
    Trio Ean = halo_load(ea, halo_mask(ea, moff_a, zb - 1), roff_a, zb - 1);
    Trio Ebn{0.0, 0.0, 0.0};
    if (TWO) Ebn = halo_load(eb, halo_mask(eb, moff_b, zb - 1), roff_b, zb - 1);
    u64 HA = halo_mask(ea, moff_a, zb), HB = TWO ? halo_mask(eb, moff_b, zb) : 0ull;  // masks of the loads step zb issues
    for (int z = zb; z < ze; ++z) {
      // (what a plane uses once -- the output pointers -- is read from the kernel arguments where it is used, every plane: held
      // in SGPRs across the march it was spilled to VGPR lanes)
      KArgPtr kz = ka;
      asm volatile("" : "+s"(kz));
      const VtlArgs& az = *(const VtlArgs*)kz;
      double F[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) F[k] = Fn[k];
      double Pp = Pn;
      if constexpr (RES) Pp = form(Tn);  // x0 of plane z + 1
      if constexpr (PDOT) {
        Pp = form(Tn);  // p of plane z + 1, from what step z - 1 requested
        F[0] = C0keep;
        C0keep = Tn.c0;
        // (the plane above a slab with a live upper neighbour: the direction on the ghost plane, kept for the next iteration)
        const bool keep = z + 1 < ze || (GHOST && z + 1 == a.nz && az.gc0_hi != nullptr);
        vtl_buf_store(az.pnew + (int64_t)(z + 1) * a.plane, pbytes, (keep && (M1 & lanebit & out_lanes)) ? roff * 8u : BUF_OOB, Pp);
      }
      const double Ea = halo_value(ea, Ean), Eb = TWO ? halo_value(eb, Ebn) : 0.0;
      const double Bv = Bn;
      // masks: one step (the halo loads') and two steps (the own row's) ahead of their use
      const u64 M3 = MASK[mo_own + z + 3];
      const u64 HAn = halo_mask(ea, moff_a, z + 1);
      const u64 HBn = TWO ? halo_mask(eb, moff_b, z + 1) : 0ull;
      // next step's operands
      load_coefs(z + 1 < ze ? M1 : 0ull, z + 1);
      if constexpr (FORMED) {
        Tn = ld3(z + 2 <= ze ? M2 : 0ull, z + 2, roff);
      } else {
        Pn = ldp(z + 2 <= ze ? M2 : 0ull, z + 2, roff);
      }
      if constexpr (RES) Bn = buf_load(az.t + (int64_t)(z + 1) * a.plane, pbytes, lane_off(z + 1 < ze ? M1 : 0ull, roff));
      Ean = halo_load(ea, HA, roff_a, z);
      if (TWO) Ebn = halo_load(eb, HB, roff_b, z);
      // publish this row
      lds[P_BASE + ((z + 1) & 1) * P_PAR + (w + 1) * 64 + lane] = Pp;
      {
        double* __restrict__ cw = lds + (w + 1 < RY ? C_BASE + (z & 1) * C_PAR + (w + 1) * 4 * 64 : DUMMY + w * 64) + lane;
        const int cs = w + 1 < RY ? 64 : 0;
        cw[0] = F[2];
        cw[cs] = F[4];
        cw[2 * cs] = F[5];
        cw[3 * cs] = F[7];
      }
      lds[halo_lds(ea, z) + lane] = Ea;
      if (TWO) lds[halo_lds(eb, z) + lane] = Eb;
      __syncthreads();
      const double* __restrict__ pr = lds + P_BASE + ((z + 1) & 1) * P_PAR + w * 64 + lane;
      const double Dn = pr[0], Un = pr[128];
      const double* __restrict__ cr = lds + C_BASE + (z & 1) * C_PAR + w * 4 * 64 + lane;
      const double H3 = cr[0], H7 = cr[64], H9 = cr[128], H13 = cr[192];
      double c[15], v[15];
      c[0] = F[0];
      c[1] = F[1];
      c[2] = from_left(F[1]);  // -x: the left neighbour's +x
      c[3] = F[2];
      c[4] = H3;                   // -y: the lower row's +y
      c[5] = F[3];
      c[6] = K5;                   // -z: the lower plane's +z
      c[7] = F[4];
      c[8] = from_left(H7);    // -x-y
      c[9] = F[5];
      c[10] = K9;                  // -y-z
      c[11] = F[6];
      const double K11l = from_left(K11), K13l = from_left(K13);
      c[12] = direct ? K11 : K11l;  // -x-z
      c[13] = F[7];
      c[14] = direct ? K13 : K13l;  // -x-y-z
      v[0] = P0;
      v[1] = from_right(P0);
      v[2] = from_left(P0);
      v[3] = U0;
      v[4] = D0;
      v[5] = Pp;
      v[6] = Pm;
      v[7] = from_right(U0);
      v[8] = from_left(D0);
      v[9] = Un;
      v[10] = Dm;
      v[11] = from_right(Pp);
      v[12] = from_left(Pm);
      v[13] = from_right(Un);
      v[14] = from_left(Dm);
      // values are selected, never multiplied by a zero coefficient: a stale ghost plane cannot leak a NaN
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 15; ++k) s = fma(c[k], (k == 0 || c[k] != 0.0) ? v[k] : 0.0, s);
      const bool out = (M0 & lanebit & out_lanes) != 0ull;
      if constexpr (BV) {
        // b = B v_ + dt stim (rr_kernel's expression for the constant-coefficient grids), stored for the second pass
        double stim = 0.0;
        for (int k = 0; k < az.nstim; ++k)
          stim = fma(az.amp[k], buf_load(az.w[k] + (int64_t)z * a.plane, pbytes, out ? roff * 8u : BUF_OOB), stim);
        const double b = fma(az.dt, stim, s);
        acc = fma(out ? b : 0.0, b, acc);
        vtl_buf_store(az.y + (int64_t)z * a.plane, pbytes, out ? roff * 8u : BUF_OOB, b);
      } else if constexpr (RES) {
        // s = A x0: r = b - A x0 (the textbook form: its rounding error is ~1e-16 |b|, far below any threshold rtol |b|), z = D^-1 r
        const double rr = Bv - s;
        const double zz = (1.0 / F[0]) * rr;
        if (out) {
          acc1 = fma(rr, zz, acc1);
          acc2 = fma(rr, rr, acc2);
        }
        vtl_buf_store(az.y + (int64_t)z * a.plane, pbytes, out ? roff * 8u : BUF_OOB, rr);
        vtl_buf_store(az.pnew + (int64_t)z * a.plane, pbytes, (out && az.pnew != nullptr) ? roff * 8u : BUF_OOB, zz);
      } else {
        acc = fma(out ? P0 : 0.0, s, acc);  // (an inactive lane's P0 is 0 anyway; s is finite)
        vtl_buf_store(az.y + (int64_t)z * a.plane, pbytes, out ? roff * 8u : BUF_OOB, s);
      }
      // roll: this plane becomes the plane below
      Pm = P0;
      P0 = Pp;
      U0 = Un;
      Dm = D0;
      D0 = Dn;
      K5 = F[3];
      K11 = F[6];
      K9 = H9;
      K13 = H13;
      direct = false;
      M0 = M1;
      M1 = M2;
      M2 = M3;
      HA = HAn;
      HB = HBn;
    }
    // the tile's share of p.q (BV: of b.b in slot 0; RES: of r.z and r.r in slots 1 and 2), summed in wave order
    if constexpr (RES) {
      acc1 = beat_wave_sum(acc1);
      acc2 = beat_wave_sum(acc2);
      if (lane == 0) {
        red[RY + w] = acc1;
        red[2 * RY + w] = acc2;
      }
    } else {
      acc = beat_wave_sum(acc);
      if (lane == 0) red[w] = acc;
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int q = (RES ? 1 : 0); q < (RES ? 3 : 1); ++q) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < RY; ++k) t += red[q * RY + k];
        if (lane == 0) a.partials[q * BEAT_MAX_PARTIALS + a.part_off + it] = t;
      }
    }
  }
  // the last workgroup to leave rewinds the counters for the next launch
  // (no fence: a __threadfence() here is an L2 write-back and invalidate per workgroup -- a thousand of them while the others
  // still live off the lines they share; the counters are only ever touched by atomics, and a workgroup's last grab, whose
  // result it had to see before it got here, precedes its tick)
  if (DYN && w == 0 && lane == 0) {
    if (atomicAdd(a_.next + 8, 1) == (int)gridDim.x - 1) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a_.next[k] = 0;
    }
  }
}

struct VtlData {
  int ry = 4;
  bool dyn = false;
  bool pdot = true;  // BEAT_VTL_PDOT=0: the three-kernel iteration (SpMV, residual update, direction update)
  bool rhs = true;   // the right-hand side in two tile passes (beat_vtl_rhs); BEAT_VTL_RHS=0: var_rhs_kernel's gathers
  VtlItem* d_items = nullptr;
  int* d_xcd_first = nullptr;  // per list 9 entries: the part of the list each XCD walks; then 9 counters (next tile per XCD, workgroups done)
  u64* d_mask = nullptr;
  // tile lists, back to back in d_items: [0] the whole slab, [1] the planes that need no ghost data, [2] the one or two that do
  // (decomposed grids; empty on a slab with two physical faces)
  int list_base[3] = {0, 0, 0}, list_count[3] = {0, 0, 0};
  int nitems = 0, nsegx = 0, nzp = 0;
  unsigned resident = 0;
};

template <int RY>
unsigned vtl_resident_blocks() {
  return std::min(beat_resident_blocks(vtl_spmv_kernel<RY, false, RY == 8 ? 1 : 0>, RY * 64, 256u), (unsigned)BEAT_MAX_PARTIALS) & ~7u;
}
}  // namespace

void beat_vtl_destroy(beat_pde* pde) {
  VtlData* d = (VtlData*)pde->vtl;
  if (d == nullptr) return;
  if (d->d_items) (void)hipFree(d->d_items);
  if (d->d_xcd_first) (void)hipFree(d->d_xcd_first);
  if (d->d_mask) (void)hipFree(d->d_mask);
  delete d;
  pde->vtl = nullptr;
}

// flags: tissue bits per 64-node segment of the slab (host copy).  Reads the switches, has vtl_plan (beat_var_plan.h) build the per-row
// lane masks along z and the lists of tiles (column x run of planes with tissue) in their eight equally heavy parts, uploads them.
int beat_vtl_setup(beat_pde* pde, const std::vector<unsigned long long>& flags) {
  // BEAT_VTL=0 keeps the segment-list kernel (var_spmv_kernel), which also serves every launch over part of a slab
  const char* sw = std::getenv("BEAT_VTL");
  if (sw != nullptr && sw[0] == '0') return BEAT_OK;
  const Geom& f = pde->g;
  if (vtl_sizes_declined(f.nx, f.ny, f.nz)) return BEAT_OK;
  VtlData* d = new VtlData();
  {
    const char* e = std::getenv("BEAT_VTL_RY");
    // eight rows per tile halve the share of the halo rows; four keep thin slabs busy.  Measured on the 401^3 shell, one box,
    // alternating (tools/vtl_ab.sh, rocprofv3 kernel times): 8 rows, runs of 16 planes, dynamic: 403 us; 8 / 32: 414-428;
    // 4 / 32 dealt statically: 423-429, dynamic: 447; 4 / 16: 409-420; 4 / 64: 466 -- the segment-list kernel: 535
    // (16 rows per tile -- 1024-thread workgroups, half the halo share again -- were built and measured too: 11.65 against 11.30 ms
    // per shell step, A B A B on one box: sixteen waves at one barrier per plane; not kept)
    d->ry = e ? (std::atoi(e) == 8 ? 8 : 4) : (f.ny >= 16 ? 8 : 4);
    // tiles dealt round-robin to an XCD's workgroups (default) or taken from a counter per XCD (BEAT_VTL_DYNAMIC=1).  The
    // counter balances better on paper and measured the same on the SpMV alone (tools/bench_voxel.py: 403 against 409 us),
    // but inside the shell's split step (tools/bench_biv.py --n 400, same box, alternating) the round trip of the atomic, with
    // the whole workgroup waiting behind it once per tile, cost 560 against 375 us per launch: 12.85 against 11.24 ms/step
    const char* dy = std::getenv("BEAT_VTL_DYNAMIC");
    d->dyn = dy && dy[0] == '1';
    const char* pd = std::getenv("BEAT_VTL_PDOT");
    d->pdot = !(pd && pd[0] == '0');
    // the right-hand side in two single-window tile passes (beat_vtl_rhs, round 5) is the default on single slabs with tiles
    // of 8 rows; BEAT_VTL_RHS=0 keeps var_rhs_kernel's gathers.  (Round 4's version -- K v_ in a first pass, then ONE pass over A
    // with two vector windows, 166 VGPRs and one workgroup per CU -- measured 1.12 against 1.30 ms and stayed opt-in; it is gone.)
    const char* rh = std::getenv("BEAT_VTL_RHS");
    d->rhs = !(rh && rh[0] == '0');
  }
  int max_run = 16;
  if (const char* e = std::getenv("BEAT_VTL_RUN")) max_run = std::max(1, std::atoi(e));
  // BEAT_VTL_ALIGN=1: every tile of a z block covers the block's tissue range as a whole, 2: the whole block.  Measured, within
  // +-2 % of tiles trimmed to their own tissue (the default)
  int aligned = 0;
  if (const char* e = std::getenv("BEAT_VTL_ALIGN")) aligned = std::atoi(e);
  VtlPlanOptions opt;
  opt.ry = d->ry;
  opt.max_run = max_run;
  opt.aligned = aligned;
  opt.max_items = BEAT_MAX_PARTIALS;
  const VtlPlan plan = vtl_plan(f.nx, f.ny, f.nz, f.z_lo_phys != 0, f.z_hi_phys != 0, flags, opt);
  if (plan.declined) {  // (a plane of more than 16384 tiles: the segment-list kernel)
    delete d;
    return BEAT_OK;
  }
  d->nsegx = plan.nsegx;
  d->nzp = plan.nzp;
  for (int k = 0; k < 3; ++k) {
    d->list_base[k] = plan.list_base[k];
    d->list_count[k] = plan.list_count[k];
  }
  d->nitems = d->list_count[0];
  pde->vtl = d;
  // per list the 9 entries of its parts, then the 9 counters (zero)
  std::vector<int> xcd_first(36, 0);
  for (int k = 0; k < 3; ++k) std::copy(plan.first[k], plan.first[k] + 9, xcd_first.begin() + 9 * k);
  hipError_t e = beat_upload(&d->d_items, plan.items);
  if (e == hipSuccess) e = beat_upload(&d->d_xcd_first, xcd_first);
  if (e == hipSuccess) e = beat_upload(&d->d_mask, plan.mask);
  if (e != hipSuccess) {
    beat_vtl_destroy(pde);
    beat_set_error("beat_vtl_setup: %s", hipGetErrorString(e));
    return BEAT_EHIP;
  }
  const int RY = d->ry;
  d->resident = RY == 8 ? vtl_resident_blocks<8>() : vtl_resident_blocks<4>();
  if (std::getenv("BEAT_VTL_VERBOSE")) {
    long planes = 0;
    for (int k = 0; k < d->nitems; ++k) planes += plan.items[(size_t)k].ze - plan.items[(size_t)k].zb;
    std::fprintf(stderr, "vtl: RY %d, %d x %d columns, %d tiles (+ %d / %d for the split launches), %.1f planes per tile, %u resident blocks\n", RY,
                 plan.nsegx, (f.ny + RY - 1) / RY, d->nitems, d->list_count[1], d->list_count[2], d->nitems ? (double)planes / d->nitems : 0.0, d->resident);
  }
  return BEAT_OK;
}

bool beat_vtl_available(const beat_pde* pde) { return pde->var && pde->vtl != nullptr && ((VtlData*)pde->vtl)->nitems > 0; }

// One tile pass: what it computes, over which list of tiles, and what each of its operands is
//   SPMV: q = A p, p.q -> st[PQ]                 PDOT: p_new = D^-1 r + beta p (first: D^-1 r) formed while loading and stored, q = A p_new
//   BV:   q = B p + dt sum_k amp_k w_k (p = v_)  RES:  q = t - A (p + e) (p = v_), p_new = D^-1 q if wanted, the sums -> red_out[0..3)
struct VtlPass {
  enum Kind { SPMV, PDOT, BV, RES };
  Kind kind = SPMV;
  int list = 0;           // 0: the whole slab | 1, 2: the tiles of part 0 / part 1 of a decomposed grid (beat_vtl_setup)
  int part_off = 0;       // partial slot of the list's first tile (one partial per tile, in list order)
  enum Reduce { NO_SUM, LIST, BOTH_PARTS };  // the partials summed behind the launch: none, this list's, lists 1 and 2 (part 1)
  Reduce reduce = LIST;
  double* st = nullptr;   // the scalar state: the latch and beta (SPMV, PDOT)
  const double* p = nullptr;  // SPMV: p | PDOT: p_old | BV, RES: v_
  double* q = nullptr;        // SPMV, PDOT: q | BV: b | RES: r
  const double* r = nullptr;  // PDOT: r
  double* p_new = nullptr;    // PDOT: p_new | RES: z = D^-1 r, or nullptr where nothing reads it
  bool first = false;         // PDOT: the first iteration (beta = 0, p unread)
  const double* const* stim_w = nullptr;  // BV: the caller's stimuli (beat_fill_stimuli)
  const double* stim_amp = nullptr;
  int n_stim = 0;
  const double* e = nullptr;  // RES: guess increment or nullptr
  const double* t = nullptr;  // RES: b
  double* red_out = nullptr;  // RES: b.b (from the BV pass), r.z, r.r
  const PcgStart* start = nullptr;  // RES: the start of the solve behind the sums, or nullptr
};
static int vtl_launch(beat_pde* pde, const VtlPass& ps);

// part -1: the whole slab (the defaults).  The two parts of a decomposed grid: part 0 = list 1 without a reduction, part 1 = list 2 and
// the sum over both lists' tiles
static void vtl_set_part(const beat_pde* pde, VtlPass& ps, int part) {
  if (part < 0) return;
  const VtlData* d = (const VtlData*)pde->vtl;
  ps.list = part + 1;
  ps.part_off = part == 0 ? 0 : d->list_count[1];
  ps.reduce = part == 0 ? VtlPass::NO_SUM : VtlPass::BOTH_PARTS;
}

// whole-slab q = A p and the sum p.q
int beat_vtl_spmv_dot(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st) {
  return beat_vtl_spmv_dot_part(pde, dev_p, dev_q, dev_st, -1);
}

// the solver's iteration in one pass: p_new = D^-1 r + beta p_old (beta from dev_st; first: p_new = D^-1 r) formed while
// loading and stored, q = A p_new, the sum p_new.q.  Single-slab operators only (both faces physical).
int beat_vtl_pdot(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new, double* dev_q, int first) {
  BEAT_REQUIRE(pde->g.z_lo_phys && pde->g.z_hi_phys, "beat_vtl_pdot is the single-slab path");
  return beat_vtl_pdot_part(pde, dev_st, dev_r, dev_p_old, dev_p_new, dev_q, first, -1);
}

bool beat_vtl_pdot_available(const beat_pde* pde) {
  // (tiles of 8 rows only: with 4 rows a wave carries two halo entries and the fused pass does not fit 128 VGPRs)
  return beat_vtl_available(pde) && ((VtlData*)pde->vtl)->pdot && ((VtlData*)pde->vtl)->ry == 8 && pde->g.z_lo_phys && pde->g.z_hi_phys;
}

static int vtl_launch(beat_pde* pde, const VtlPass& ps) {
  const bool bv = ps.kind == VtlPass::BV, res = ps.kind == VtlPass::RES, pdot = ps.kind == VtlPass::PDOT;
  VtlData* d = (VtlData*)pde->vtl;
  const Geom& f = pde->g;
  VtlArgs a{};
  a.ld = pde->v_ld;
  a.nx = f.nx;
  a.ny = f.ny;
  a.nz = f.nz;
  a.plane = f.plane;
  a.nsegx = d->nsegx;
  a.nzp = d->nzp;
  a.partials = pde->ctx->d_partials;
  const int count = d->list_count[ps.list];
  const int reduce_count = ps.reduce == VtlPass::BOTH_PARTS ? d->list_count[1] + d->list_count[2] : count;
  if (count == 0) {  // (a split launch without tiles: only the reduction over what the other part wrote)
    return ps.reduce != VtlPass::NO_SUM ? beat_pde_launch_reduce(pde, reduce_count, 1, ps.st + PQ, ps.st) : BEAT_OK;
  }
  a.part_off = ps.part_off - d->list_base[ps.list];  // the kernel indexes its partial by the tile's position in the whole array
  a.st = ps.st;
  // blocks in eights (one per XCD), at most the resident number, at least one tile per block on average
  const unsigned grid = std::max(8u, std::min(d->resident, (unsigned)((count + 7) & ~7)));
  a.x = res ? ps.e : ps.p;  // (RES forms its window from v_ and e: nullptr = no guess on record)
  a.y = ps.q;
  a.rows = bv ? pde->v_B : pde->v_A;
  a.ignore_stop = bv || res;
  if (bv) {
    a.dt = pde->dt;
    beat_fill_stimuli(a, ps.stim_w, ps.stim_amp, ps.n_stim);
  }
  a.t = ps.t;
  a.mask = d->d_mask;
  a.items = d->d_items;
  a.xcd_first = d->d_xcd_first + 9 * ps.list;
  a.next = d->d_xcd_first + 27;
  a.r = res ? ps.p : ps.r;
  a.pnew = ps.p_new;
  a.first = ps.first ? 1 : 0;
  if (pdot && pde->v_gc0 != nullptr) {  // a slab with live neighbours: the direction is formed and kept on the ghost planes too
    a.gc0_lo = f.z_lo_phys ? nullptr : pde->v_gc0;
    a.gc0_hi = f.z_hi_phys ? nullptr : pde->v_gc0 + f.plane;
    if (a.gc0_lo != nullptr) a.first |= 2;
  }
  auto launch = [&](auto kernel, int ry) { BEAT_KERNEL(kernel, dim3(grid), dim3(ry * 64), 0, pde->ctx->stream, a); };
  if (bv) {
    launch(vtl_spmv_kernel<8, false, 2>, 8);
  } else if (res) {
    launch(vtl_spmv_kernel<8, false, 4>, 8);
  } else if (pdot) {  // (tiles dealt round-robin: the counter of BEAT_VTL_DYNAMIC serves the plain SpMV only)
    (a.gc0_lo != nullptr || a.gc0_hi != nullptr) ? launch(vtl_spmv_kernel<8, false, 3>, 8) : launch(vtl_spmv_kernel<8, false, 1>, 8);
  } else if (d->ry == 8) {
    d->dyn ? launch(vtl_spmv_kernel<8, true, 0>, 8) : launch(vtl_spmv_kernel<8, false, 0>, 8);
  } else {
    d->dyn ? launch(vtl_spmv_kernel<4, true, 0>, 4) : launch(vtl_spmv_kernel<4, false, 0>, 4);
  }
  BEAT_LAUNCH_CHECK();
  if (ps.reduce == VtlPass::NO_SUM) return BEAT_OK;
  if (res) return beat_pde_launch_reduce(pde, count, 3, ps.red_out, nullptr, ScalarStep::begin(ps.red_out, ps.start));
  return beat_pde_launch_reduce(pde, reduce_count, 1, ps.st + PQ, ps.st);
}

// The right-hand side of a step on the tiles (what beat_var_rhs computes with gathers: 352 B/node from beyond the L2 on the 401^3
// shell against 168 algorithmic, 1.30 ms, profiles/r04_shell400.md), in the formulation of the constant-coefficient kernels
// (beat_pde_rr.hip):
//   pass 1 (BV):  b = B v_ + dt sum_k amp_k w_k  -- the plain tile product over the rows of B = C_m Mass - (1 - theta) dt K, which
//                 beat_var_form_A forms beside A (beat_pde::v_B) --, b stored in a work field, per-tile partials of b.b;
//   pass 2 (RES): r = b - A x0 with x0 = v_ + e formed while loading (ONE vector window, as the iteration's fused pass forms its
//                 direction), z = D^-1 r where the three-kernel iteration wants it; per-tile partials of r.z and r.r.
// Two passes at the plain product's cost and register budget (4 waves per SIMD) instead of one pass with two windows at 166 VGPRs.
// r differs from var_rhs_kernel's  dt (stim - K v_) - A e  by rounding (~1e-16 |b|: far below any threshold rtol |b|): the solves
// are the same solves, not the same bits (tests/test_var_gpu.py).  Single slabs, tiles of 8 rows.  dev_t: a work field (the
// solver's q, free until the first iteration).
bool beat_vtl_rhs_available(const beat_pde* pde) {
  if (!(beat_vtl_available(pde) && pde->g.z_lo_phys && pde->g.z_hi_phys)) return false;
  const VtlData* d = (const VtlData*)pde->vtl;
  return d->ry == 8 && d->rhs && pde->v_B != nullptr;
}
bool beat_vtl_rhs_wanted(const beat_pde* pde) {  // (before the rows of B exist: beat_var_form_A allocates them when this says so)
  if (!(beat_vtl_available(pde) && pde->g.z_lo_phys && pde->g.z_hi_phys)) return false;
  const VtlData* d = (const VtlData*)pde->vtl;
  return d->ry == 8 && d->rhs;
}

int beat_vtl_rhs(beat_pde* pde, const double* dev_v_prev, const double* const* host_dev_stim_w, const double* host_stim_amp, int n_stim,
                 double* dev_x, double* dev_r, double* dev_p, double* dev_t, double* dev_red, const double* dev_e, const PcgStart* start) {
  if (dev_x != dev_v_prev)  // nodes outside the tissue keep their value: copy everything first (as beat_var_rhs does)
    BEAT_HIP_CHECK(hipMemcpyAsync(dev_x, dev_v_prev, sizeof(double) * (size_t)pde->n, hipMemcpyDeviceToDevice, pde->ctx->stream));
  VtlPass bv;
  bv.kind = VtlPass::BV;
  bv.reduce = VtlPass::NO_SUM;  // (its partials of b.b are summed behind the second pass)
  bv.st = pde->d_st;
  bv.p = dev_v_prev;
  bv.q = dev_t;
  bv.stim_w = host_dev_stim_w;
  bv.stim_amp = host_stim_amp;
  bv.n_stim = n_stim;
  if (int rc = vtl_launch(pde, bv)) return rc;
  VtlPass res;
  res.kind = VtlPass::RES;
  res.st = pde->d_st;
  res.p = dev_v_prev;
  res.e = dev_e;
  res.t = dev_t;
  res.q = dev_r;
  // (z: only the three-kernel iteration reads it -- the fused pass forms its first direction from r itself)
  res.p_new = beat_vtl_pdot_available(pde) ? nullptr : dev_p;
  res.red_out = dev_red;
  res.start = start;
  return vtl_launch(pde, res);
}

// The fused pass on a slab with live neighbours, in the two parts of the split launches: part 0 = the planes whose stencil
// needs no ghost plane (enqueue it while the ghost planes of r travel), part 1 = the one or two slab-boundary planes -- which also
// form and keep the direction on the ghost planes next to them, from the exchanged r, the direction kept there by the previous
// iteration and the neighbours' centre coefficients (beat_pde::v_gc0) -- and the sum over both parts' tiles.  p is never exchanged.
bool beat_vtl_pdot_dist_available(const beat_pde* pde) {
  if (!(beat_vtl_available(pde) && beat_vtl_parts_available(pde)) || (pde->g.z_lo_phys && pde->g.z_hi_phys)) return false;
  const VtlData* d = (const VtlData*)pde->vtl;
  static const bool on = [] {  // BEAT_VTL_PDOT_DIST=0: the three-kernel iteration with an exchange of p (A/B runs)
    const char* e = std::getenv("BEAT_VTL_PDOT_DIST");
    return !(e && e[0] == '0');
  }();
  return on && d->pdot && d->ry == 8 && pde->v_gc0 != nullptr;
}

int beat_vtl_pdot_part(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new, double* dev_q,
                       int first, int part) {
  BEAT_REQUIRE(dev_p_old != dev_p_new, "the direction update is out of place");
  VtlPass ps;
  ps.kind = VtlPass::PDOT;
  ps.st = dev_st;
  ps.p = dev_p_old;
  ps.r = dev_r;
  ps.p_new = dev_p_new;
  ps.q = dev_q;
  ps.first = first != 0;
  vtl_set_part(pde, ps, part);
  return vtl_launch(pde, ps);
}

// the split launches of a decomposed grid: part 0 = the planes that need no ghost plane of p (no reduction), part 1 = the
// slab-boundary planes + the sum over both parts' tiles
bool beat_vtl_parts_available(const beat_pde* pde) {
  if (!(pde->var && pde->vtl != nullptr)) return false;
  const VtlData* d = (const VtlData*)pde->vtl;
  return d->list_count[1] + d->list_count[2] > 0;
}

int beat_vtl_spmv_dot_part(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st, int part) {
  VtlPass ps;
  ps.st = dev_st;
  ps.p = dev_p;
  ps.q = dev_q;
  vtl_set_part(pde, ps, part);
  return vtl_launch(pde, ps);
}
