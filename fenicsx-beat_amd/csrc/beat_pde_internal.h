// Internal declarations shared by the two translation units of the diffusion step:
//   beat_pde.hip      constant-coefficient (27 node types) stencil kernels, PCG kernels, the C ABI
//   beat_pde_var.hip  per-node-coefficient operators, device-side row assembly, Dirichlet elimination
#pragma once
#include "beat_common.h"
#include "beat_pcg_scalar.h"
#include "beat_slab_parts.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace beat_pde_detail {

// (the slots of the PCG scalar state `st` and BEAT_ST_DOUBLES: beat_pcg_scalar.h)
constexpr int PRING = 6;  // search directions kept by the deferred-x PCG before x must be brought up to date (default ring)
// Per-node-row operators on a single slab keep PRING_MAX directions (beat_pde::ring): their solves take 9 - 12 iterations at the
// reference's dt (profiles/r05_shell_guess.md), and with a ring of 6 every one of them paid an in-loop flush -- x and the guess's
// fields read and written a second time, 48 B/node per step.  Kernels size their arrays by PRING_MAX and take the ring as an argument.
constexpr int PRING_MAX = 12;
constexpr int TABW = 16;  // padded row width of the device coefficient tables

extern const int kOffsets[45];  // (dx, dy, dz) of the 15 stencil points

struct Geom {
  int nx, ny, nz;
  int64_t plane;
  int tiles_x, tiles_y, nchunks, zc, total;
  int z_lo_phys, z_hi_phys;
  int tile_tx;  // 64, 128 or 256: which Tile<> instantiation the grid was sized for
  int z_lo, z_hi;    // planes [z_lo, z_hi) computed by this launch (whole slab: 0, nz)
  int part_off;      // first block-partial slot this launch writes
};

enum { MODE_APPLY = 0, MODE_SPMV_DOT = 1, MODE_RHS = 2, MODE_PC = 3 };

// The loops of a multi-launch solve (beat_pde::OpenSolve::kind): each is one body of the iterations beat_pde.hip enqueues
enum SolveKind {
  SOLVE_RR = 0,  // register-row kernels, constant coefficients: the loop that never stores q = A p
  SOLVE_ROWS,    // per-node rows (OpenSolve::pdot: the fused tile pass)
  SOLVE_TILED,   // the LDS-tiled constant-coefficient kernels (more blocks than BEAT_MAX_PARTIALS, or BEAT_RR=0)
  SOLVE_POLY,    // the polynomial preconditioner: classic in-place recurrences, x updated as it goes, no ring
  SOLVE_DIST     // a decomposed solve (beat_dist.hip; OpenSolve::rr / merged / vpdot say which of its loops runs)
};

// The passes that run in the two parts of beat_slab_parts.h (beat_pde::Part0::pass: which of them wrote part 0's block partials)
enum PartPass { PASS_NONE = 0, PASS_SPMV, PASS_RR_RHS, PASS_RR_PDOT, PASS_RR_UDOT, PASS_VAR_RHS, PASS_VAR_SPMV, PASS_VRR_SPMV };

}  // namespace beat_pde_detail

struct beat_pde {
  beat_ctx* ctx = nullptr;
  beat_pde_detail::Geom g{};
  int64_t n = 0;
  double h_mass[27 * 15], h_stiff[27 * 15];
  double h_A[27 * 15], h_B[27 * 15], h_dinv[27];
  bool have_dt = false;
  double C_m = 1.0, theta = 0.5, dt = 0.0;
  // device: 4 padded tables (A, B, Mass, K), then dinv[32]
  double* d_tabs = nullptr;
  double* d_st = nullptr;  // BEAT_ST_DOUBLES doubles, PCG scalar state of beat_pde_solve (the host reads the first 16)
  int last_iters = -1;
  int z_last_iters = -1;  // iterations of the last shifted solve (beat_pde_zsolve: its first chunk of enqueued iterations)
  unsigned vec_grid = 1;
  double* d_alphas = nullptr;  // PRING_MAX step lengths of the deferred-x PCG
  // A solve that has been ENQUEUED and not yet looked at by the host (beat_solve_open / beat_solve_end, round 5): right-hand side, the
  // iterations the previous solve needed + 1 and the copy of the scalar state are in the stream, `ev_st` marks the copy.  The next
  // ionic launch may be enqueued behind it before the host waits (PendingV::dev_st): the device does not idle while the host wakes up.
  // Every multi-launch solve goes through this state; only the register-row and per-node-row ones may be left open by a caller.
  struct OpenSolve {
    bool on = false;
    int kind = beat_pde_detail::SOLVE_RR;
    bool pdot = false;
    double* x = nullptr;
    double* work = nullptr;
    int max_it = 0, launched = 0;
    int limit = 0;  // iterations that may be enqueued: max_it (+ 1 merged: the pass that finds r_k converged is one more than the k updates)
    // a decomposed solve (beat_dist.hip: beat_dist_solve_begin): its communicator and which of its loops runs
    void* comm = nullptr;
    bool rr = false, merged = false, vpdot = false;
  } open;
  // part 0 of a pass in two parts (beat_launch_parts): the block partials it wrote, for the part 1 of the same pass that follows it
  struct Part0 {
    int pass = beat_pde_detail::PASS_NONE;
    int blocks = 0;
  } part0;
  double* h_st = nullptr;       // pinned copy of the scalar state of the open solve (16 doubles)
  hipEvent_t ev_st = nullptr;   // recorded behind that copy
  beat_ksp_info last_info{};    // of the last solve that was finished
  int last_rc = 0;
  int ring = beat_pde_detail::PRING;  // search directions kept before x is brought up to date (6; 12: per-node rows on a single slab)
  int last_base = 0;                  // first iteration of the ring cycle the last deferring solve left pending
  // the register-row loop tests convergence from a prediction of r_{i+1} . r_{i+1} behind PDOT and skips the residual update when
  // that settles it (beat_pcg_predict; BEAT_PCG_PREDICT_STOP=0 when the operator is created: the explicit test only)
  bool predict_stop = true;
  double predict_c = 0.0;  // its error-bound constant (beat_rr_predict_bound), computed on first use
  double* d_batch_st = nullptr;  // scalar states of the solves of a beat_split_steps batch (BEAT_MAX_BATCH x 16)
  // z node type of the ghost planes (the neighbouring slabs' boundary planes): 1 unless that plane is a face of the
  // whole grid (a neighbour that owns a single plane); set with beat_pde_set_ghost_types
  int ghost_lo_tz = 1, ghost_hi_tz = 1;
  int single_reduction = -1;               // decomposed solve: 1 one all-reduce per iteration, 0 two, -1 as BEAT_DIST_MERGED says
  beat_guess_state guess;                  // the extrapolated initial guess: order, history fields, terms of the solve in progress (beat_guess.h)
  void* vrr = nullptr;      // work lists of the z-marching per-node SpMV (beat_pde_vrr.hip), or nullptr
  void* vtl = nullptr;      // tiles and lane masks of the workgroup-tile per-node SpMV (beat_pde_vtl.hip), or nullptr
  bool small_enabled = true;  // grids of a few thousand nodes: whole solve in one launch (beat_pde_small.hip)
  int pc_ncoef = 1;       // 1: Jacobi; m >= 2: Chebyshev polynomial of degree m-1 in D^-1 A (m-1 stencil passes)
  double pc_coef[8] = {1.0};
  // variable-coefficient mode (beat_pde_create_var): caller-owned Mass / K rows, A and 1/diag owned here
  bool var = false;
  const double* v_mass = nullptr;
  const double* v_stiff = nullptr;
  double* v_A = nullptr;
  double* v_dinv = nullptr;
  double* v_B = nullptr;  // rows of B = C_m Mass - (1 - theta) dt K, formed beside A when the right-hand side runs on the tiles (beat_vtl_rhs)
  // a slab with live neighbours: the centre coefficients of the neighbours' boundary planes ([0, plane): below, [plane, 2 plane):
  // above), exchanged by beat_pde_solve_dist when v_gc0_valid is false (the operator changed) -- what the fused tile pass needs to
  // form the search direction on the ghost planes (beat_vtl_pdot_part)
  double* v_gc0 = nullptr;
  bool v_gc0_valid = false;
  bool v_pdot_dist = false;  // all ranks of the decomposition can run the fused tile pass (agreed when v_gc0 is refreshed)
  int64_t v_ld = 0;
  int* v_seg = nullptr;        // device: indices of the 64-node segments that hold tissue nodes (ascending)
  std::vector<int> h_seg;      // host copy (sub-ranges are located by binary search)
  unsigned long long* v_segmask = nullptr;  // device: per list entry, bit l set = node 64 seg + l is a tissue node
  int* v_seg_tiled = nullptr;               // the same list (and masks) ordered by tiles of T rows x T planes (BEAT_VAR_TILE, experiments)
  unsigned long long* v_segmask_tiled = nullptr;
  const double* d_tab(int which) const { return d_tabs + (size_t)which * 27 * beat_pde_detail::TABW; }
  const double* d_dinv() const { return d_tabs + (size_t)4 * 27 * beat_pde_detail::TABW; }
  const double* dinv_arg() const { return var ? v_dinv : d_dinv(); }
};

// The PCG's work area (beat_pde_work_fields fields, beat_pde_field_stride doubles apart): [ghost plane | r | q | z | ring[0..]].
// Each field sits behind its lower ghost plane, which the stencil kernels read (a decomposed grid: the neighbour's boundary plane)
// like the upper one behind it; z is only touched by the polynomial preconditioner; ring[j] = ring + j * fld.  (HipOps in
// beat/_engine.py mirrors this layout.)
struct PcgWork {
  double *r, *q, *z, *ring;
  int64_t fld;
};
inline PcgWork beat_pcg_work(const beat_pde* pde, double* work) {
  const int64_t fld = beat_pde_field_stride(pde);
  double* r = work + pde->g.plane;
  return {r, r + fld, r + 2 * fld, r + 3 * fld, fld};
}

// Iterations enqueued before the host first looks at the convergence latch: the previous solve's count plus one.  A
// latched iteration costs four empty launches (~20 us); one short costs a host round trip with the GPU idle plus a
// second one after the catch-up iterations, and consecutive time steps differ by one iteration all the time.
inline int beat_pde_first_chunk(const beat_pde* pde) {
  static const int extra = [] {
    const char* e = std::getenv("BEAT_CHUNK_EXTRA");
    return e ? std::max(0, std::atoi(e)) : 1;
  }();
  return pde->last_iters >= 0 ? std::max(1, pde->last_iters + extra) : 8;
}

// What a solve starts with (beat_pcg_begin's arguments).  A right-hand side that is given one runs the start in the launch that sums its
// partials; nullptr: the caller starts the solve itself (a decomposed solve: the all-reduce sits between the sums and the start)
struct PcgStart {
  double rtol, atol;
  int max_it;
};

// One scalar step of the PCG (beat_pcg_step in beat_pcg_scalar.h) on the state `st`: behind a reduction's sums, in the same launch
// (BEAT_PCG_FUSE=0: in a launch of its own behind it), or in a launch of its own (beat_pcg_launch_step: the stage API, and a decomposed
// solve between its all-reduce and the next pass)
struct ScalarStep {
  beat_pde_detail::PcgStep kind = beat_pde_detail::STEP_NONE;
  double* st = nullptr;       // the scalar state the step works on (behind a reduction: the one the sums were just written into)
  double* counter = nullptr;  // behind a reduction, any kind: counts the executed residual update (st + NUPD) when it is not latched
  double rtol = 0.0, atol = 0.0;  // STEP_BEGIN: the start of a solve
  int max_it = 0;
  double* alpha_slot = nullptr;  // STEP_PREDICT, STEP_MERGED: the ring slot's step length (d_alphas + slot)
  double bound_c = 0.0;          // STEP_PREDICT: beat_rr_predict_bound
  // behind a deferred-x residual update: counts it and, with `roll`, rolls the iteration (beta, iteration count, latch)
  static ScalarStep after_update(double* st, bool roll) {
    return {roll ? beat_pde_detail::STEP_ROLL : beat_pde_detail::STEP_NONE, st, st + beat_pde_detail::NUPD};
  }
  static ScalarStep roll(double* st) { return {beat_pde_detail::STEP_ROLL, st}; }
  static ScalarStep begin(double* st, const PcgStart* s) {
    return s ? ScalarStep{beat_pde_detail::STEP_BEGIN, st, nullptr, s->rtol, s->atol, s->max_it} : ScalarStep{};
  }
  static ScalarStep with_slot(beat_pde_detail::PcgStep kind, double* st, double* alpha_slot, double bound_c = 0.0) {
    return {kind, st, nullptr, 0.0, 0.0, 0, alpha_slot, bound_c};
  }
};
// fixed-order sum of `count` block partials of `nsum` quantities into out[0..nsum), skipped when st[STOP] is set (st may be nullptr);
// then `step` (beat_pde.hip)
int beat_pde_launch_reduce(beat_pde* pde, int count, int nsum, double* out, const double* st, const ScalarStep& step = {});
int beat_pcg_launch_step(beat_pde* pde, const ScalarStep& step);  // `step` alone, one thread

// The hand-off between the two parts of a pass: part 0 puts its block count under the pass's name, the part 1 that follows takes it
// (once) and must be of the same pass
inline void beat_part0_put(beat_pde* pde, int pass, int blocks) { pde->part0 = {pass, blocks}; }
inline int beat_part0_take(beat_pde* pde, int pass, int* blocks) {
  BEAT_REQUIRE(pde->part0.pass == pass, "part 1 of a pass must follow part 0 of the same pass");
  *blocks = pde->part0.blocks;
  pde->part0 = {};
  return BEAT_OK;
}

// a device array with a copy of `host` (one element where `host` is empty: never a null pointer)
template <class T>
hipError_t beat_upload(T** dev, const std::vector<T>& host) {
  hipError_t e = hipMalloc(dev, sizeof(T) * std::max<size_t>(1, host.size()));
  if (e == hipSuccess && !host.empty()) e = hipMemcpy(*dev, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice);
  return e;
}

// The workgroups of `block` threads of `kernel` the chip holds at once (occupancy x CUs); `on_failure` where it cannot be asked.  Grid-
// stride and list-walking kernels are launched with at most this many; each caller adds its own cap and rounding.  A failure of any
// one of the three queries gives `on_failure` as a whole: no product of one answer with a guess at the other (an assumed CU count
// times the occupancy found, or the CUs found times one block).
template <class Kernel>
unsigned beat_resident_blocks(Kernel kernel, int block, unsigned on_failure) {
  int per_cu = 0, cus = 0, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 || cus < 1)
    return on_failure;
  return (unsigned)(per_cu * cus);
}

inline beat_pde_detail::SlabPart beat_slab_part(const beat_pde* pde, int part) {
  return beat_pde_detail::beat_slab_part(pde->g.nz, pde->g.z_lo_phys != 0, pde->g.z_hi_phys != 0, part);
}

// A pass in the parts of beat_slab_parts.h.  launch(z_lo, z_hi, part_off) enqueues the pass on planes [z_lo, z_hi) with its block
// partials from slot part_off on and returns how many it writes.  Part 0 leaves its count in pde->part0 under the pass's name; part 1
// must follow the part 0 of the same pass and continues from that count: the slots are interior, lower plane, upper plane, the order
// the fixed-order sums have always had.  *reduce_count = the partials to sum (parts -1 and 1; part 0 sums nothing: 0).
template <class Launch>
int beat_launch_parts(beat_pde* pde, int pass, int part, Launch&& launch, int* reduce_count) {
  const beat_pde_detail::SlabPart sp = beat_slab_part(pde, part);
  int off = 0;
  if (part == 1)
    if (int rc = beat_part0_take(pde, pass, &off)) return rc;
  for (int k = 0; k < sp.count; ++k) off += launch(sp.range[k].z_lo, sp.range[k].z_hi, off);
  BEAT_LAUNCH_CHECK();
  if (part == 0) beat_part0_put(pde, pass, off);
  BEAT_REQUIRE(off <= BEAT_MAX_PARTIALS, "too many block partials");
  *reduce_count = part == 0 ? 0 : off;
  return BEAT_OK;
}

// the stimuli a right-hand side adds: those with a weight field and a non-zero amplitude, in the caller's order
template <class Args>
void beat_fill_stimuli(Args& a, const double* const* host_dev_stim_w, const double* host_stim_amp, int n_stim) {
  a.nstim = 0;
  for (int k = 0; k < n_stim; ++k) {
    if (host_dev_stim_w[k] == nullptr || host_stim_amp[k] == 0.0) continue;
    a.w[a.nstim] = host_dev_stim_w[k];
    a.amp[a.nstim] = host_stim_amp[k];
    ++a.nstim;
  }
}

// per-node-coefficient variants of the stage operations (beat_pde_var.hip); same contracts as the beat_pde_*
// entry points that dispatch to them
int beat_var_form_A(beat_pde* pde);
int beat_var_apply(beat_pde* pde, int which, const double* dev_x, double* dev_y);
int beat_var_rhs(beat_pde* pde, const double* dev_v_prev, const double* const* host_dev_stim_w,
                 const double* host_stim_amp, int n_stim, double* dev_x, double* dev_r, double* dev_p, double* dev_red,
                 const double* dev_e = nullptr,  // dev_e: initial-guess increment (r = b - A (v_ + e)) or nullptr
                 int part = -1);  // decomposed grids: 0 = the planes that need no ghost data, 1 = the boundary planes + the sums; -1: all
int beat_var_spmv_dot(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st);
int beat_var_spmv_dot_part(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st, int part);
int beat_var_update_r(beat_pde* pde, double* dev_st, double* dev_r, const double* dev_q, int slot, bool roll = false);
int beat_var_pupdate_oop(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_cur, double* dev_p_next);
int beat_var_flush(beat_pde* pde, const double* dev_st, double* dev_x, const double* dev_ring0, int64_t field_stride,
                   int ring_base, int only_if_full, const beat_pde_detail::GuessTerms& gt);

// the x update of a deferred-x solve with the guess's terms for that ring cycle (beat_guess_state::terms, take_pending)
int beat_pde_x_flush_terms(beat_pde* pde, const double* dev_st, double* dev_x, const double* dev_ring0, int64_t field_stride,
                           int ring_base, int only_if_full, const beat_pde_detail::GuessTerms& gt);
// behind iteration i of the open solve's deferred-x loop: the x update above when that iteration filled the ring, else nothing
int beat_flush_if_ring_full(beat_pde* pde, int i);

// per-node-coefficient SpMV that marches along z and loads only the forward half of each row (beat_pde_vrr.hip)
int beat_vrr_setup(beat_pde* pde, const std::vector<unsigned long long>& host_tissue_flags);
void beat_vrr_destroy(beat_pde* pde);
bool beat_vrr_available(const beat_pde* pde);
int beat_vrr_spmv_dot(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st, int part);

// per-node-coefficient SpMV on workgroup tiles: forward coefficients and rows of p loaded once per tile, shared through
// LDS and registers (beat_pde_vtl.hip); whole-slab launches only
int beat_vtl_setup(beat_pde* pde, const std::vector<unsigned long long>& host_tissue_flags);
void beat_vtl_destroy(beat_pde* pde);
bool beat_vtl_available(const beat_pde* pde);
int beat_vtl_spmv_dot(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st);
bool beat_vtl_parts_available(const beat_pde* pde);
bool beat_vtl_pdot_dist_available(const beat_pde* pde);
int beat_vtl_pdot_part(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new, double* dev_q,
                       int first, int part);
int beat_vtl_spmv_dot_part(beat_pde* pde, const double* dev_p, double* dev_q, double* dev_st, int part);
bool beat_vtl_pdot_available(const beat_pde* pde);
bool beat_vtl_rhs_available(const beat_pde* pde);
bool beat_vtl_rhs_wanted(const beat_pde* pde);
int beat_vtl_rhs(beat_pde* pde, const double* dev_v_prev, const double* const* host_dev_stim_w, const double* host_stim_amp, int n_stim,
                 double* dev_x, double* dev_r, double* dev_p, double* dev_t, double* dev_red, const double* dev_e, const PcgStart* start);
int beat_vtl_pdot(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new, double* dev_q, int first);

// The multi-launch solves in two halves.  beat_solve_open (beat_pde.hip), called by a begin once its right-hand side and start are
// enqueued: pde->open = `o` (limit set from o.max_it), the first chunk of iterations and the copy of the scalar state for the first
// look.  beat_solve_end: wait for that look, enqueue more iterations if the residual asks for them, do the host's bookkeeping;
// *needed_more = the first look found the solve unlatched (a launch enqueued behind it with PendingV::dev_st has done nothing); a
// solve that was never opened: the last finished solve's record
bool beat_solve_lazy_available(const beat_pde* pde);
int beat_solve_open(beat_pde* pde, beat_pde::OpenSolve o);
int beat_solve_end(beat_pde* pde, int defer_flush, beat_ksp_info* info, int* host_pending, bool* needed_more);
// the record of a solve from its scalar state h (16 doubles); BEAT_ENOTCONV with the error set when it did not converge (batch_step
// >= 0: the solve of that step of a beat_split_steps batch)
beat_ksp_info beat_pcg_info(const double* h);
int beat_pcg_check(const beat_ksp_info& info, int batch_step = -1);
// the decomposed solve's part of the above (beat_dist.hip): its begin, iterations [open.launched, + count) with their exchanges and
// all-reduces, the error of a peer after each look (ipc transport), the exchange left in flight by the last residual update
struct beat_comm;
int beat_dist_solve_begin(beat_pde* pde, beat_comm* comm, const double* dev_v_prev, const double* const* host_dev_stim_w,
                          const double* host_stim_amp, int n_stim, double* dev_x, double* dev_work, double rtol, double atol, int max_it);
int beat_dist_enqueue_iterations(beat_pde* pde, int count);
int beat_dist_check(beat_pde* pde);
int beat_dist_drain(beat_pde* pde);

// one-workgroup solve of small constant-coefficient grids (beat_pde_small.hip)
bool beat_small_available(const beat_pde* pde);
int beat_small_launch(beat_pde* pde, const double* dev_v_prev, const double* const* host_dev_stim_w,
                      const double* host_stim_amp, int n_stim, double* dev_x, double rtol, double atol, int max_it,
                      double* dev_st);
int beat_small_solve(beat_pde* pde, const double* dev_v_prev, const double* const* host_dev_stim_w,
                     const double* host_stim_amp, int n_stim, double* dev_x, double rtol, double atol, int max_it,
                     beat_ksp_info* info);

// register-row kernels of the constant-coefficient Jacobi-PCG that never stores q = A p (beat_pde_rr.hip)
bool beat_rr_available(const beat_pde* pde);
int beat_rr_rhs(beat_pde* pde, const double* dev_v_prev, const double* const* host_dev_stim_w, const double* host_stim_amp,
                int n_stim, double* dev_x, double* dev_r, double* dev_st, int part = -1,  // part: as beat_var_rhs
                const PcgStart* start = nullptr);  // part -1 only: the start of the solve behind the sums
// slot >= 0: the single-slab loop's pass, which predicts the stop when the operator was created with it on (see beat_rr_pdot_part)
int beat_rr_pdot(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new, int slot = -1);
int beat_rr_pdot_part(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new,
                      int part, int slot = -1);
double beat_rr_predict_bound(const beat_pde* pde);
int beat_rr_rupd(beat_pde* pde, double* dev_st, const double* dev_r, double* dev_r_new, const double* dev_p, int slot,
                 bool roll = true);
// the single-reduction (Chronopoulos-Gear) iteration of a decomposed solve: see beat_pde_rr.hip
int beat_rr_udot_part(beat_pde* pde, double* dev_st, const double* dev_r, int part);
int beat_rr_prupd(beat_pde* pde, double* dev_st, const double* dev_r, const double* dev_p_old, double* dev_p_new,
                  double* dev_r_new);
