// Per-node event maps of the potential, kept on the device: time of the first and of the last upstroke through a threshold, time of
// the repolarisation behind it, their difference (APD), the maximal upstroke velocity and the maximal potential.  The reference's
// tissue demos build the first of these on the host from the whole potential after every step
//   demos/irksome_model_gotranx.py:251-254   crossed = (v_arr >= activation_threshold) & (tact_arr < 0.0); tact_arr[crossed] = t
//   demos/niederer_benchmark.py:285-287      the same rule with > 0.0 at probe points
// which here would cost a flush of the deferred update, a device-to-host copy of the field and a synchronisation per step.
//
// The kernel (beat_events_kernel.h).  One pass, one double per lane: a wavefront walks over 512-byte pieces of the potential that are aligned in memory (the first piece
// starts up to 63 nodes before the field and masks those lanes), every stream is read once, the maps are stored on events only.
// Loads and stores are plain ones.  That is a choice still to be measured, not a result: the potential was written by the launch before
// this one and the next launch reads it again, and the maps are read again a step later, which speaks for keeping them cacheable; the
// pending directions and the guess's fields in the fused flush are read once and not again before they are overwritten, the ionic kernel
// loads the same ring non-temporally, and they are the first candidates for a non-temporal load when this pass is profiled.
// No atomics, no LDS.  Null map pointers choose a template instance (v_prev, the flush) or a branch that is uniform over the launch.
//
// FLUSH: the pass also IS the deferred update of the potential (beat_pde_x_flush with only_if_full = 0), in x_flush_kernel's
// expressions and order (beat_pde.hip; as ionic_models.h does for the update an ionic kernel applies): 1 its plain branch, 2 the
// branch that records the initial guess's increment.
#include "beat_events_kernel.h"

namespace {

using namespace beat_pde_detail;
using namespace beat_events_detail;

// what both entry points ask of the maps; nothing has been enqueued when this refuses
int check_maps(const beat_event_maps* m, double t0, double t1) {
  BEAT_REQUIRE(m != nullptr, "null beat_event_maps");
  BEAT_REQUIRE(m->mode == 0 || m->mode == 1, "mode must be 0 (step) or 1 (linear), got %d", m->mode);
  BEAT_REQUIRE(m->strict == 0 || m->strict == 1, "strict must be 0 (>=) or 1 (>), got %d", m->strict);
  BEAT_REQUIRE(m->thr_up == m->thr_up, "thr_up is NaN");
  BEAT_REQUIRE(t1 > t0, "a step (t0, t1) with t1 > t0 expected");
  const bool down = m->repol != nullptr || m->apd != nullptr;
  BEAT_REQUIRE(!down || m->act_last != nullptr, "repol / apd need act_last (the activation a repolarisation belongs to)");
  BEAT_REQUIRE(!down || m->thr_down == m->thr_down, "thr_down is NaN");
  const bool needs_vp = m->act_last != nullptr || down || m->dvdt_max != nullptr || (m->mode == 1 && m->act_first != nullptr);
  BEAT_REQUIRE(!needs_vp || m->v_prev != nullptr, "act_last, repol, apd, dvdt_max and the linear mode need v_prev");
  return BEAT_OK;
}

template <int FLUSH>
int launch_events(beat_ctx* ctx, double* dev_v, int64_t n, const beat_event_maps& m, double t0, double t1, const FlushArgs& fa) {
  const int shift = (int)(((uintptr_t)dev_v >> 3) & 63);  // nodes between the 512-byte boundary below the field and its first node
  const int64_t npieces = (n + shift + 63) >> 6;
  const unsigned grid = (unsigned)std::min<int64_t>(4096, (npieces + BEAT_BLOCK / 64 - 1) / (BEAT_BLOCK / 64));
  if (m.v_prev != nullptr)
    BEAT_KERNEL((events_kernel<FLUSH, true>), dim3(grid), dim3(BEAT_BLOCK), 0, ctx->stream, n, shift, dev_v, m, t0, t1, fa);
  else
    BEAT_KERNEL((events_kernel<FLUSH, false>), dim3(grid), dim3(BEAT_BLOCK), 0, ctx->stream, n, shift, dev_v, m, t0, t1, fa);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}

}  // namespace

// The pass on a potential that is up to date (demos/irksome_model_gotranx.py:251-254, demos/niederer_benchmark.py:285-287)
extern "C" int beat_field_events(beat_ctx* ctx, const double* dev_v, int64_t n, const beat_event_maps* maps, double t0, double t1) {
  BEAT_REQUIRE(ctx != nullptr && dev_v != nullptr, "null argument");
  BEAT_REQUIRE(n > 0, "n must be positive");
  BEAT_REQUIRE(((uintptr_t)dev_v & 7) == 0, "dev_v is not 8-byte aligned");
  if (int rc = check_maps(maps, t0, t1)) return rc;
  return launch_events<0>(ctx, const_cast<double*>(dev_v), n, *maps, t0, t1, FlushArgs{});
}

// beat_pde_x_flush(only_if_full = 0) and that pass as one pass over x (the same reference lines: the host loop reads the potential
// the solve has just completed, src/beat/base_model.py:236)
extern "C" int beat_pde_x_flush_events(beat_pde* pde, const double* dev_st, double* dev_x, const double* dev_ring0, int64_t field_stride,
                                       int ring_base, const beat_event_maps* maps, double t0, double t1) {
  BEAT_REQUIRE(pde != nullptr && dev_x != nullptr && dev_ring0 != nullptr, "null argument");
  BEAT_REQUIRE(((uintptr_t)dev_x & 7) == 0, "dev_x is not 8-byte aligned");
  BEAT_REQUIRE(!pde->open.on, "the operator has an open solve: finish it first (beat_pde_solve_end)");
  if (int rc = check_maps(maps, t0, t1)) return rc;
  if (pde->var) {  // per-node rows: their flush works on a list of segments; two passes
    if (int rc = beat_pde_x_flush(pde, dev_st, dev_x, dev_ring0, field_stride, ring_base, 0)) return rc;
    return launch_events<0>(pde->ctx, dev_x, pde->n, *maps, t0, t1, FlushArgs{});
  }
  FlushArgs fa;
  fa.st = dev_st != nullptr ? dev_st : pde->d_st;  // the scalar state of beat_pde_solve[_ex]
  fa.ring = dev_ring0;
  fa.fld = field_stride;
  fa.alphas = pde->d_alphas;
  fa.ring_base = ring_base;
  fa.R = pde->ring;
  // the application a deferring solve left to its caller carries that solve's guess terms (as beat_pde_x_flush)
  fa.gt = pde->guess.take_pending();
  if (fa.gt.d != nullptr) return launch_events<2>(pde->ctx, dev_x, pde->n, *maps, t0, t1, fa);
  return launch_events<1>(pde->ctx, dev_x, pde->n, *maps, t0, t1, fa);
}
