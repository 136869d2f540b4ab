// Field snapshots behind the time loop: down-sampled, cropped and converted on the device, copied to pinned host memory on a side
// stream while the loop goes on.  Every tissue demo of the reference saves from the host, once per millisecond of simulated time:
//   demos/niederer_benchmark.py:226-277, demos/slab.py:284-299, demos/lv_endocardial.py:311-326, demos/biv_endocardial.py:299-314,
//   demos/ukb_atlas.py:386-418, demos/fitzhughnagumo.py:252-301
//       vtx.write(t); io4dolfinx.write_function(..., solver.pde.state, time=t, name="v"); print(v.max(), v.min())
// which here is a flush of the deferred update, a synchronous copy of the whole fp64 field and a disk write on the thread that
// drives the GPU.
//
// A beat_snap owns `depth` slots -- a device staging buffer and a pinned host buffer of the same layout (the frames of the fields one
// after another, then the pack kernel's block partials of min / max / nonfinite), and two events -- and one non-blocking side stream
// (as beat_dist.hip makes its own).  beat_snap_enqueue: the pack launch on the context's compute stream, behind whatever last wrote
// the fields; an event there; the side stream waits for it and copies the slot device-to-host; a second event.  The fields may be
// overwritten as soon as enqueue has returned: the frame is in the staging buffer by stream order.  beat_snap_wait blocks on the
// second event -- from any host thread -- and finishes the statistics on the host, in a fixed order.  A slot is in flight from
// enqueue to release; with every slot in flight enqueue returns BEAT_EBUSY: back-pressure is the caller's decision.
#include "beat_snap_kernel.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <vector>

using namespace beat_snap_detail;

struct beat_snap {
  beat_ctx* ctx = nullptr;
  SnapLaunch launch{};
  int dtype = 0, depth = 0, nt_loads = 0;
  dim3 grid{1, 1, 1};
  int64_t nblocks = 0;
  size_t frame_bytes = 0;     // all fields' frames
  size_t partials_off = 0;    // where the partials begin in a slot (8-byte aligned)
  size_t slot_bytes = 0;
  hipStream_t side = nullptr;
  struct Slot {
    void* dev = nullptr;
    void* host = nullptr;
    hipEvent_t packed = nullptr, copied = nullptr;
    std::atomic<int> in_flight{0};
  };
  std::vector<Slot> slots;
  int next = 0;  // where enqueue starts looking for a free slot (frames then take the slots in turn)
};

namespace {

void snap_free(beat_snap* s) {
  for (auto& sl : s->slots) {
    if (sl.packed) (void)hipEventDestroy(sl.packed);
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.host) (void)hipHostFree(sl.host);
  }
  if (s->side) (void)hipStreamDestroy(s->side);
  delete s;
}

// allocation of everything a snapshot object owns; a failure leaves what was made to the caller's snap_free
int snap_allocate(beat_snap* s) {
  BEAT_HIP_CHECK(hipSetDevice(s->ctx->device));
  BEAT_HIP_CHECK(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
  for (auto& sl : s->slots) {
    BEAT_HIP_CHECK(hipMalloc(&sl.dev, s->slot_bytes));
    BEAT_HIP_CHECK(hipHostMalloc(&sl.host, s->slot_bytes, hipHostMallocDefault));
    BEAT_HIP_CHECK(hipEventCreateWithFlags(&sl.packed, hipEventDisableTiming));
    BEAT_HIP_CHECK(hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
  }
  return BEAT_OK;
}

// the instance that keeps statistics for at least the handle's fields
template <bool F32, bool NT>
void snap_launch(const beat_snap* s, const SnapFields& fields, void* out, double* partials) {
  const dim3 block(BEAT_BLOCK);
  hipStream_t stream = s->ctx->stream;
  const int nf = s->launch.nfields;
  if (nf <= 1)
    BEAT_KERNEL((snap_pack_kernel<F32, NT, 1>), s->grid, block, 0, stream, s->launch, fields, out, partials);
  else if (nf <= 2)
    BEAT_KERNEL((snap_pack_kernel<F32, NT, 2>), s->grid, block, 0, stream, s->launch, fields, out, partials);
  else if (nf <= 4)
    BEAT_KERNEL((snap_pack_kernel<F32, NT, 4>), s->grid, block, 0, stream, s->launch, fields, out, partials);
  else
    BEAT_KERNEL((snap_pack_kernel<F32, NT, BEAT_SNAP_MAX_FIELDS>), s->grid, block, 0, stream, s->launch, fields, out, partials);
}

}  // namespace

// (the reference call sites above: what vtx.write and io4dolfinx.write_function are given is decided here, once per writer)
extern "C" int beat_snap_create(beat_ctx* ctx, const int64_t n[3], const int64_t lo[3], const int64_t hi[3], const int64_t stride[3],
                                int dtype, int nfields, int depth, const unsigned char* dev_mask, double fill, int flags,
                                beat_snap** out) {
  BEAT_REQUIRE(ctx != nullptr && n != nullptr && lo != nullptr && hi != nullptr && stride != nullptr && out != nullptr, "null argument");
  BEAT_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (fp64) or 1 (fp32), got %d", dtype);
  BEAT_REQUIRE(nfields >= 1 && nfields <= BEAT_SNAP_MAX_FIELDS, "nfields must be 1..%d, got %d", BEAT_SNAP_MAX_FIELDS, nfields);
  BEAT_REQUIRE(depth >= 1 && depth <= BEAT_SNAP_MAX_DEPTH, "depth must be 1..%d, got %d", BEAT_SNAP_MAX_DEPTH, depth);
  BEAT_REQUIRE((flags & ~(BEAT_SNAP_STATS | BEAT_SNAP_NT_LOADS)) == 0, "unknown flags 0x%x", flags);
  SnapLaunch a{};
  int64_t nodes = 1;
  a.frame_items = 1;
  for (int k = 0; k < 3; ++k) {
    BEAT_REQUIRE(n[k] >= 1 && n[k] < ((int64_t)1 << 40), "n[%d] = %lld", k, (long long)n[k]);
    BEAT_REQUIRE(stride[k] >= 1, "stride[%d] must be positive, got %lld", k, (long long)stride[k]);
    BEAT_REQUIRE(lo[k] >= 0 && lo[k] < hi[k] && hi[k] <= n[k], "box [%lld, %lld) of axis %d is empty or leaves the grid of %lld nodes",
                 (long long)lo[k], (long long)hi[k], k, (long long)n[k]);
    a.g.n[k] = n[k];
    a.g.lo[k] = lo[k];
    a.g.hi[k] = hi[k];
    a.g.stride[k] = stride[k];
    a.ns[k] = snap_axis_count(lo[k], hi[k], stride[k]);
    a.frame_items *= a.ns[k];
    nodes *= n[k];
    BEAT_REQUIRE(nodes < ((int64_t)1 << 40), "a grid of 2^40 nodes or more");
  }
  a.nfields = nfields;
  a.stats = (flags & BEAT_SNAP_STATS) ? 1 : 0;
  a.fill = fill;
  a.mask = dev_mask;

  beat_snap* s = new beat_snap;
  s->ctx = ctx;
  s->launch = a;
  s->dtype = dtype;
  s->depth = depth;
  s->nt_loads = (flags & BEAT_SNAP_NT_LOADS) ? 1 : 0;
  // the launch: about 4096 blocks over (y rows, z planes, pieces of an x row), each walking the rest with grid-stride loops
  const int64_t rows_y = a.stats ? hi[1] - lo[1] : a.ns[1], rows_z = a.stats ? hi[2] - lo[2] : a.ns[2];
  const int64_t piece_groups = ((hi[0] - lo[0] + 63 + 63) / 64 + BEAT_BLOCK / 64 - 1) / (BEAT_BLOCK / 64);
  const int64_t gx = std::min<int64_t>(rows_y, 64), gy = std::min<int64_t>(rows_z, 4096 / gx);
  const int64_t gz = std::min<int64_t>(piece_groups, std::max<int64_t>(1, 4096 / (gx * gy)));
  s->grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
  s->nblocks = gx * gy * gz;
  s->frame_bytes = (size_t)a.frame_items * (size_t)nfields * (dtype == 1 ? 4 : 8);
  s->partials_off = (s->frame_bytes + 7) & ~(size_t)7;
  s->slot_bytes = s->partials_off + (size_t)nfields * (size_t)s->nblocks * 3 * sizeof(double);
  s->slots = std::vector<beat_snap::Slot>(depth);
  if (int rc = snap_allocate(s)) {
    snap_free(s);
    return rc;
  }
  *out = s;
  return BEAT_OK;
}

// what the frames of those call sites look like in memory, for the caller that writes the files
extern "C" int beat_snap_info(const beat_snap* snap, int64_t* host_out) {
  BEAT_REQUIRE(snap != nullptr && host_out != nullptr, "null argument");
  for (int k = 0; k < 3; ++k) host_out[k] = snap->launch.ns[k];
  host_out[3] = (int64_t)snap->frame_bytes / snap->launch.nfields;
  host_out[4] = (int64_t)snap->slot_bytes;
  host_out[5] = snap->nblocks;
  return BEAT_OK;
}

// vtx.write(t) / io4dolfinx.write_function(..., time=t) of the call sites above, up to the disk: nothing here waits for the device
extern "C" int beat_snap_enqueue(beat_snap* snap, const double* const* dev_fields, int* slot_out) {
  BEAT_REQUIRE(snap != nullptr && dev_fields != nullptr && slot_out != nullptr, "null argument");
  SnapFields fields{};
  for (int f = 0; f < snap->launch.nfields; ++f) {
    BEAT_REQUIRE(dev_fields[f] != nullptr, "field %d is null", f);
    BEAT_REQUIRE(((uintptr_t)dev_fields[f] & 7) == 0, "field %d is not 8-byte aligned", f);
    fields.f[f] = dev_fields[f];
  }
  int slot = -1;
  for (int k = 0; k < snap->depth && slot < 0; ++k) {
    const int c = (snap->next + k) % snap->depth;
    if (snap->slots[c].in_flight.load(std::memory_order_acquire) == 0) slot = c;
  }
  if (slot < 0) {
    beat_set_error("all %d slots are in flight: wait for one and release it", snap->depth);
    return BEAT_EBUSY;
  }
  beat_snap::Slot& sl = snap->slots[slot];
  beat_ctx* ctx = snap->ctx;
  double* partials = reinterpret_cast<double*>(static_cast<char*>(sl.dev) + snap->partials_off);
  if (snap->dtype == 1)
    snap->nt_loads ? snap_launch<true, true>(snap, fields, sl.dev, partials) : snap_launch<true, false>(snap, fields, sl.dev, partials);
  else
    snap->nt_loads ? snap_launch<false, true>(snap, fields, sl.dev, partials) : snap_launch<false, false>(snap, fields, sl.dev, partials);
  BEAT_LAUNCH_CHECK();
  BEAT_HIP_CHECK(hipEventRecord(sl.packed, ctx->stream));
  BEAT_HIP_CHECK(hipStreamWaitEvent(snap->side, sl.packed, 0));
  BEAT_HIP_CHECK(hipMemcpyAsync(sl.host, sl.dev, snap->slot_bytes, hipMemcpyDeviceToHost, snap->side));
  BEAT_HIP_CHECK(hipEventRecord(sl.copied, snap->side));
  sl.in_flight.store(1, std::memory_order_release);
  snap->next = (slot + 1) % snap->depth;
  *slot_out = slot;
  return BEAT_OK;
}

// the demos' print(v.max(), v.min()) comes out of the same pass: no second copy of the field
extern "C" int beat_snap_wait(beat_snap* snap, int slot, void** host_ptr, double* host_stats) {
  BEAT_REQUIRE(snap != nullptr, "null argument");
  BEAT_REQUIRE(slot >= 0 && slot < snap->depth, "slot %d of %d", slot, snap->depth);
  beat_snap::Slot& sl = snap->slots[slot];
  BEAT_REQUIRE(sl.in_flight.load(std::memory_order_acquire) != 0, "slot %d is not in flight", slot);
  BEAT_HIP_CHECK(hipSetDevice(snap->ctx->device));  // (the calling thread may be one that has not touched the device yet)
  BEAT_HIP_CHECK(hipEventSynchronize(sl.copied));
  if (host_ptr != nullptr) *host_ptr = sl.host;
  if (host_stats != nullptr) {
    const double* partials = reinterpret_cast<const double*>(static_cast<const char*>(sl.host) + snap->partials_off);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int f = 0; f < snap->launch.nfields; ++f) {
      double* st = host_stats + 3 * f;
      if (!snap->launch.stats) {  // not computed
        st[0] = st[1] = nan;
        st[2] = -1.0;
        continue;
      }
      double mn = std::numeric_limits<double>::infinity(), mx = -mn, cnt = 0.0;
      for (int64_t b = 0; b < snap->nblocks; ++b) {
        const double* p = partials + ((int64_t)f * snap->nblocks + b) * 3;
        if (p[0] < mn) mn = p[0];
        if (p[1] > mx) mx = p[1];
        cnt += p[2];
      }
      const bool any = mn <= mx;  // (no tissue node in the box, or NaN at every one of them: no minimum)
      st[0] = any ? mn : nan;
      st[1] = any ? mx : nan;
      st[2] = cnt;
    }
  }
  return BEAT_OK;
}

// (the same call sites: the reference's save(t) has returned, its buffers are free for the next one)
extern "C" int beat_snap_release(beat_snap* snap, int slot) {
  BEAT_REQUIRE(snap != nullptr, "null argument");
  BEAT_REQUIRE(slot >= 0 && slot < snap->depth, "slot %d of %d", slot, snap->depth);
  beat_snap::Slot& sl = snap->slots[slot];
  BEAT_REQUIRE(sl.in_flight.load(std::memory_order_acquire) != 0, "slot %d is not in flight", slot);
  BEAT_HIP_CHECK(hipSetDevice(snap->ctx->device));
  BEAT_HIP_CHECK(hipEventSynchronize(sl.copied));  // (a release without a wait: the copy still has to leave the staging buffer)
  sl.in_flight.store(0, std::memory_order_release);
  return BEAT_OK;
}

// vtx.close() at the end of the demos' loops (demos/niederer_benchmark.py:226-277): what is still on its way arrives first
extern "C" int beat_snap_destroy(beat_snap* snap) {
  if (snap == nullptr) return BEAT_OK;
  hipError_t e = hipSetDevice(snap->ctx->device);
  if (e == hipSuccess) e = hipStreamSynchronize(snap->side);  // copies still on their way
  snap_free(snap);
  if (e != hipSuccess) {
    beat_set_error("draining the snapshot stream failed: %s", hipGetErrorString(e));
    return BEAT_EHIP;
  }
  return BEAT_OK;
}
