// State rows of a solver that keeps one array per class of nodes, as fields of the grid -- and back.  The reference's multi-model
// solver keeps an (S_m, N_m) array per marker and moves rows between them and functions on the host:
//   src/beat/odesolver.py:312-339  assign_all_states / states_to_dolfin: for every state, for every marker,
//       arr[self._inds[marker]] = self.values(marker)[index, :]
//   src/beat/odesolver.py:280-292  to_dolfin / from_dolfin: the same for the potential row, in both directions
// Here the arrays live on the device in one of three layouts (one array over the grid with a class byte per node; one compact array
// with a node map; one array per marker), and one launch over the nodes of the grid does the move for up to BEAT_ROWS_MAX_FIELDS
// rows at once: node i reads its class byte cls[i] and its position pos[i] and copies element pos[i] of the row its class has for
// field f to element i of field f (beat_rows_to_fields), or the other way (beat_fields_to_rows).  The kernel and its rule are in
// beat_rows_kernel.h.
#include "beat_rows_kernel.h"

#include <algorithm>

using namespace beat_rows_detail;

static_assert(BEAT_ROWS_MAX_CLASSES == BEAT_MAX_CLASSES, "the class tables of the rows kernel hold BEAT_MAX_CLASSES entries");

struct beat_rows_plan {
  beat_ctx* ctx = nullptr;
  RowsShape shape{};
  const unsigned char* cls = nullptr;
  const int32_t* pos = nullptr;
};

namespace {

const char* rows_error_text(RowsError e) {
  switch (e) {
    case ROWS_NULL: return "a null pointer";
    case ROWS_NFIELDS: return "nfields must be 1..8";
    case ROWS_NCLASSES: return "num_classes must be 1..32";
    case ROWS_N: return "n must be in [0, 2^31)";
    case ROWS_CLASS_N: return "a class_n is not in [0, 2^31)";
    case ROWS_CLASS_LD: return "a class_ld is below its class_n";
    case ROWS_CLASS_ROWS: return "a class has no rows";
    case ROWS_ALIGN: return "a pointer is not aligned (doubles: 8 bytes, positions: 4)";
    case ROWS_ROW: return "a row is outside [0, class_rows[c])";
    case ROWS_ROW_TWICE: return "two fields name the same row of a class";
    case ROWS_MODE: return "unknown mode bits";
    default: return "ok";
  }
}

unsigned rows_grid(int64_t n, int max_blocks) {
  int64_t b = std::max<int64_t>(1, (n + BEAT_BLOCK - 1) / BEAT_BLOCK);
  b = std::min<int64_t>(b, max_blocks > 0 ? max_blocks : 4096);  // (sixteen blocks per CU: the rest is walked grid-stride)
  return (unsigned)b;
}

template <bool COLLAPSE, bool FILL, bool NT>
void rows_launch(const beat_rows_plan* p, const RowsLaunch& a, const RowsTable& t, const RowsFields& fields, int max_blocks) {
  const dim3 grid(rows_grid(a.n, max_blocks)), block(BEAT_BLOCK);
  hipStream_t stream = p->ctx->stream;
  if (a.nfields <= 1)
    BEAT_KERNEL((rows_kernel<COLLAPSE, FILL, NT, 1>), grid, block, 0, stream, a, t, fields);
  else if (a.nfields <= 2)
    BEAT_KERNEL((rows_kernel<COLLAPSE, FILL, NT, 2>), grid, block, 0, stream, a, t, fields);
  else if (a.nfields <= 4)
    BEAT_KERNEL((rows_kernel<COLLAPSE, FILL, NT, 4>), grid, block, 0, stream, a, t, fields);
  else
    BEAT_KERNEL((rows_kernel<COLLAPSE, FILL, NT, BEAT_ROWS_MAX_FIELDS>), grid, block, 0, stream, a, t, fields);
}

// the checks and tables both directions share; BEAT_EINVAL before anything is launched
int rows_prepare(const beat_rows_plan* plan, int nfields, const int* host_rows, const double* const* host_dev_fields, bool collapse,
                 RowsLaunch& a, RowsTable& t, RowsFields& fields) {
  BEAT_REQUIRE(plan != nullptr, "null plan");
  BEAT_REQUIRE(host_rows != nullptr && host_dev_fields != nullptr, "null argument");
  BEAT_REQUIRE(nfields >= 1 && nfields <= BEAT_ROWS_MAX_FIELDS, "nfields must be 1..%d, got %d", BEAT_ROWS_MAX_FIELDS, nfields);
  const RowsShape& s = plan->shape;
  uint64_t addr[BEAT_ROWS_MAX_FIELDS];
  for (int f = 0; f < nfields; ++f) addr[f] = (uint64_t)(uintptr_t)host_dev_fields[f];
  const RowsError e = rows_args_ok(s, nfields, host_rows, addr, collapse);
  BEAT_REQUIRE(e == ROWS_OK, "%s", rows_error_text(e));
  a.n = s.n;
  a.cls = plan->cls;
  a.pos = plan->pos;
  a.num_classes = s.num_classes;
  a.nfields = nfields;
  a.fill = 0.0;
  for (int c = 0; c < s.num_classes; ++c) t.class_n[c] = (uint32_t)s.class_n[c];
  for (int f = 0; f < nfields; ++f) {
    fields.f[f] = const_cast<double*>(host_dev_fields[f]);
    for (int c = 0; c < s.num_classes; ++c)
      t.src[f][c] = reinterpret_cast<double*>((uintptr_t)s.class_base[c]) + rows_element(s, c, host_rows[f * s.num_classes + c], 0);
  }
  return BEAT_OK;
}

}  // namespace

// (odesolver.py:312-339, 280-292: self._inds[marker] and which array a marker's nodes live in, said once)
extern "C" int beat_rows_plan_create(beat_ctx* ctx, int64_t n, const unsigned char* dev_cls, const int32_t* dev_pos, int num_classes,
                                     double* const* host_class_base, const int64_t* host_class_ld, const int64_t* host_class_n,
                                     const int* host_class_rows, beat_rows_plan** out) {
  BEAT_REQUIRE(ctx != nullptr && out != nullptr, "null argument");
  BEAT_REQUIRE(host_class_base != nullptr && host_class_ld != nullptr && host_class_n != nullptr && host_class_rows != nullptr,
               "null argument");
  BEAT_REQUIRE(num_classes >= 1 && num_classes <= BEAT_ROWS_MAX_CLASSES, "num_classes must be 1..%d, got %d", BEAT_ROWS_MAX_CLASSES,
               num_classes);
  RowsShape s{};
  s.n = n;
  s.num_classes = num_classes;
  for (int c = 0; c < num_classes; ++c) {
    s.class_base[c] = (uint64_t)(uintptr_t)host_class_base[c];
    s.class_ld[c] = host_class_ld[c];
    s.class_n[c] = host_class_n[c];
    s.class_rows[c] = host_class_rows[c];
  }
  const RowsError e = rows_plan_ok(s, (uint64_t)(uintptr_t)dev_cls, (uint64_t)(uintptr_t)dev_pos);
  BEAT_REQUIRE(e == ROWS_OK, "%s (n = %lld)", rows_error_text(e), (long long)n);
  beat_rows_plan* p = new beat_rows_plan;
  p->ctx = ctx;
  p->shape = s;
  p->cls = dev_cls;
  p->pos = dev_pos;
  *out = p;
  return BEAT_OK;
}

// odesolver.py:312-339: arr[self._inds[marker]] = self.values(marker)[index, :] for every marker, for up to eight `index` at once
extern "C" int beat_rows_to_fields(beat_rows_plan* plan, int nfields, const int* host_rows, double* const* host_dev_out, int mode,
                                   double fill, int max_blocks) {
  BEAT_REQUIRE((mode & ~(BEAT_ROWS_FILL | BEAT_ROWS_NT_LOADS)) == 0, "unknown mode bits 0x%x", mode);
  RowsLaunch a{};
  RowsTable t{};
  RowsFields fields{};
  if (int rc = rows_prepare(plan, nfields, host_rows, host_dev_out, false, a, t, fields)) return rc;
  if (a.n == 0) return BEAT_OK;
  a.fill = fill;
  const bool nt = (mode & BEAT_ROWS_NT_LOADS) != 0;
  if (mode & BEAT_ROWS_FILL)
    nt ? rows_launch<false, true, true>(plan, a, t, fields, max_blocks) : rows_launch<false, true, false>(plan, a, t, fields, max_blocks);
  else
    nt ? rows_launch<false, false, true>(plan, a, t, fields, max_blocks) : rows_launch<false, false, false>(plan, a, t, fields, max_blocks);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}

// odesolver.py:280-292 (from_dolfin: self._values[marker][v_index, :] = arr[self._inds[marker]]) for any rows
extern "C" int beat_fields_to_rows(beat_rows_plan* plan, int nfields, const int* host_rows, const double* const* host_dev_in,
                                   int max_blocks) {
  RowsLaunch a{};
  RowsTable t{};
  RowsFields fields{};
  if (int rc = rows_prepare(plan, nfields, host_rows, host_dev_in, true, a, t, fields)) return rc;
  if (a.n == 0) return BEAT_OK;
  rows_launch<true, false, false>(plan, a, t, fields, max_blocks);
  BEAT_LAUNCH_CHECK();
  return BEAT_OK;
}

extern "C" int beat_rows_plan_destroy(beat_rows_plan* plan) {
  delete plan;
  return BEAT_OK;
}
