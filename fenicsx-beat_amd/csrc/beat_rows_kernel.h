// State rows of per-class arrays as fields of the grid, and back (see beat_rows.hip, which launches the kernel; include/beat_hip.h:
// beat_rows_plan_create has the rule).  The first half is plain C++17 without a HIP call: the argument check and one node's rule,
// which the kernel runs on the device and tests/rows_host_harness.cpp on the host against NumPy (tests/test_rows_host_cpu.py).  The
// kernel half is compiled by hipcc only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BEAT_ROWS_FN __host__ __device__ __forceinline__
#else
#define BEAT_ROWS_FN inline
#endif

#ifndef BEAT_ROWS_MAX_FIELDS
#define BEAT_ROWS_MAX_FIELDS 8
#endif
#ifndef BEAT_ROWS_MAX_CLASSES
#define BEAT_ROWS_MAX_CLASSES 32  // BEAT_MAX_CLASSES of include/beat_hip.h (beat_rows.hip asserts that they agree)
#endif

namespace beat_rows_detail {

// what rows_args_ok found (0: nothing); beat_rows.hip has the words
enum RowsError {
  ROWS_OK = 0,
  ROWS_NULL,          // a null pointer where one is needed
  ROWS_NFIELDS,       // nfields outside 1..BEAT_ROWS_MAX_FIELDS
  ROWS_NCLASSES,      // num_classes outside 1..BEAT_ROWS_MAX_CLASSES
  ROWS_N,             // n outside [0, 2^31)
  ROWS_CLASS_N,       // a class_n outside [0, 2^31)
  ROWS_CLASS_LD,      // a class_ld below its class_n
  ROWS_CLASS_ROWS,    // a class without rows
  ROWS_ALIGN,         // a pointer that is not aligned for what it points at
  ROWS_ROW,           // a row outside [0, class_rows[c])
  ROWS_ROW_TWICE,     // collapse: two fields name the same row of a class
  ROWS_MODE,          // unknown mode bits
};

// The sources: class c is an array of class_rows[c] rows of class_n[c] doubles, class_ld[c] doubles apart from class_base[c] on
// (an address as an integer: the host half forms none).
struct RowsShape {
  int64_t n;  // nodes of the grid
  int num_classes;
  uint64_t class_base[BEAT_ROWS_MAX_CLASSES];
  int64_t class_ld[BEAT_ROWS_MAX_CLASSES];
  int64_t class_n[BEAT_ROWS_MAX_CLASSES];
  int class_rows[BEAT_ROWS_MAX_CLASSES];
};

BEAT_ROWS_FN bool rows_below_2_31(int64_t v) { return v >= 0 && v < ((int64_t)1 << 31); }

// what a plan is made of: counts, ranges, alignment (cls: a byte per node, pos: an int32 per node or 0 = none)
BEAT_ROWS_FN RowsError rows_plan_ok(const RowsShape& s, uint64_t cls, uint64_t pos) {
  if (s.num_classes < 1 || s.num_classes > BEAT_ROWS_MAX_CLASSES) return ROWS_NCLASSES;
  if (!rows_below_2_31(s.n)) return ROWS_N;
  if (cls == 0) return ROWS_NULL;
  if ((pos & 3) != 0) return ROWS_ALIGN;
  for (int c = 0; c < s.num_classes; ++c) {
    if (!rows_below_2_31(s.class_n[c])) return ROWS_CLASS_N;
    if (s.class_rows[c] < 1) return ROWS_CLASS_ROWS;
    if (s.class_ld[c] < s.class_n[c]) return ROWS_CLASS_LD;
    if (s.class_base[c] == 0) return ROWS_NULL;
    if ((s.class_base[c] & 7) != 0) return ROWS_ALIGN;
  }
  return ROWS_OK;
}

// what one call brings: rows[f * num_classes + c] is the row of class c that field f is, fields[f] the field's address
BEAT_ROWS_FN RowsError rows_args_ok(const RowsShape& s, int nfields, const int* rows, const uint64_t* fields, bool collapse) {
  if (s.num_classes < 1 || s.num_classes > BEAT_ROWS_MAX_CLASSES) return ROWS_NCLASSES;  // (the tables below hold that many)
  if (nfields < 1 || nfields > BEAT_ROWS_MAX_FIELDS) return ROWS_NFIELDS;
  if (rows == nullptr || fields == nullptr) return ROWS_NULL;
  for (int f = 0; f < nfields; ++f) {
    if (fields[f] == 0) return ROWS_NULL;
    if ((fields[f] & 7) != 0) return ROWS_ALIGN;
    for (int c = 0; c < s.num_classes; ++c) {
      const int r = rows[f * s.num_classes + c];
      if (r < 0 || r >= s.class_rows[c]) return ROWS_ROW;
      if (collapse)  // two stores to one element would race
        for (int g = 0; g < f; ++g)
          if (rows[g * s.num_classes + c] == r) return ROWS_ROW_TWICE;
    }
  }
  return ROWS_OK;
}

// One node's rule in two steps, the second taken with the class known (on the device: wave-uniform).  A class byte at or above
// num_classes has no source (255: tissue without a model, 254: padding) ...
BEAT_ROWS_FN int rows_node_class(unsigned cls, int num_classes) { return (int)cls < num_classes ? (int)cls : -1; }
// ... nor has a position outside the class's array: never addressed
BEAT_ROWS_FN bool rows_pos_ok(int32_t pos, int64_t class_n) { return pos >= 0 && (int64_t)pos < class_n; }

// which element of its class's rows node i is (pos: per node, or null: the array spans the grid, pos[i] = i); -1: no source
BEAT_ROWS_FN int64_t rows_node_source(const RowsShape& s, const unsigned char* cls, const int32_t* pos, int64_t i, int* cls_out) {
  const int c = rows_node_class(cls[i], s.num_classes);
  if (c < 0) return -1;
  const int32_t p = pos != nullptr ? pos[i] : (int32_t)i;
  if (!rows_pos_ok(p, s.class_n[c])) return -1;
  *cls_out = c;
  return p;
}

// the element of class c that field row r's node at position p is, counted in doubles from class_base[c]
BEAT_ROWS_FN int64_t rows_element(const RowsShape& s, int c, int r, int64_t p) { return (int64_t)r * s.class_ld[c] + p; }

}  // namespace beat_rows_detail

#if defined(__HIPCC__)
#include "beat_common.h"

namespace beat_rows_detail {

// The kernel's tables: src[f][c] = class_base[c] + rows[f][c] * class_ld[c], the row of class c that field f is, made per call on
// the host; class_n for the range test.  Both are read with a wave-uniform class only (scalar loads from the argument segment).
struct RowsTable {
  double* src[BEAT_ROWS_MAX_FIELDS][BEAT_ROWS_MAX_CLASSES];
  uint32_t class_n[BEAT_ROWS_MAX_CLASSES];
};

struct RowsFields {
  double* f[BEAT_ROWS_MAX_FIELDS];
};

struct RowsLaunch {
  int64_t n;
  const unsigned char* cls;
  const int32_t* pos;  // or null
  int num_classes;
  int nfields;
  double fill;
};

// One pass over the n nodes of the grid, grid-stride in blocks of BEAT_BLOCK: node i reads its class byte and its position and moves
// up to NF >= nfields doubles between element pos of its class's rows and element i of the fields.  COLLAPSE false (expand): the
// fields are written, once per node and a whole wave at a time; a node without a source keeps what it has or, FILL, takes `fill`.
// COLLAPSE true: the fields are read a whole wave at a time and the rows written; a node without a source writes nothing.  A wave
// takes the classes it meets one at a time: the class of the first lane still to do becomes wave-uniform, the rows' addresses are
// read from the argument segment with that uniform index (SGPRs) and every lane of that class adds its position.  Runs of one class
// (the compact layout, thirds) take the loop once.  No atomics, no second pass: the same input gives the same bits.  NT: the loads
// of what is copied are non-temporal -- a choice to measure (tools/bench_rows.py).
template <bool COLLAPSE, bool FILL, bool NT, int NF>
__global__ __launch_bounds__(BEAT_BLOCK) void rows_kernel(RowsLaunch a, RowsTable t, RowsFields fields) {
  const int64_t step = (int64_t)gridDim.x * BEAT_BLOCK;
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * BEAT_BLOCK + threadIdx.x; i < a.n; i += step) {
    const int c = rows_node_class(a.cls[i], a.num_classes);
    const int32_t p = a.pos != nullptr ? (c >= 0 ? a.pos[i] : 0) : (int32_t)i;
    double v[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      v[f] = a.fill;
      if (COLLAPSE && f < a.nfields) v[f] = NT ? __builtin_nontemporal_load(fields.f[f] + i) : fields.f[f][i];
    }
    bool todo = c >= 0, got = false;
    while (todo) {  // (the lanes still to do)
      const int cu = __builtin_amdgcn_readfirstlane(c);
      // the class's lanes are singled out through a ballot: behind a plain `c == cu` the compiler knows the two are equal and
      // indexes the tables with the lane's c (vector loads of the argument segment, one dependent trip more)
      if ((__ballot(c == cu) >> lane) & 1) {
        const int64_t n_cu = (int64_t)t.class_n[cu];
        todo = false;
        if (rows_pos_ok(p, n_cu)) {
          got = true;
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            if (f < a.nfields) {
              double* row = t.src[f][cu];
              if (COLLAPSE)
                row[(uint32_t)p] = v[f];
              else
                v[f] = NT ? __builtin_nontemporal_load(row + (uint32_t)p) : row[(uint32_t)p];
            }
          }
        }
      }
    }
    if (!COLLAPSE && (FILL || got)) {
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (f < a.nfields) fields.f[f][i] = v[f];
    }
  }
}

}  // namespace beat_rows_detail
#endif  // __HIPCC__
