// Drives the host half of csrc/beat_rows_kernel.h (tests/test_rows_host_cpu.py): the argument checks, and one node's rule for every
// node of a small grid -- the same functions the kernel calls.
//   rows_host run <case file>     expand (KEEP and FILL) and collapse over whole arrays
//   rows_host check <case file>   the codes of rows_plan_ok and rows_args_ok (expand, collapse); no array is touched
// The case file is a list of "key count values...": n, num_classes, class_base (doubles from the arena's start), class_ld, class_n,
// class_rows, nfields, rows (nfields * num_classes), arena (doubles in it), fill, cls, pos (count 0: none), addr (check: the
// addresses of cls, pos, the arena and the fields).
// run: the arena holds arena[j] = j; expand reads field f of node i from it into an output that held -(1 + i + 1000 f) -- printed
// as "keep f v..." / "fill f v..."; collapse writes 1e7 + 1e5 f + i from the fields into the arena -- printed as "arena v...".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "beat_rows_kernel.h"

using namespace beat_rows_detail;

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: rows_host run|check <case file>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::map<std::string, std::vector<double>> kv;
  std::string key;
  size_t count;
  while (in >> key >> count) {
    std::vector<double>& v = kv[key];
    v.resize(count);
    for (size_t k = 0; k < count; ++k) in >> v[k];
  }
  if (!in.eof() && in.fail() && !kv.count("n")) {
    std::fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  auto num = [&](const char* k) { return kv.at(k).at(0); };
  const int num_classes = (int)num("num_classes"), nfields = (int)num("nfields");
  RowsShape s{};
  s.n = (int64_t)num("n");
  s.num_classes = num_classes;
  const bool check = std::strcmp(argv[1], "check") == 0;
  const uint64_t arena_addr = check ? (uint64_t)kv.at("addr").at(2) : 0;
  for (int c = 0; c < num_classes && c < BEAT_ROWS_MAX_CLASSES; ++c) {
    s.class_base[c] = arena_addr + 8 * (uint64_t)kv.at("class_base").at(c);  // (run: a byte offset into the arena)
    s.class_ld[c] = (int64_t)kv.at("class_ld").at(c);
    s.class_n[c] = (int64_t)kv.at("class_n").at(c);
    s.class_rows[c] = (int)kv.at("class_rows").at(c);
  }
  std::vector<int> rows(kv.at("rows").begin(), kv.at("rows").end());

  if (check) {
    const std::vector<double>& addr = kv.at("addr");
    std::vector<uint64_t> fields(addr.begin() + 3, addr.end());
    const bool null_rows = kv.count("null_rows") != 0;
    std::printf("plan %d\n", (int)rows_plan_ok(s, (uint64_t)addr[0], (uint64_t)addr[1]));
    std::printf("expand %d\n", (int)rows_args_ok(s, nfields, null_rows ? nullptr : rows.data(), fields.data(), false));
    std::printf("collapse %d\n", (int)rows_args_ok(s, nfields, null_rows ? nullptr : rows.data(), fields.data(), true));
    return 0;
  }

  if (rows_plan_ok(s, 1, 0) != ROWS_OK) {  // (alignment apart: the offsets stand for addresses)
    std::fprintf(stderr, "the case is not a valid plan\n");
    return 2;
  }
  const int64_t n = s.n;
  std::vector<unsigned char> cls(kv.at("cls").begin(), kv.at("cls").end());
  std::vector<int32_t> pos(kv.at("pos").begin(), kv.at("pos").end());
  const int32_t* posp = pos.empty() ? nullptr : pos.data();
  std::vector<double> arena((size_t)num("arena"));
  for (size_t j = 0; j < arena.size(); ++j) arena[j] = (double)j;
  const double fill = num("fill");
  // element of the arena that field f of node i is, or -1
  auto element = [&](int f, int64_t i) -> int64_t {
    int c = -1;
    const int64_t p = rows_node_source(s, cls.data(), posp, i, &c);
    if (p < 0) return -1;
    return (int64_t)(s.class_base[c] / 8) + rows_element(s, c, rows[f * num_classes + c], p);
  };
  for (int mode = 0; mode < 2; ++mode) {
    for (int f = 0; f < nfields; ++f) {
      std::vector<double> out((size_t)n);  // exactly n long: the sanitizer sees a store outside [0, n)
      for (int64_t i = 0; i < n; ++i) out[i] = -(1.0 + i + 1000.0 * f);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t e = element(f, i);
        if (e >= 0)
          out[i] = arena.at((size_t)e);
        else if (mode == 1)
          out[i] = fill;
      }
      std::printf(mode == 0 ? "keep %d" : "fill %d", f);
      for (int64_t i = 0; i < n; ++i) std::printf(" %.17g", out[i]);
      std::printf("\n");
    }
  }
  uint64_t unused[BEAT_ROWS_MAX_FIELDS] = {8, 8, 8, 8, 8, 8, 8, 8};
  if (rows_args_ok(s, nfields, rows.data(), unused, true) == ROWS_OK) {
    for (int f = 0; f < nfields; ++f)
      for (int64_t i = 0; i < n; ++i) {
        const int64_t e = element(f, i);
        if (e >= 0) arena.at((size_t)e) = 1e7 + 1e5 * f + i;
      }
    std::printf("arena");
    for (double v : arena) std::printf(" %.17g", v);
    std::printf("\n");
  }
  return 0;
}
