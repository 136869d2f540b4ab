// Drives csrc/beat_guess.h on the host (tests/test_guess_policy_cpu.py): one command per line on stdin, one line of key=value
// words per command on stdout.  The history fields are host arrays of N doubles, laid out like the operator's: each behind a ghost
// plane, FLD doubles apart; a field is printed as its index in that allocation (-1: null pointer).
//   configure ORDER | reset | skip | begin | advance | observe ITERATIONS | end NUPD DEFERRED RING | take | applied
//   record RING_BASE INC_0 .. INC_{N-1}     the x update's part of a flush kernel: loads, then beat_guess_record per node
//   batch IT_0 IT_1 ..                      observe_batch over those solves' iteration counts
//   state | history | fields | traffic | ghost
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "beat_guess.h"

using beat_pde_detail::GuessTerms;

namespace {
constexpr int N = 3, PLANE = 1, FLD = N + 2 * PLANE;

beat_guess_state g;
std::vector<double> mem;

int field_of(const double* p) { return p == nullptr ? -1 : (int)((p - mem.data() - PLANE) / FLD); }

void print_terms(const char* what, const GuessTerms& t) {
  std::printf("%s a=%.17g cd=%.17g cp0=%.17g cp1=%.17g use_e=%d acc=%d d=%d dp0=%d dp1=%d e=%d", what, t.a, t.cd, t.cp[0], t.cp[1], t.use_e,
              t.accumulate, field_of(t.d), field_of(t.dp[0]), field_of(t.dp[1]), field_of(t.e));
}

void print_field(const char* name, const double* f) {
  std::printf(" %s=", name);
  for (int i = 0; i < N; ++i) std::printf(f ? "%s%.17g" : "%snone", i ? "," : "", f ? f[i] : 0.0);
}

void record(int ring_base, const double* inc) {
  const GuessTerms t = g.terms(ring_base);
  for (int i = 0; i < N; ++i) {
    using namespace beat_pde_detail;
    const double e_old = beat_guess_needs_e(t) ? t.e[i] : 0.0;
    const double d_old = beat_guess_needs_d(t) ? t.d[i] : 0.0;
    const double dp0 = beat_guess_needs_dp(t, 0) ? t.dp[0][i] : 0.0;
    const double dp1 = beat_guess_needs_dp(t, 1) ? t.dp[1][i] : 0.0;
    beat_guess_record(t, t.d + i, t.e + i, inc[i], d_old, dp0, dp1, e_old);
  }
  print_terms("record", t);
}
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "configure") {
      int order = 0;
      in >> order;
      const int need = g.configure(order);
      if (need > g.fields()) {  // as beat_pde_set_guess_order: zeroed fields, handed over
        g.attach(nullptr, 0, 0, 0);
        mem.assign((size_t)need * FLD, 0.0);
        g.attach(mem.data(), need, PLANE, FLD);
      }
      std::printf("configure need=%d fields=%d", need, g.fields());
    } else if (cmd == "reset") {
      g.reset();
      std::printf("reset");
    } else if (cmd == "skip") {
      g.skip();
      std::printf("skip");
    } else if (cmd == "begin") {
      g.begin();
      print_terms("begin", g.cur);
    } else if (cmd == "record") {
      int ring_base = 0;
      double inc[N] = {};
      in >> ring_base;
      for (double& v : inc) in >> v;
      if (g.cur.d == nullptr)
        std::printf("record d=-1");
      else
        record(ring_base, inc);
    } else if (cmd == "advance") {
      g.advance();
      std::printf("advance count=%d", g.hist_n);
    } else if (cmd == "observe") {
      int iterations = 0;
      in >> iterations;
      g.observe(iterations);
      std::printf("observe");
    } else if (cmd == "batch") {
      std::vector<double> st;  // the batch's scalar states, 16 doubles per solve: the iteration count in one slot of each
      for (double it; in >> it;) {
        st.resize(st.size() + 16, -1.0);
        st[st.size() - 16] = it;
      }
      g.observe_batch(st.data(), 16, (int)(st.size() / 16));
      std::printf("batch");
    } else if (cmd == "end") {
      int nupd = 0, deferred = 0, ring = 6;
      in >> nupd >> deferred >> ring;
      const bool due = g.end(nupd, deferred != 0, ring);
      std::printf("end due=%d pending=%d count=%d", due ? 1 : 0, g.pending ? 1 : 0, g.hist_n);
    } else if (cmd == "take") {
      print_terms("take", g.take_pending());
    } else if (cmd == "applied") {
      g.pending_applied_behind();
      std::printf("applied");
    } else if (cmd == "state") {
      std::printf("state order=%d cur=%d next=%d e_order=%d since=%d up=%d count=%d pending=%d seen=%d,%d,%d,%d score=%.17g,%.17g,%.17g,%.17g "
                  "hist=%d,%d,%d guess=%d",
                  g.order, g.auto_cur, g.auto_next, g.auto_e_order, g.auto_since_probe, g.auto_probe_up, g.hist_n, g.pending ? 1 : 0,
                  g.auto_seen[0], g.auto_seen[1], g.auto_seen[2], g.auto_seen[3], g.auto_score[0], g.auto_score[1], g.auto_score[2],
                  g.auto_score[3], field_of(g.d_hist[0]), field_of(g.d_hist[1]), field_of(g.d_hist[2]), field_of(g.d_guess));
    } else if (cmd == "history") {
      double *d = nullptr, *e = nullptr;
      int count = -1;
      g.history(&d, &e, &count);
      std::printf("history count=%d", count);
      print_field("d", d);
      print_field("e", e);
    } else if (cmd == "fields") {
      std::printf("fields");
      for (int f = 0; f < g.fields(); ++f) print_field(("f" + std::to_string(f)).c_str(), mem.data() + PLANE + (size_t)f * FLD);
    } else if (cmd == "traffic") {
      int out[4];
      g.traffic(out);
      std::printf("traffic reads=%d writes=%d order=%d who=%d", out[0], out[1], out[2], out[3]);
    } else if (cmd == "ghost") {
      std::printf("ghost e=%d", field_of(g.ghost_e()));
    } else {
      std::printf("unknown command");
      std::fflush(stdout);
      return 2;
    }
    std::printf("\n");
    std::fflush(stdout);
  }
  return 0;
}
