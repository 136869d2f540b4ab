// Drives csrc/beat_pcg_scalar.h on the host (tests/test_pcg_scalar_cpu.py, tests/test_pcg_scalar_gpu.py): one command per line on
// stdin, one line per command on stdout.  One scalar state of BEAT_ST_DOUBLES doubles and a ring of 12 step lengths; every step goes
// through beat_pcg_step, as the kernels' do.  Numbers come in as strtod reads them (hex floats, nan, inf) and go out as the 16 hex
// digits of their bits.
//   layout                         the slots, BEAT_ST_DOUBLES and the step kinds as name=value words
//   set SLOT VALUE [SLOT VALUE ..] state slots
//   alpha SLOT VALUE [..]          ring slots
//   begin RTOL ATOL MAX_IT | roll | predict SLOT C | merged SLOT | dump
// Every command but layout answers with the state and the ring: "<command> st=b,b,.. alphas=b,b,..".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "beat_pcg_scalar.h"

using namespace beat_pde_detail;

namespace {
constexpr int NALPHA = 12;
double st[BEAT_ST_DOUBLES], alphas[NALPHA];

void print_bits(const char* name, const double* v, int n) {
  std::printf(" %s=", name);
  for (int i = 0; i < n; ++i) {
    uint64_t b;
    std::memcpy(&b, v + i, 8);
    std::printf("%s%016llx", i ? "," : "", (unsigned long long)b);
  }
}

bool read_pairs(std::istringstream& in, double* dst, int n) {
  std::string v;
  for (int slot; in >> slot >> v;) {
    if (slot < 0 || slot >= n) return false;
    dst[slot] = std::strtod(v.c_str(), nullptr);
  }
  return true;
}

double number(std::istringstream& in) {
  std::string v;
  in >> v;
  return std::strtod(v.c_str(), nullptr);
}
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    bool ok = true;
    if (cmd == "layout") {
      std::printf("layout BB=%d RZ=%d RR=%d PQ=%d RZN=%d RRN=%d TOL2=%d BETA=%d STOP=%d ITERS=%d REASON=%d RTOL=%d ATOL=%d MAXIT=%d NUPD=%d RR0=%d "
                  "ALPHA=%d PQS=%d RQ=%d QQ=%d DOUBLES=%d NONE=%d ROLL=%d BEGIN=%d PREDICT=%d MERGED=%d\n",
                  BB, RZ, RR, PQ, RZN, RRN, TOL2, BETA, STOP, ITERS, REASON, RTOL, ATOL, MAXIT, NUPD, RR0, ALPHA, PQS, RQ, QQ, BEAT_ST_DOUBLES,
                  STEP_NONE, STEP_ROLL, STEP_BEGIN, STEP_PREDICT, STEP_MERGED);
      std::fflush(stdout);
      continue;
    }
    if (cmd == "set") {
      ok = read_pairs(in, st, BEAT_ST_DOUBLES);
    } else if (cmd == "alpha") {
      ok = read_pairs(in, alphas, NALPHA);
    } else if (cmd == "begin") {
      const double rtol = number(in), atol = number(in), max_it = number(in);
      beat_pcg_step(STEP_BEGIN, st, rtol, atol, max_it, nullptr, 0.0);
    } else if (cmd == "roll") {
      beat_pcg_step(STEP_ROLL, st, 0.0, 0.0, 0.0, nullptr, 0.0);
    } else if (cmd == "predict" || cmd == "merged") {
      int slot = -1;
      in >> slot;
      const double c = cmd == "predict" ? number(in) : 0.0;
      ok = slot >= 0 && slot < NALPHA;
      if (ok) beat_pcg_step(cmd == "predict" ? STEP_PREDICT : STEP_MERGED, st, 0.0, 0.0, 0.0, alphas + slot, c);
    } else if (cmd != "dump") {
      ok = false;
    }
    if (!ok) {
      std::printf("bad command\n");
      std::fflush(stdout);
      return 2;
    }
    std::printf("%s", cmd.c_str());
    print_bits("st", st, BEAT_ST_DOUBLES);
    print_bits("alphas", alphas, NALPHA);
    std::printf("\n");
    std::fflush(stdout);
  }
  return 0;
}
