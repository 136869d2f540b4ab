// Drives csrc/beat_jit_check.h on the host (tests/test_jit_check_cpu.py): one command per line on stdin, one line of key=value
// words per command on stdout.  Numbers travel as C99 hexadecimal floats (or nan / inf), so both sides see the same bits.
//   compare ROWS NC RTOL ATOL A_0 .. A_{ROWS NC - 1} B_0 .. B_{ROWS NC - 1}     a (under test) against b (the reference), row-major
//   env unset | env set [VALUE]                                                 BEAT_JIT_SELF_CHECK, then what the switch says
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "beat_jit_check.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, word;
    in >> cmd;
    if (cmd == "compare") {
      size_t rows = 0, nc = 0;
      in >> rows >> nc;
      std::vector<double> v;
      while (in >> word) v.push_back(std::strtod(word.c_str(), nullptr));
      if (v.size() != 2 + 2 * rows * nc) {
        std::printf("compare error=count\n");
        return 2;
      }
      // (two allocations of exactly rows x nc doubles: a read outside either is the address sanitizer's to report)
      const std::vector<double> a(v.begin() + 2, v.begin() + 2 + rows * nc), b(v.begin() + 2 + rows * nc, v.end());
      BeatJitMismatch bad;
      if (beat_jit_rows_agree(a.data(), b.data(), rows, nc, v[0], v[1], &bad))
        std::printf("compare ok=1");
      else
        std::printf("compare ok=0 row=%zu node=%zu x=%a y=%a", bad.row, bad.node, bad.x, bad.y);
    } else if (cmd == "env") {
      in >> word;
      if (word == "unset") {
        ::unsetenv("BEAT_JIT_SELF_CHECK");
      } else {
        std::string value;
        in >> value;
        ::setenv("BEAT_JIT_SELF_CHECK", value.c_str(), 1);
      }
      std::printf("env off=%d", beat_jit_checks_off() ? 1 : 0);
    } else {
      std::printf("unknown command\n");
      return 2;
    }
    std::printf("\n");
    std::fflush(stdout);
  }
  return 0;
}
