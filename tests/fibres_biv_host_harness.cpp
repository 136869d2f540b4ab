// Drives the bi-ventricular half of csrc/beat_fibres_kernel.h on the host (tests/test_fibres_biv_cpu.py), as fibres_host_harness.cpp
// drives the single-ventricle half: a problem comes in on stdin, one "name values.." line per item, and every "run" or "bislerp" line
// answers with one line on stdout.  Numbers come in as strtod reads them (hex floats) and go out as the 16 hex digits of their bits.
// The voxel loop and its index arithmetic are the kernel's (csrc/beat_fibres.hip), the rule is the header's.
//   cells CX CY CZ | h HX HY HZ | angles A_ENDO A_EPI B_ENDO B_EPI (radians) | cond S_L S_T | axis AX AY AZ
//   phi_lv V0 V1 .. | phi_rv .. | phi_epi ..  (nodes, x fastest) | psi V0 V1 ..  (absent: the axis) | active 0110..  (absent: every voxel)
//   run            -> "run degenerate=N f=b,b,.. s=.. n=.. M=.."   ((nvoxels, 3) x 3 and (nvoxels, 9), row-major)
//   bislerp FA(3) SA(3) NA(3) FB(3) SB(3) NB(3) T
//                  -> "bislerp qa=.. qb=.. q=.. f=.. s=.. n=.."    (the two frames' quaternions (w, x, y, z), the blend, and its frame)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "beat_fibres_kernel.h"

using namespace beat_fibres_detail;

namespace {

void print_bits(const char* name, const std::vector<double>& v) {
  std::printf(" %s=", name);
  for (size_t i = 0; i < v.size(); ++i) {
    uint64_t b;
    std::memcpy(&b, &v[i], 8);
    std::printf("%s%016llx", i ? "," : "", (unsigned long long)b);
  }
}

void print_quat(const char* name, const beat_fibres_quat& q) { print_bits(name, {q.w, q.x, q.y, q.z}); }

std::vector<double> numbers(std::istringstream& in) {
  std::vector<double> out;
  for (std::string w; in >> w;) out.push_back(std::strtod(w.c_str(), nullptr));
  return out;
}

int fail(const char* why) {
  std::printf("bad input: %s\n", why);
  std::fflush(stdout);
  return 2;
}

}  // namespace

int main() {
  int64_t cells[3] = {0, 0, 0};
  double h[3] = {0, 0, 0}, angles[4] = {0, 0, 0, 0}, cond[2] = {1, 1}, axis[3] = {0, 0, 0};
  bool has_axis = false;
  std::vector<double> phi_lv, phi_rv, phi_epi, psi;
  std::string active;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "cells") {
      const std::vector<double> v = numbers(in);
      if (v.size() != 3) return fail("cells");
      for (int k = 0; k < 3; ++k) cells[k] = (int64_t)v[k];
    } else if (cmd == "h" || cmd == "angles" || cmd == "cond" || cmd == "axis") {
      const std::vector<double> v = numbers(in);
      double* dst = cmd == "h" ? h : cmd == "angles" ? angles : cmd == "cond" ? cond : axis;
      const size_t want = cmd == "angles" ? 4 : cmd == "cond" ? 2 : 3;
      if (v.size() != want) return fail(cmd.c_str());
      for (size_t k = 0; k < want; ++k) dst[k] = v[k];
      if (cmd == "axis") has_axis = true;
    } else if (cmd == "phi_lv") {
      phi_lv = numbers(in);
    } else if (cmd == "phi_rv") {
      phi_rv = numbers(in);
    } else if (cmd == "phi_epi") {
      phi_epi = numbers(in);
    } else if (cmd == "psi") {
      psi = numbers(in);
    } else if (cmd == "active") {
      in >> active;
    } else if (cmd == "run") {
      if (cells[0] < 1 || cells[1] < 1 || cells[2] < 1) return fail("no cells");
      const int64_t cx = cells[0], cy = cells[1], cz = cells[2];
      const int64_t nvox = cx * cy * cz, nx = cx + 1, plane = nx * (cy + 1), nodes = plane * (cz + 1);
      if ((int64_t)phi_lv.size() != nodes || (int64_t)phi_rv.size() != nodes || (int64_t)phi_epi.size() != nodes)
        return fail("a transmural field does not have one value per node");
      if (!psi.empty() && (int64_t)psi.size() != nodes) return fail("psi does not have one value per node");
      if (psi.empty() && !has_axis) return fail("neither psi nor axis");
      if (!active.empty() && (int64_t)active.size() != nvox) return fail("active does not have one flag per voxel");
      std::vector<double> f((size_t)(3 * nvox), 0.0), s(f), n(f), M((size_t)(9 * nvox), 0.0);
      long long degenerate = 0;
      for (int64_t v = 0; v < nvox; ++v) {
        if (!active.empty() && active[(size_t)v] == '0') continue;
        const int64_t ix = v % cx, iy = (v / cx) % cy, iz = v / (cx * cy);
        const int64_t base = ix + nx * iy + plane * iz;
        double lv[8], rv[8], epi[8], q[8];
        for (int c = 0; c < 8; ++c) {
          const int64_t node = base + (c & 1) + nx * ((c >> 1) & 1) + plane * ((c >> 2) & 1);
          lv[c] = phi_lv[(size_t)node];
          rv[c] = phi_rv[(size_t)node];
          epi[c] = phi_epi[(size_t)node];
          if (!psi.empty()) q[c] = psi[(size_t)node];
        }
        degenerate += beat_fibres_biv_voxel(lv, rv, epi, psi.empty() ? nullptr : q, h, axis, angles[0], angles[1], angles[2], angles[3],
                                            &f[(size_t)(3 * v)], &s[(size_t)(3 * v)], &n[(size_t)(3 * v)], cond[0], cond[1],
                                            &M[(size_t)(9 * v)])
                          ? 1
                          : 0;
      }
      std::printf("run degenerate=%lld", degenerate);
      print_bits("f", f);
      print_bits("s", s);
      print_bits("n", n);
      print_bits("M", M);
      std::printf("\n");
      std::fflush(stdout);
    } else if (cmd == "bislerp") {
      const std::vector<double> v = numbers(in);
      if (v.size() != 19) return fail("bislerp takes two frames (f, s, n) and t");
      const beat_fibres_quat qa = beat_fibres_frame_to_quat(&v[0], &v[3], &v[6]);
      const beat_fibres_quat qb = beat_fibres_frame_to_quat(&v[9], &v[12], &v[15]);
      const beat_fibres_quat q = beat_fibres_bislerp(qa, qb, v[18]);
      std::vector<double> f(3), s(3), n(3);
      beat_fibres_quat_to_frame(q, f.data(), s.data(), n.data());
      std::printf("bislerp");
      print_quat("qa", qa);
      print_quat("qb", qb);
      print_quat("q", q);
      print_bits("f", f);
      print_bits("s", s);
      print_bits("n", n);
      std::printf("\n");
      std::fflush(stdout);
    } else if (!cmd.empty()) {
      return fail("unknown command");
    }
  }
  return 0;
}
