// Drives the lattice half of csrc/beat_snap_kernel.h on the host (tests/test_output_cpu.py): the same functions the pack kernel
// calls per node, here for every node of a small grid.
//   snap_host nx ny nz  lox loy loz  hix hiy hiz  sx sy sz
// prints "counts <nxs> <nys> <nzs>", "samples" followed by snap_node_sample of every node, x fastest, and "wide" followed by four
// values of the per-axis rule past 2^32.
//   snap_host shift <address>
// prints "shift" and the nodes between the 512-byte boundary below the address and the address.
#include <cstdio>
#include <cstdlib>

#include "beat_snap_kernel.h"

using namespace beat_snap_detail;

int main(int argc, char** argv) {
  if (argc == 3 && argv[1][0] == 's') {  // snap_host shift <address>
    std::printf("shift %d\n", snap_row_shift(std::strtoull(argv[2], nullptr, 10)));
    return 0;
  }
  if (argc != 13) {
    std::fprintf(stderr, "usage: snap_host nx ny nz lox loy loz hix hiy hiz sx sy sz\n");
    return 2;
  }
  SnapGeometry g;
  for (int a = 0; a < 3; ++a) {
    g.n[a] = std::atoll(argv[1 + a]);
    g.lo[a] = std::atoll(argv[4 + a]);
    g.hi[a] = std::atoll(argv[7 + a]);
    g.stride[a] = std::atoll(argv[10 + a]);
  }
  std::printf("counts %lld %lld %lld\nsamples", (long long)snap_axis_count(g.lo[0], g.hi[0], g.stride[0]),
              (long long)snap_axis_count(g.lo[1], g.hi[1], g.stride[1]), (long long)snap_axis_count(g.lo[2], g.hi[2], g.stride[2]));
  for (int64_t iz = 0; iz < g.n[2]; ++iz)
    for (int64_t iy = 0; iy < g.n[1]; ++iy)
      for (int64_t ix = 0; ix < g.n[0]; ++ix) std::printf(" %lld", (long long)snap_node_sample(g, ix, iy, iz));
  std::printf("\n");
  // the 64-bit branch of the per-axis rule, which no small grid reaches: indices and strides past 2^32
  const int64_t big = (int64_t)1 << 33;
  std::printf("wide %lld %lld %lld %lld\n", (long long)snap_axis_sample(3 * big, big), (long long)snap_axis_sample(3 * big + 1, big),
              (long long)snap_axis_sample(big + 6, 3), (long long)snap_axis_sample(big + 7, 3));
  return 0;
}
