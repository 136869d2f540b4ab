// Prints what csrc/beat_ode_grid.h yields, one line per case:  tiles num_states cap_env tile_min_states balance blocks
// (tests/test_ode_grid_cpu.py).  First the explicit caps (BEAT_ODE_GRID=<cap>) over 1..600 tiles, then the choice by the model's
// size (cap_env = -1) at the sizes the comments of ode_grid quote and around them.
#include <cstdio>

#include "beat_ode_grid.h"

static void line(unsigned tiles, int num_states, int cap_env, int tile_min_states, int balance) {
  std::printf("%u %d %d %d %d %u\n", tiles, num_states, cap_env, tile_min_states, balance,
              beat_ode_detail::beat_ode_grid_blocks(tiles, num_states, cap_env, tile_min_states, balance != 0));
}

int main() {
  const int caps[] = {0, 1, 2, 3, 5, 7, 8, 64, 24576};
  for (unsigned tiles = 1; tiles <= 600; ++tiles)
    for (int cap : caps)
      for (int balance = 0; balance < 2; ++balance) line(tiles, 19, cap, 12, balance);
  // 256^3 = 65 536 tiles, 512^3 = 524 288; 24 576 and 8 * 24 576 = 196 608: the last sizes without a loop / with balancing
  const unsigned sizes[] = {1, 12, 600, 24576, 24577, 65536, 196608, 196609, 524288};
  const int states[] = {2, 5, 11, 12, 19, 45};
  const int mins[] = {12, 6, 46};
  for (unsigned tiles : sizes)
    for (int ns : states)
      for (int tmin : mins)
        for (int balance = 0; balance < 2; ++balance) line(tiles, ns, -1, tmin, balance);
  return 0;
}
