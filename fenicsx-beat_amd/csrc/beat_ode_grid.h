// How many blocks an ionic launch over `tiles` tiles of BEAT_BLOCK nodes gets.  Plain C++: beat_ode.hip (ode_grid, which reads the
// three environment switches once per process and keeps the measurements behind these rules) and the CPU test
// (tests/test_ode_grid_cpu.py) read the arithmetic from here.  A block takes the tiles b, b + blocks, b + 2 blocks, ...
//   cap_env          BEAT_ODE_GRID: blocks per launch at the most; 0: one block per tile; < 0 (unset): by the model's size --
//   tile_min_states  models of this many states and more get one block per tile, smaller ones BEAT_ODE_GRID_SMALL_CAP blocks
//   balance          a cap that leaves at most BEAT_ODE_BALANCE_MAX_TILES tiles to a block is lowered until every block has the
//                    same number of tiles (the last blocks one fewer): no block walks more tiles than under the plain cap
#pragma once

namespace beat_ode_detail {

constexpr int BEAT_ODE_GRID_SMALL_CAP = 24576;
constexpr unsigned BEAT_ODE_BALANCE_MAX_TILES = 8;

inline unsigned beat_ode_grid_blocks(unsigned tiles, int num_states, int cap_env, int tile_min_states, bool balance) {
  unsigned grid = tiles;
  const int grid_cap = cap_env >= 0 ? cap_env : (num_states >= tile_min_states ? 0 : BEAT_ODE_GRID_SMALL_CAP);
  if (grid_cap > 0 && grid > (unsigned)grid_cap) {
    const unsigned per_block = (grid + (unsigned)grid_cap - 1) / (unsigned)grid_cap;
    grid = (balance && per_block <= BEAT_ODE_BALANCE_MAX_TILES) ? (grid + per_block - 1) / per_block : (unsigned)grid_cap;
  }
  return grid;
}

}  // namespace beat_ode_detail
