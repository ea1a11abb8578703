// Prints the S3 tile map of the symmetric-half degree-2 kernel (mimi_amd/csrc/p2_tile_map.hpp) for
// tests/test_wgsym_tile_map_cpu.py: one line "a1 pair tile row" per row of the three chains of a packed b1, then the
// constants the kernel's row moves use and which b1 are packed per block mode.
#include <cstdio>

#include "../mimi_amd/csrc/p2_tile_map.hpp"

int main() {
  using namespace mimi_hip;
  for (int a1 = 0; a1 < 3; ++a1)
    for (int pair = 0; pair < 9; ++pair) {
      const P2TileSlot s = p2_tile_slot(a1, pair);
      std::printf("slot %d %d %d %d\n", a1, pair, s.tile, s.row);
    }
  std::printf("tiles %d\nrider %d\nsplit %d\nshift_low %d\nshift_high %d\n", P2_TILES_PACKED, P2_RIDER, P2_RIDER_SPLIT,
              P2_RIDER_SHIFT_LOW, P2_RIDER_SHIFT_HIGH);
  for (int level = 0; level < 3; ++level)
    for (int mode = 0; mode < 3; ++mode)
      for (int b1 = 0; b1 < 3; ++b1) std::printf("packed %d %d %d %d\n", level, mode, b1, p2_b1_packed(mode, b1, level) ? 1 : 0);
  return 0;
}
