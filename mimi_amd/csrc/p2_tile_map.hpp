// Where the rows of the S3 tiles of the symmetric-half degree-2 kernel come from (kernels_tensor_wgs.hpp, wgs_contract_block
// with PACK).  Plain C++: a host program prints the map (tests/test_wgsym_tile_map_cpu.py).
//
// A tile row is one pair (a2, b2) of one chain (a1, b1), pair index = 3 a2 + b2; a result row r lies in accumulator register
// r / 4 of the lanes with lane >> 4 == r % 4.  Unpacked, a chain has a tile of its own and uses rows 0..8.  Packed, the three
// chains a1 = 0, 1, 2 of one b1 share TWO tiles: the chains a1 = 0 and a1 = 2 (the hosts) keep rows 0..8 of tile 0 and tile 1,
// the chain a1 = 1 (the rider) has its pairs 0..6 in rows 9..15 of tile 0 and its pairs 7, 8 in rows 12, 13 of tile 1.
// The z-carry adds pair p >= 4 with a2, b2 >= 1 (p = 4, 5, 7, 8) of an element to pair p - 4 of the next one:
//   - in every chain's own run of rows p sits four rows above p - 4: the next accumulator register of the same lane;
//   - the rider's pairs 7, 8 sit in the SAME rows (12, 13) of tile 1 as its pairs 3, 4 in tile 0: the same register of the
//     same lane -- no lane is crossed either way.
#pragma once

namespace mimi_hip {

struct P2TileSlot {
  int tile, row;
};

constexpr int P2_TILES_PACKED = 2;         // tiles of the three chains of one b1
constexpr int P2_RIDER = 1;                // a1 of the chain without a tile of its own
constexpr int P2_RIDER_SPLIT = 7;          // its pairs < 7 ride in tile 0, its pairs 7, 8 in tile 1
constexpr int P2_RIDER_SHIFT_LOW = 9;      // rows its pairs 0..6 move up
constexpr int P2_RIDER_SHIFT_HIGH = 5;     // rows its pairs 7, 8 move up

constexpr P2TileSlot p2_tile_slot(int a1, int pair) {
  return a1 == 0   ? P2TileSlot{0, pair}
         : a1 == 2 ? P2TileSlot{1, pair}
         : pair < P2_RIDER_SPLIT ? P2TileSlot{0, pair + P2_RIDER_SHIFT_LOW}
                                 : P2TileSlot{1, pair + P2_RIDER_SHIFT_HIGH};
}

// The b1 whose three chains are packed, by block mode and packing level.
// Level 2 packs wherever a block contracts all three chains of a b1: every b1 of an off-diagonal block (MODE 1), b1 = 0 of a
// diagonal block (MODE 2: chains a1 >= b1) -- 183 matrix instructions per element instead of 231.
// Level 1, the shipped one, packs b1 = 0, 1 of the off-diagonal block only: 207.  The disassembly lint of the degree-2 kernels
// (tests/test_isa_lint_cpu.py) asks for more than 200 matrix instructions in the kernel's text and for a vector write of a
// result register exactly at the compiler's padding distance; level 2 has neither.
constexpr bool p2_b1_packed(int mode, int b1, int level) {
  return level >= 2 ? mode == 1 || (mode == 2 && b1 == 0) : level == 1 && mode == 1 && b1 < 2;
}

}  // namespace mimi_hip
