// Prints the launch geometry of the symmetric-half degree-2 kernel (mimi_amd/csrc/wgsym_geometry.hpp) for
// tests/test_wgsym_geometry_cpu.py: the compile-time constants, then one line "n0 n1 n2 min_wgs nseg seg_len cols_per_wg grid"
// per box read from standard input ("n0 n1 n2 min_wgs" per line; min_wgs 0 = the shipped WGSYM_MIN_WGS).
#include <cstdio>

#include "../mimi_amd/csrc/wgsym_geometry.hpp"

int main() {
  using namespace mimi_hip;
  std::printf("const %d %d %d\n", WGSYM_SPLIT_BELOW, WGSYM_MAX_COLS, WGSYM_MIN_WGS);
  int n[3], min_wgs;
  while (std::scanf("%d %d %d %d", &n[0], &n[1], &n[2], &min_wgs) == 4) {
    const WgsymGeometry g = wgsym_geometry(n, min_wgs ? min_wgs : WGSYM_MIN_WGS);
    std::printf("%d %d %d %d %d %d %d %d\n", n[0], n[1], n[2], min_wgs, g.nseg, g.seg_len, g.cols_per_wg, g.grid);
  }
  return 0;
}
