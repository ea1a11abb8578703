// The launch geometry of the symmetric-half degree-2 kernel (kernels_tensor_wgsym.hpp) as a function of the element box alone.
// Plain C++: a host program prints it (tests/test_wgsym_geometry_cpu.py).
//
// A unit is one segment of seg_len elements of an element column; a workgroup walks cols_per_wg units back to back
// (ColumnWalk, kernels_tensor_wgs.hpp), the last workgroup what is left of them.
//   - Few columns (the boundary layers of a multi-GPU slab): each column is cut into segments with a workgroup of their own,
//     so that the launch still fills the chip; a segment end stores its carried rows like a column end (phase 2 knows).
//   - Many columns: several units per workgroup (the pipeline of the four waves then runs through the unit boundaries: one
//     prologue per workgroup instead of one per unit) as long as the grid still fills the chip several times over.
#pragma once

namespace mimi_hip {

#ifndef WGSYM_SPLIT_BELOW
#define WGSYM_SPLIT_BELOW 512   // cut the columns into segments while the launch has at most this many workgroups
#endif
#ifndef WGSYM_MAX_COLS
#define WGSYM_MAX_COLS 4      // units per workgroup at most
#define WGSYM_MIN_WGS 2048    // ... while at least this many workgroups remain (4 per resident slot)
#endif

struct WgsymGeometry {
  int nseg, seg_len;   // segments per column, elements per segment: nseg * seg_len == box_n[2]
  int cols_per_wg;     // units a workgroup walks
  int grid;            // workgroups: the last one walks n_units - (grid - 1) * cols_per_wg units, n_units = box_n[0] box_n[1] nseg
};

// min_wgs: WGSYM_MIN_WGS, or what MIMI_HIP_WGSYM_MIN_WGS put in its place on the handle (a test seam: INTEGRATION.md section 5)
constexpr WgsymGeometry wgsym_geometry(const int box_n[3], int min_wgs) {
  int nseg = 1;
  while (box_n[0] * box_n[1] * nseg * 2 <= WGSYM_SPLIT_BELOW && box_n[2] % (nseg * 2) == 0 && box_n[2] / (nseg * 2) >= 4) nseg *= 2;
  const int n_units = box_n[0] * box_n[1] * nseg;
  const int want = n_units / min_wgs;
  const int cols_per_wg = want < 1 ? 1 : (want > WGSYM_MAX_COLS ? WGSYM_MAX_COLS : want);
  return WgsymGeometry{nseg, box_n[2] / nseg, cols_per_wg, (n_units + cols_per_wg - 1) / cols_per_wg};
}

}  // namespace mimi_hip
