// What the boundary-face kernels of pressure.hip (integrators::FollowerPressure) and surface.hip (integrators::
// CouplingSurface) share: the size limits of a face, the wave-wide lane read, the non-normalised outward normal of a face
// point, and the face-node incidence lists that give every node gather its fixed summation order.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#ifndef MH_DEV
#define MH_DEV __device__ __forceinline__
#endif

namespace mimi_hip {

constexpr int kPressureMaxDof = 16;    // nodes of a face: (p + 1)^2 at degree 3
constexpr int kPressureMaxQuad = 25;   // points of a face: (p + 2)^2 at degree 3 (rule 2 p + 3)

MH_DEV double pressure_lane_read(double v, int l) {   // the value lane l holds, in every lane (l wave-uniform)
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// the non-normalised outward normal from the surface tangents t = [a_1 | a_2] (contact.hip surface_normal; the orientation
// is the one splines.face_tables builds the face parametrisation for)
template<int DIM>
MH_DEV void pressure_normal(const double* t /*[DIM-1][DIM]*/, double* m) {
  if constexpr (DIM == 2) {
    m[0] = t[1];
    m[1] = -t[0];
  } else {
    m[0] = t[1] * t[5] - t[2] * t[4];
    m[1] = t[2] * t[3] - t[0] * t[5];
    m[2] = t[0] * t[4] - t[1] * t[3];
  }
}

// Host set-up of a node gather over faces of n_dof nodes each (dofs[n_faces * n_dof]): fnodes = the sorted unique node
// ids, local[k] = the index of dofs[k] in fnodes, and per face node l its (face, local node) incidences
// adj[adj_ptr[l] .. adj_ptr[l + 1]) encoded (face << 6) | local node, faces ascending: the summation order of the gather.
// The caller refuses n_faces >= 2^25 (the encoding).
struct FaceIncidences {
  std::vector<int32_t> fnodes, local, adj_ptr, adj;
};

inline FaceIncidences face_incidences(const std::vector<int32_t>& dofs, int n_dof) {
  FaceIncidences r;
  const size_t nfd = dofs.size();
  r.fnodes = dofs;
  std::sort(r.fnodes.begin(), r.fnodes.end());
  r.fnodes.erase(std::unique(r.fnodes.begin(), r.fnodes.end()), r.fnodes.end());
  r.local.resize(nfd);
  for (size_t k = 0; k < nfd; ++k)
    r.local[k] = (int32_t)(std::lower_bound(r.fnodes.begin(), r.fnodes.end(), dofs[k]) - r.fnodes.begin());
  r.adj_ptr.assign(r.fnodes.size() + 1, 0);
  r.adj.resize(nfd);
  for (size_t k = 0; k < nfd; ++k) ++r.adj_ptr[r.local[k] + 1];
  for (size_t l = 0; l < r.fnodes.size(); ++l) r.adj_ptr[l + 1] += r.adj_ptr[l];
  std::vector<int32_t> fill(r.adj_ptr.begin(), r.adj_ptr.end() - 1);
  for (size_t k = 0; k < nfd; ++k) r.adj[fill[r.local[k]]++] = (int32_t)(((k / n_dof) << 6) | (k % n_dof));
  return r;
}

}  // namespace mimi_hip
