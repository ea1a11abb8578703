// The wave-per-face layer of the boundary kernels -- contact.hip and the kernels_face_*.hpp headers; pressure_face_kernel,
// surface_face_kernel, contact_residual_wave_kernel and contact_friction_action_kernel have the same stages in their own text
// (see there).  One wave per face, kFaceWavesPerGroup per workgroup, registers only, no LDS.  A face kernel is made of
//   face_wave_index       the wave's lane and face; false for a wave beyond the last face
//   face_load_nodes       lane c < n_dof holds node c of the face (lanes >= n_dof hold zeros)
//   face_point_stage      lane q = point q: any subset of {nodal scalar, position / direction, (DIM-1) x DIM tangents} at the
//                         point, from the node lanes by face_lane_read
//   face_normal_len / face_normal_rate / face_normal_column    m and |m|, dm along a direction, dm / dx_bj
//   face_lane_entry / face_scatter_points    lane (i, a): the face vector entry summed over the points
//   face_pair_loop        lane = node pair (a, b): the DIM x DIM blocks of the dense face tangent
// THE CONTRACT.  Every accumulator of the point stage sees the nodes c = 0 .. n_dof - 1 in ascending order, one fused
// multiply-add each, in the operand forms fma(N[c], s_c, sq), fma(x, N[c], xq[i]), fma(x, dN[k n_dof + c], t[k DIM + i]);
// the accumulators are independent, so which of them a kernel asks for changes no bit of the others.  Every face vector entry
// sees the points q = 0 .. n_q - 1 in ascending order, one operation each: fused (FUSED) or a product and a sum.  Two kernels
// that form the same x_q, tangents or entries therefore form the same bytes, because there is one text.
// A lane holds one point: FaceSet::create (face_common.hpp) refuses a face of more than 64 points.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#ifndef MH_DEV
#define MH_DEV __device__ __forceinline__
#endif
#define MH_WAVE __device__ __forceinline__   // what reads lanes: device only, whatever MH_DEV is (the host test harness)

namespace mimi_hip {

constexpr int kFaceWavesPerGroup = 4;
constexpr int kFaceWaveThreads = 64 * kFaceWavesPerGroup;

// the face tables every face kernel reads (FaceSet::view() on the host)
struct FaceView {
  int n_faces, n_dof, n_q;
  const int32_t* dofs;       // [n_faces][n_dof] global node ids
  const int32_t* local;      // [n_faces][n_dof] index into the nodal arrays of the face nodes
  const double* N;           // [n_faces][n_q][n_dof]
  const double* dN;          // [n_faces][n_q][dim-1][n_dof]
  const double* weight;      // [n_faces][n_q]
  const double* x_ref;       // [n_nodes][dim]
};

inline dim3 face_wave_grid(int n_faces) { return dim3((unsigned)((n_faces + kFaceWavesPerGroup - 1) / kFaceWavesPerGroup)); }

MH_WAVE bool face_wave_index(const FaceView& v, int& lane, int& f) {
  lane = threadIdx.x & 63;
  f = blockIdx.x * kFaceWavesPerGroup + (threadIdx.x >> 6);
  return f < v.n_faces;
}

MH_WAVE double face_lane_read(double v, int l) {   // the value lane l holds, in every lane (l wave-uniform)
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// the point of the lane (point 0 for the lanes >= n_q, which compute and store nothing that is read)
MH_WAVE int64_t face_lane_point(const FaceView& v, int f, int lane) {
  const int q = lane < v.n_q ? lane : 0;
  return (int64_t)f * v.n_q + q;
}

// Lane c < n_dof: xc = x[node c] -- a direction, or the reference configuration -- or, ADD_REF, x[node c] + x_ref[node c]
// (integrator_utils.cpp:80-89).  Returns the lane's nodal scalar: nodal[local c] (kNodal), that or `value` where nodal is null
// (kNodalOrValue), 0 (kNoNodal).  One guarded block, the scalar first: the lanes >= n_dof keep zeros.
enum FaceNodal { kNoNodal, kNodal, kNodalOrValue };
template<int DIM, bool ADD_REF, FaceNodal NODAL = kNoNodal>
MH_WAVE double face_load_nodes(const FaceView& v, int f, int lane, const double* x, double* xc, const double* nodal = nullptr,
                               double value = 0.0) {
  double sc = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < v.n_dof) {
    if constexpr (NODAL == kNodal) sc = nodal[v.local[(int64_t)f * v.n_dof + lane]];
    if constexpr (NODAL == kNodalOrValue) sc = nodal ? nodal[v.local[(int64_t)f * v.n_dof + lane]] : value;
    const int64_t node = v.dofs[(int64_t)f * v.n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = ADD_REF ? x[node * DIM + i] + v.x_ref[node * DIM + i] : x[node * DIM + i];
  }
  return sc;
}

// lane = point pt: sq = sum_c N_c sc(c), xq = sum_c xc(c) N_c, tq[k][i] = sum_c xc_i(c) dN_k,c -- what the flags ask for
template<int DIM, bool WITH_SCALAR, bool WITH_POS, bool WITH_TANG>
MH_WAVE void face_point_stage(const FaceView& v, int64_t pt, double sc, const double* xc, double* sq, double* xq, double* tq) {
  const int n_dof = v.n_dof;
  const double* N = v.N + pt * n_dof;
  const double* dN = v.dN + pt * n_dof * (DIM - 1);
  if constexpr (WITH_SCALAR) *sq = 0.0;
  if constexpr (WITH_POS) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) xq[i] = 0.0;
  }
  if constexpr (WITH_TANG) {
#pragma unroll
    for (int k = 0; k < (DIM - 1) * DIM; ++k) tq[k] = 0.0;
  }
  for (int c = 0; c < n_dof; ++c) {
    if constexpr (WITH_SCALAR) *sq = __builtin_fma(N[c], face_lane_read(sc, c), *sq);
    if constexpr (WITH_POS || WITH_TANG) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double x = face_lane_read(xc[i], c);
        if constexpr (WITH_POS) xq[i] = __builtin_fma(x, N[c], xq[i]);
        if constexpr (WITH_TANG) {
#pragma unroll
          for (int k = 0; k < DIM - 1; ++k) tq[k * DIM + i] = __builtin_fma(x, dN[k * n_dof + c], tq[k * DIM + i]);
        }
      }
    }
  }
}

// the non-normalised outward normal from the surface tangents t = [a_1 | a_2] (the orientation is the one
// splines.face_tables builds the face parametrisation for)
template<int DIM>
MH_DEV void face_normal(const double* t /*[DIM-1][DIM]*/, double* m) {
  if constexpr (DIM == 2) {
    m[0] = t[1];
    m[1] = -t[0];
  } else {
    m[0] = t[1] * t[5] - t[2] * t[4];
    m[1] = t[2] * t[3] - t[0] * t[5];
    m[2] = t[0] * t[4] - t[1] * t[3];
  }
}

// m, and |m| = |J| (DenseMatrix::Weight, integrator_utils.hpp:216-251)
template<int DIM>
MH_DEV double face_normal_len(const double* t, double* m) {
  face_normal<DIM>(t, m);
  if constexpr (DIM == 2) return sqrt(m[0] * m[0] + m[1] * m[1]);
  else return sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
}

// m, and its rate dm = dt_1 x t_2 + t_1 x dt_2 (3-D), (dt_y, -dt_x) (2-D) along the tangents' rate dt
template<int DIM>
MH_DEV void face_normal_rate(const double* t, const double* dt, double* m, double* dm) {
  face_normal<DIM>(t, m);
  if constexpr (DIM == 2) {
    dm[0] = dt[1];
    dm[1] = -dt[0];
  } else {
    const double *t1 = t, *t2 = t + 3, *d1 = dt, *d2 = dt + 3;
    dm[0] = (d1[1] * t2[2] - d1[2] * t2[1]) + (t1[1] * d2[2] - t1[2] * d2[1]);
    dm[1] = (d1[2] * t2[0] - d1[0] * t2[2]) + (t1[2] * d2[0] - t1[0] * d2[2]);
    dm[2] = (d1[0] * t2[1] - d1[1] * t2[0]) + (t1[0] * d2[1] - t1[1] * d2[0]);
  }
}

// dm / dx_bj: the rate above for dt_k = dN[k n_dof + b] e_j, through the unit vector e (the products by 0 and 1 are exact)
template<int DIM>
MH_DEV void face_normal_column(const double* t, const double* dN, int n_dof, int b, int j, double* dm) {
  if constexpr (DIM == 2) {
    dm[0] = (j == 1) ? dN[b] : 0.0;
    dm[1] = (j == 0) ? -dN[b] : 0.0;
  } else {
    double e[3] = {0, 0, 0};
    e[j] = 1.0;
    const double* t1 = t;
    const double* t2 = t + 3;
    const double d1 = dN[b], d2 = dN[n_dof + b];
    dm[0] = d1 * (e[1] * t2[2] - e[2] * t2[1]) + d2 * (t1[1] * e[2] - t1[2] * e[1]);
    dm[1] = d1 * (e[2] * t2[0] - e[0] * t2[2]) + d2 * (t1[2] * e[0] - t1[0] * e[2]);
    dm[2] = d1 * (e[0] * t2[1] - e[1] * t2[0]) + d2 * (t1[0] * e[1] - t1[1] * e[0]);
  }
}

// lane k = i n_dof + a < n_dof DIM: entry (i, a) of a face vector, sum_q g_i(q) N_q[a] over the points in ascending order, fused
// or as a product and a sum; g is the per-point vector that lane q holds
// The entry comes from face_lane_entry, which a kernel calls AHEAD of its point stage: the integer division then runs under the
// latency of that stage's loads, not between the stage and this loop.
struct FaceEntry {
  int i, a;
};
template<int DIM>
MH_WAVE FaceEntry face_lane_entry(const FaceView& v, int lane) {   // (entry 0 for the lanes >= n_dof DIM, which store nothing)
  const int k = lane < v.n_dof * DIM ? lane : 0;
  return {k / v.n_dof, k % v.n_dof};
}
template<int DIM, bool FUSED>
MH_WAVE double face_scatter_points(const FaceView& v, int f, FaceEntry e, const double* g) {
  const int n_dof = v.n_dof, n_q = v.n_q, i = e.i, a = e.a;
  double Y = 0.0;
  for (int q = 0; q < n_q; ++q) {
    double gi = face_lane_read(g[0], q);
#pragma unroll
    for (int ii = 1; ii < DIM; ++ii) {
      const double w = face_lane_read(g[ii], q);
      gi = i == ii ? w : gi;
    }
    const double Na = v.N[((int64_t)f * n_q + q) * n_dof + a];
    if constexpr (FUSED) Y = __builtin_fma(gi, Na, Y);
    else Y += gi * Na;
  }
  return Y;
}

// lane = node pair (a, b), in trips of 64: body(a, b, acc) fills acc[i DIM + j]; Kf[(a, i)][(j, b)] = acc, or += with ACCUMULATE
template<int DIM, bool ACCUMULATE, class Body>
MH_WAVE void face_pair_loop(int n_dof, int lane, double* Kf, Body&& body) {
  const int n_pairs = n_dof * n_dof, NT = n_dof * DIM;
  for (int pair0 = 0; pair0 < n_pairs; pair0 += 64) {
    const int pair = pair0 + lane;
    const bool on = pair < n_pairs;
    const int a = on ? pair / n_dof : 0, b = on ? pair % n_dof : 0;
    double acc[DIM * DIM];
#pragma unroll
    for (int k = 0; k < DIM * DIM; ++k) acc[k] = 0.0;
    body(a, b, acc);
    if (on) {
#pragma unroll
      for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          double& K = Kf[(a * DIM + i) * NT + j * n_dof + b];
          K = ACCUMULATE ? K + acc[i * DIM + j] : acc[i * DIM + j];
        }
    }
  }
}

}  // namespace mimi_hip
