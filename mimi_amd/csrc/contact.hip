// C ABI + kernels of the contact integrator: integrators::MortarContact
// (reference: src/mimi/integrators/mortar_contact.{hpp,cpp}, MortarContactWorkData in
// integrators/integrator_utils.{hpp,cpp}, NearestDistanceBase::Results in
// coefficients/nearest_distance.hpp:54-194).
//
// The reference's closest-point query is splinepy's proximity search (an absent, un-pinned
// third-party library, nearest_distance.hpp:268-279); here the rigid body is analytic
// (sphere / half space).  Everything downstream of the query follows the reference:
//   pass 1  ElementGapAndArea + ComputePressure   mortar_contact.cpp:148-261
//           nodal area A_i += w |J| N_i, gap G_i += w |J| g N_i, p_i = eps G_i / A_i
//   pass 2  ElementResidual                        mortar_contact.hpp:99-134
//           R(a,i) += -(w |J| p_q) N_a n_i   for faces with any non-zero nodal pressure
//   tangent with the pressure frozen               mortar_contact.cpp:263-295 (FD in the reference;
//           analytic here, or the reference's FD rule in MIMI_HIP_TANGENT_REFERENCE_FD mode)
// Instead of per-thread copies + a mutex (mortar_contact.cpp:235-260,338-341,400-408) every contribution is stored
// densely -- per quadrature point the nodal area / gap shares, per face the residual vector and the tangent block --
// and summed afterwards in a fixed order through the marked nodes' (face, local node) incidences: no atomics, results
// bitwise reproducible like the domain paths (round 3; rounds 1-2 used fp64 atomics here).  The face tables, the
// incidences, the pair positions, the fixed-order sums and the row gather are face_common.hpp's, shared with pressure.hip;
// the stages of the wave-per-face kernels (wave index, node load, point stage, normals, point scatter, node-pair loop) are
// face_wave.hpp's, shared with the action and friction kernels (contact_residual_wave_kernel has them in its own text).
// The matrix-free action of the frozen-pressure tangent (mimi_hip_contact_linearize / _apply_tangent, and the Krylov
// solvers' boundary terms through apply_seam.hpp) is kernels_face_action.hpp, shared with pressure.hip as well: it builds
// no face tangent block.  The consistent tangent -- the frozen one plus the derivative of the nodal pressure, which leaves the
// CSR pattern -- exists as such an action only (mimi_hip_contact_set_consistent_tangent, kernels_face_consistent.hpp).
// Friction joins either action when the handle is set to it (mimi_hip_contact_set_friction_action,
// kernels_face_friction_action.hpp).  In the mode "augmented" (mimi_hip_contact_set_augmented, kernels_face_augmented.hpp) the
// nodal pressure is p_i = min(0, lambda_i + eps G_i / A_i) with a multiplier per marked node and the unclamped point gap in
// G_i; a handle that never switches the mode on runs the kernels of the penalty law on its bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "apply_seam.hpp"
#include "common.hpp"
#include "face_common.hpp"
#include "kernels_face_action.hpp"
#include "kernels_face_augmented.hpp"
#include "kernels_face_consistent.hpp"
#include "kernels_face_friction.hpp"
#include "kernels_face_friction_action.hpp"
#include "materials.hpp"
#include "spline_body.hpp"

namespace mimi_hip {

struct ContactArgs {
  SplineBodyDev spline;      // body_kind == MIMI_HIP_BODY_SPLINE
  FaceView v;
  int body_kind;
  double body[8];
  double penalty;
  const double* u;
  double* area;              // [n_marked]
  double* gap;
  double* pressure;
  double* scalars;           // [0] area, [1] pressure integral, [2..4] force, [5] gap norm^2
  int mode;
  // No atomics (round 3): every contribution is stored densely and summed afterwards in a fixed order --
  // bitwise reproducible like the domain paths.
  double* pt_area;           // [n_faces][n_q][n_dof]  w |J| N_a        of a quadrature point
  double* pt_gap;            // [n_faces][n_q][n_dof]  w |J| g N_a
  double* pt_scal;           // [n_faces][n_q]         w |J|  (GapNorm: min(g, 0)^2)
  double* face_r;            // [n_faces][dim][n_dof]  face residual vectors
  double* face_k;            // [n_faces][(a, i)][(j, b)]  face tangent blocks
  double* face_scal;         // [n_faces][1 + dim]     pressure integral, force
  unsigned char* face_active;   // IsPressureZero == false
};

// analytic stand-in for NearestDistance + ComputeNormal<true> + NormalGap
// (nearest_distance.hpp:139-193): true gap and |x_rigid - x_query|
template<int DIM>
MH_DEV void nearest_body(const ContactArgs& p, const double* xq, double& true_g, double& distance) {
  if (p.body_kind == MIMI_HIP_BODY_SPHERE) {
    double d[DIM], nrm = 0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      d[i] = xq[i] - p.body[i];
      nrm += d[i] * d[i];
    }
    nrm = sqrt(nrm);
    const double R = p.body[3];
    double g = 0, dist = 0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double n = d[i] / nrm;
      const double pmq = (p.body[i] + R * n) - xq[i];
      g -= n * pmq;
      dist += pmq * pmq;
    }
    true_g = g;
    distance = sqrt(dist);
  } else if (p.body_kind == MIMI_HIP_BODY_SPLINE) {
    sb_nearest(p.spline, xq, true_g, distance);
  } else {
    double s = 0, dist = 0, g = 0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) s += (xq[i] - p.body[i]) * p.body[3 + i];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double pmq = -s * p.body[3 + i];
      g -= p.body[3 + i] * pmq;
      dist += pmq * pmq;
    }
    true_g = g;
    distance = sqrt(dist);
  }
}

// nearest_body with the body's unit normal at the closest point, the gradient of the gap (kernels_face_consistent.hpp)
template<int DIM>
MH_DEV void nearest_body_normal(const ContactArgs& p, const double* xq, double& true_g, double& distance, double* nu) {
  if (p.body_kind == MIMI_HIP_BODY_SPLINE) {
    double n[3];
    sb_nearest(p.spline, xq, true_g, distance, n);
#pragma unroll
    for (int i = 0; i < DIM; ++i) nu[i] = n[i];
    return;
  }
  nearest_body<DIM>(p, xq, true_g, distance);
  if (p.body_kind == MIMI_HIP_BODY_SPHERE) {
    double nrm = 0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      nu[i] = xq[i] - p.body[i];
      nrm += nu[i] * nu[i];
    }
    nrm = sqrt(nrm);
#pragma unroll
    for (int i = 0; i < DIM; ++i) nu[i] /= nrm;
  } else {
#pragma unroll
    for (int i = 0; i < DIM; ++i) nu[i] = p.body[3 + i];
  }
}

// the Body of contact_consistent_record_kernel
struct ContactBodyQuery {
  ContactArgs a;
  template<int DIM>
  MH_DEV void nearest(const double* xq, double& true_g, double& distance, double* nu) const {
    nearest_body_normal<DIM>(a, xq, true_g, distance, nu);
  }
};

// J = x_e^T dN_dxi (integrator_utils.cpp:101-105); returns |J| (DenseMatrix::Weight) and the
// NON-normalised normal m (ComputeUnitNormal before the division, integrator_utils.hpp:216-251)
template<int DIM>
MH_DEV double surface_normal(int n_dof, const double* x_e /*[DIM][n_dof]*/, const double* dN /*[DIM-1][n_dof]*/,
                             double* m, double* t /*[DIM-1][DIM]*/) {
#pragma unroll
  for (int k = 0; k < DIM - 1; ++k)
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      double s = 0;
      for (int a = 0; a < n_dof; ++a) s += x_e[i * n_dof + a] * dN[k * n_dof + a];
      t[k * DIM + i] = s;
    }
  return face_normal_len<DIM>(t, m);
}

template<int DIM>
MH_DEV void gather_x(const ContactArgs& p, int f, double* x_e) {
  // integrator_utils.cpp:80-89: x_e = u[v_dofs] + X_ref
  for (int a = 0; a < p.v.n_dof; ++a) {
    const int64_t node = p.v.dofs[(int64_t)f * p.v.n_dof + a];
#pragma unroll
    for (int i = 0; i < DIM; ++i) x_e[i * p.v.n_dof + a] = p.u[node * DIM + i] + p.v.x_ref[node * DIM + i];
  }
}

// pass 1: one thread per (face, quadrature point).  AUG (the augmented mode): the gap enters the nodal sum unclamped, the
// clamp sits at the node (contact_pressure_kernel<true>); the gap norm and pt_scal are the same in both
template<int DIM, bool AUG>
__global__ void contact_gap_area_kernel(ContactArgs p, int gap_norm_only) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)p.v.n_faces * p.v.n_q) return;
  const int f = idx / p.v.n_q;
  const int64_t pt = idx;
  // x_e = u[v_dofs] + X_ref (integrator_utils.cpp:80-89) is used node by node as it arrives: the point's position and the
  // two tangents J = x_e^T dN_dxi (integrator_utils.cpp:101-105) in one pass, no private array
  const double* N = p.v.N + pt * p.v.n_dof;
  const double* dN = p.v.dN + pt * p.v.n_dof * (DIM - 1);
  double xq[DIM], t[(DIM - 1) * DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xq[i] = 0.0;
#pragma unroll
  for (int k = 0; k < (DIM - 1) * DIM; ++k) t[k] = 0.0;
  for (int a = 0; a < p.v.n_dof; ++a) {
    const int64_t node = p.v.dofs[(int64_t)f * p.v.n_dof + a];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double x = p.u[node * DIM + i] + p.v.x_ref[node * DIM + i];
      xq[i] = __builtin_fma(x, N[a], xq[i]);
#pragma unroll
      for (int k = 0; k < DIM - 1; ++k) t[k * DIM + i] = __builtin_fma(x, dN[k * p.v.n_dof + a], t[k * DIM + i]);
    }
  }
  double true_g, distance;
  nearest_body<DIM>(p, xq, true_g, distance);
  if (gap_norm_only) {
    // GapNorm (mortar_contact.cpp:423-467)
    p.pt_scal[pt] = true_g < 0.0 ? true_g * true_g : 0.0;
    return;
  }
  double g = (AUG || true_g < 0.) ? true_g : 0.;
  // |J| (DenseMatrix::Weight) from the non-normalised normal (integrator_utils.hpp:216-251); this kernel keeps its own text
  double detJ;
  if constexpr (DIM == 2) {
    detJ = sqrt(t[1] * t[1] + t[0] * t[0]);
  } else {
    const double m0 = t[1] * t[5] - t[2] * t[4], m1 = t[2] * t[3] - t[0] * t[5], m2 = t[0] * t[4] - t[1] * t[3];
    detJ = sqrt(m0 * m0 + m1 * m1 + m2 * m2);
  }
  const double fac = p.v.weight[pt] * detJ;
  p.pt_scal[pt] = fac;
  const double ratio = fabs(true_g) / distance;
  if (acos(ratio < 1. ? ratio : 1.) > 1.e-5) g = 0.0;  // angle tolerance, mortar_contact.cpp:172-181
  const double fac_g = fac * g;
  for (int a = 0; a < p.v.n_dof; ++a) {
    p.pt_area[pt * p.v.n_dof + a] = fac * N[a];
    p.pt_gap[pt * p.v.n_dof + a] = fac_g * N[a];
  }
}

// nodal area / gap (mortar_contact.cpp:182-190, the sums the reference forms under a mutex): one WAVE per marked node;
// entry k = (incidence, quadrature point) of the node goes to lane k % 64 in order, then a fixed-shape tree over the
// lanes -- the same bits every run
__global__ __launch_bounds__(256) void contact_nodal_kernel(int n_marked, int n_q, int n_dof, const int32_t* __restrict__ adj_ptr,
                                                            const int32_t* __restrict__ adj, const double* __restrict__ pt_area,
                                                            const double* __restrict__ pt_gap, double* __restrict__ area,
                                                            double* __restrict__ gap) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= n_marked) return;
  const int t0 = adj_ptr[l], n = (adj_ptr[l + 1] - t0) * n_q;
  double sa = 0.0, sg = 0.0;
  for (int k = lane; k < n; k += 64) {
    const int ea = adj[t0 + k / n_q];
    const int64_t pt = (int64_t)(ea >> 6) * n_q + k % n_q;
    sa += pt_area[pt * n_dof + (ea & 63)];
    sg += pt_gap[pt * n_dof + (ea & 63)];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sa += __shfl_down(sa, off, 64);
    sg += __shfl_down(sg, off, 64);
  }
  if (lane == 0) {
    area[l] = sa;
    gap[l] = sg;
  }
}

// (AUG: p_i = min(0, lambda_i + eps G_i / A_i), +0.0 on a released node)
template<bool AUG>
__global__ void contact_pressure_kernel(int n, const double* area, const double* gap, double penalty, const double* lambda,
                                        double* pressure) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (AUG) {
    if (i < n) {
      const double v = lambda[i] + gap[i] / area[i] * penalty;
      pressure[i] = v < 0.0 ? v : 0.0;
    }
  } else {
    if (i < n) pressure[i] = gap[i] / area[i] * penalty;  // mortar_contact.cpp:253-257
  }
}

// element residual at given x_e (used by the FD mode too)
template<int DIM>
MH_DEV void face_residual(const ContactArgs& p, int f, const double* x_e, const double* p_e, double* R_e,
                          double* force, double* pint) {
  for (int k = 0; k < p.v.n_dof * DIM; ++k) R_e[k] = 0.0;
  for (int q = 0; q < p.v.n_q; ++q) {
    const int64_t pt = (int64_t)f * p.v.n_q + q;
    const double* N = p.v.N + pt * p.v.n_dof;
    double pq = 0;
    for (int a = 0; a < p.v.n_dof; ++a) pq += N[a] * p_e[a];
    double m[DIM], t[(DIM - 1) * DIM];
    const double detJ = surface_normal<DIM>(p.v.n_dof, x_e, p.v.dN + pt * p.v.n_dof * (DIM - 1), m, t);
    const double fac = p.v.weight[pt] * detJ * pq;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double aw = (m[i] / detJ) * (-fac);
      for (int a = 0; a < p.v.n_dof; ++a) R_e[i * p.v.n_dof + a] += aw * N[a];
      if (force) force[i] += fac * (m[i] / detJ);
    }
    if (pint) *pint += fac;
  }
}

// reference-FD mode of pass 2: one thread per face, the face tangent block by forward differences of the face residual
// (stored densely: face_row_gather_kernel)
template<int DIM>
__global__ void contact_residual_kernel(ContactArgs p, int with_grad) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= p.v.n_faces) return;
  double p_e[kFaceMaxDof];
  bool any = false;
  for (int a = 0; a < p.v.n_dof; ++a) {
    p_e[a] = p.pressure[p.v.local[(int64_t)f * p.v.n_dof + a]];
    any = any || (p_e[a] != 0.0);
  }
  if (!any) return;  // IsPressureZero (integrator_utils.cpp:112-119)
  double x_e[DIM * kFaceMaxDof], R_e[DIM * kFaceMaxDof];
  gather_x<DIM>(p, f, x_e);
  face_residual<DIM>(p, f, x_e, p_e, R_e, nullptr, nullptr);
  const int NT = p.v.n_dof * DIM;
  // (the face residual, pressure integral and force are stored by contact_residual_wave_kernel in every mode, so that
  // the history scalars do not depend on the tangent mode to the last bit; this kernel adds the difference tangent)
  if (!with_grad) return;
  double* Kf = p.face_k + (int64_t)f * NT * NT;     // row (a, i): [j][b]
  // mortar_contact.cpp:263-295: forward FD on the current POSITION, pressure frozen
  double fwd[DIM * kFaceMaxDof];
  for (int c = 0; c < NT; ++c) {
    const double orig = x_e[c];
    const double step = (orig != 0.0) ? fabs(orig) * 1.0e-8 : 1.0e-10;
    const double step_inv = 1. / step;
    x_e[c] = orig + step;
    face_residual<DIM>(p, f, x_e, p_e, fwd, nullptr, nullptr);
    x_e[c] = orig;
    const int b = c % p.v.n_dof, j = c / p.v.n_dof;
    for (int a = 0; a < p.v.n_dof; ++a)
#pragma unroll
      for (int i = 0; i < DIM; ++i)
        Kf[(a * DIM + i) * NT + j * p.v.n_dof + b] = (fwd[i * p.v.n_dof + a] - R_e[i * p.v.n_dof + a]) * step_inv;
  }
}

// pass 2 without the reference-FD tangent, one WAVE per face: lane = quadrature point for pressure, normal and weights,
// then lane = (i, a) for the residual entries -- summed over the points in the order of the one-thread form above, so
// the two give the same bits (that form left 9 216 faces to 144 waves: 0.19 ms of latency at configuration 4)
// (The kernel keeps its own stage text: on face_wave.hpp's helpers it computed the same bytes with 2 to 5 instructions more.)
template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_residual_wave_kernel(ContactArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.v.n_faces) return;
  const int n_dof = p.v.n_dof, n_q = p.v.n_q, NT = n_dof * DIM;
  double pc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    pc = p.pressure[p.v.local[(int64_t)f * n_dof + lane]];
    const int64_t node = p.v.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.u[node * DIM + i] + p.v.x_ref[node * DIM + i];
  }
  const bool any = __ballot(pc != 0.0) != 0;
  if (lane == 0) p.face_active[f] = any ? 1 : 0;
  if (!any) return;  // IsPressureZero (integrator_utils.cpp:112-119)
  // lane q: fac = w detJ p(q), n = m / detJ
  double fac = 0.0, nq[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) nq[i] = 0.0;
  {
    const int q = lane < n_q ? lane : 0;
    const int64_t pt = (int64_t)f * n_q + q;
    const double* N = p.v.N + pt * n_dof;
    const double* dN = p.v.dN + pt * n_dof * (DIM - 1);
    double pq = 0.0, t[(DIM - 1) * DIM];
#pragma unroll
    for (int k = 0; k < (DIM - 1) * DIM; ++k) t[k] = 0.0;
    for (int c = 0; c < n_dof; ++c) {
      pq = __builtin_fma(N[c], face_lane_read(pc, c), pq);
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double x = face_lane_read(xc[i], c);
#pragma unroll
        for (int k = 0; k < DIM - 1; ++k) t[k * DIM + i] = __builtin_fma(x, dN[k * n_dof + c], t[k * DIM + i]);
      }
    }
    double m[DIM], detJ;
    if constexpr (DIM == 2) {
      m[0] = t[1];
      m[1] = -t[0];
      detJ = sqrt(m[0] * m[0] + m[1] * m[1]);
    } else {
      m[0] = t[1] * t[5] - t[2] * t[4];
      m[1] = t[2] * t[3] - t[0] * t[5];
      m[2] = t[0] * t[4] - t[1] * t[3];
      detJ = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    }
    fac = p.v.weight[pt] * detJ * pq;
#pragma unroll
    for (int i = 0; i < DIM; ++i) nq[i] = m[i] / detJ;
  }
  // lane k = i n_dof + a: R(a, i) = sum_q (n_i (-fac))_q N_q[a]
  {
    const int k = lane < NT ? lane : 0, i = k / n_dof, a = k % n_dof;
    double R = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const double mf = -face_lane_read(fac, q);
      double aw = face_lane_read(nq[0], q) * mf;
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double v = face_lane_read(nq[ii], q) * mf;
        aw = i == ii ? v : aw;
      }
      R += aw * p.v.N[((int64_t)f * n_q + q) * n_dof + a];
    }
    if (lane < NT) p.face_r[(int64_t)f * NT + lane] = R;      // [i][a]
  }
  // pressure integral and force of the face: lane 0, in the order of the points
  {
    double pint = 0.0, force[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) force[i] = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const double fq = face_lane_read(fac, q);
#pragma unroll
      for (int i = 0; i < DIM; ++i) force[i] += fq * face_lane_read(nq[i], q);
      pint += fq;
    }
    if (lane == 0) {
      p.face_scal[(int64_t)f * (1 + DIM)] = pint;
#pragma unroll
      for (int i = 0; i < DIM; ++i) p.face_scal[(int64_t)f * (1 + DIM) + 1 + i] = force[i];
    }
  }
}

// analytic frozen-pressure tangent, one WAVE per face (R(a,i) = -w p N_a m_i, d m / d x_bj with p frozen).  Stage 1, lane =
// quadrature point: the pressure and the two surface tangents at the point, from the face's nodal values handed round by
// lane reads (lane c holds node c).  Stage 2, lane = node pair (a, b): its DIM x DIM block accumulated over the points in
// registers, the point's seven numbers read from the lane that computed them.  (Before: every pair lane recomputed
// pressure and tangents of every point from private arrays -- 0.44 ms for the 9 216 faces of configuration 4.)
template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_tangent_kernel(ContactArgs p) {
  int lane, f;
  if (!face_wave_index(p.v, lane, f)) return;
  const int n_dof = p.v.n_dof, n_q = p.v.n_q;   // (<= 16 nodes; <= 64 points: checked at create)
  double xc[DIM];
  const double pc = face_load_nodes<DIM, true, kNodal>(p.v, f, lane, p.u, xc, p.pressure);
  if (__ballot(pc != 0.0) == 0) return;  // IsPressureZero (integrator_utils.cpp:112-119)
  // stage 1: lane q < n_q
  const int64_t pt_q = face_lane_point(p.v, f, lane);
  double pq, tq[(DIM - 1) * DIM];
  face_point_stage<DIM, true, false, true>(p.v, pt_q, pc, xc, &pq, nullptr, tq);
  const double wq = -p.v.weight[pt_q] * pq;
  face_pair_loop<DIM, false>(n_dof, lane, p.face_k + (int64_t)f * (n_dof * DIM) * (n_dof * DIM), [&](int a, int b, double* acc) {
    for (int q = 0; q < n_q; ++q) {
      const int64_t pt = (int64_t)f * n_q + q;
      const double wpn = face_lane_read(wq, q) * p.v.N[pt * n_dof + a];
      const double* dN = p.v.dN + pt * n_dof * (DIM - 1);
      double t[(DIM - 1) * DIM];
#pragma unroll
      for (int k = 0; k < (DIM - 1) * DIM; ++k) t[k] = face_lane_read(tq[k], q);
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        double dm[DIM];
        face_normal_column<DIM>(t, dN, n_dof, b, j, dm);
#pragma unroll
        for (int i = 0; i < DIM; ++i) acc[i * DIM + j] += wpn * dm[i];
      }
    }
  });
}

}  // namespace mimi_hip

using namespace mimi_hip;

// (n_fnodes, fnodes, adj_ptr / adj of the FaceSet are the reference's marked nodes and their incidences)
struct mimi_hip_contact_s : FaceAssembly {
  int mode = MIMI_HIP_TANGENT_ANALYTIC;
  int body_kind = 0;
  double body[8] = {0};
  double penalty = 1e4;
  DeviceBuffer<double> area, gap, pressure, scalars;
  DeviceBuffer<double> pt_area, pt_gap, pt_scal;   // per quadrature point: the dense stores of pass 1
  SplineBodyDev spline{};
  DeviceBuffer<double> sb_knots[2], sb_ctrl, sb_sample_xi, sb_sample_x;
  // mimi_hip_contact_linearize / _apply_tangent (kernels_face_action.hpp, kernels_face_consistent.hpp, kernels_face_friction_action.hpp)
  FrictionContactAction action;
  bool consistent_tangent = false;   // what the NEXT linearize records (mimi_hip_contact_set_consistent_tangent)
  bool friction_action = false;      // friction has a matrix-free action (mimi_hip_contact_set_friction_action)
  // Coulomb friction (kernels_face_friction.hpp); mu == 0: none of it is allocated or launched
  double mu = 0.0, eps_t = 0.0, body_inc[3] = {0.0, 0.0, 0.0};
  DeviceBuffer<double> fr_xi, fr_xbar, fr_xi_t, fr_xbar_t, fr_face, fr_scalars;
  DeviceBuffer<unsigned char> fr_c, fr_c_t;
  bool fr_trial = false;   // an evaluation has written the trial state since create / reset
  // the multipliers of the augmented mode (kernels_face_augmented.hpp); never switched on: none of it is allocated
  AugmentedState aug;
};

// the friction state of a handle: allocated and zeroed by the first set_friction with mu > 0
static void friction_reset(mimi_hip_contact_s* h) {
  const size_t npts = (size_t)h->n_faces * h->n_q, ns = npts * h->dim;
  h->fr_xi.resize(ns);
  h->fr_xbar.resize(ns);
  h->fr_xi_t.resize(ns);
  h->fr_xbar_t.resize(ns);
  h->fr_c.resize(npts);
  h->fr_c_t.resize(npts);
  h->fr_face.resize((size_t)h->n_faces * kFrictionScalars);
  h->fr_scalars.resize(kFrictionScalars);
  for (DeviceBuffer<double>* b : {&h->fr_xi, &h->fr_xbar, &h->fr_xi_t, &h->fr_xbar_t})
    MH_HIP(hipMemsetAsync(b->ptr, 0, ns * sizeof(double), h->stream));
  MH_HIP(hipMemsetAsync(h->fr_c.ptr, 0, npts, h->stream));
  MH_HIP(hipMemsetAsync(h->fr_c_t.ptr, 0, npts, h->stream));
  MH_HIP(hipMemsetAsync(h->fr_scalars.ptr, 0, kFrictionScalars * sizeof(double), h->stream));
  h->fr_trial = false;
}

// the face tables, u and the stores of this evaluation (c), and the handle's friction state
static FrictionArgs friction_args(const mimi_hip_contact_s* h, const ContactArgs& c) {
  return {c.v, c.u, c.pressure, c.face_r, c.face_k, h->mu, h->eps_t, {h->body_inc[0], h->body_inc[1], h->body_inc[2]},
          h->fr_xi.ptr, h->fr_xbar.ptr, h->fr_c.ptr, h->fr_xi_t.ptr, h->fr_xbar_t.ptr, h->fr_c_t.ptr, h->fr_face.ptr};
}

// the trial state over the committed one, on the handle's stream; nothing waits
static void friction_commit(mimi_hip_contact_s* h) {
  const int64_t npts = (int64_t)h->n_faces * h->n_q, ns = npts * h->dim;
  launch(contact_friction_commit_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, h->stream, ns, npts, h->fr_xi_t.ptr,
         h->fr_xbar_t.ptr, h->fr_c_t.ptr, h->fr_xi.ptr, h->fr_xbar.ptr, h->fr_c.ptr);
}

// (lifted: what mimi_hip_contact_set_friction_action(h, 1) makes available)
static void refuse_friction(const mimi_hip_contact_s* h, const char* what, bool lifted = false) {
  if (h->mu > 0.0 && !lifted)
    fail("%s is not available on a contact handle with friction (mu = %g): the friction tangent is assembled only "
         "(set_friction(h, 0, 0) removes it)", what, h->mu);
}

// ---- the operator seam of the Krylov solvers (apply_seam.hpp) ----------------------------------------------------------------
namespace mimi_hip {
int64_t operator_size(const mimi_hip_contact_s* h) { return h->n_vdofs; }
int operator_device(const mimi_hip_contact_s* h) { return h->device; }
void operator_begin_solve(mimi_hip_contact_s* h, hipStream_t solver_stream) {
  refuse_friction(h, "the matrix-free tangent action", h->friction_action);
  h->action.require("contact");
  MH_HIP(hipSetDevice(h->device));
  h->action.begin(*h, solver_stream);
}
void operator_add_action(mimi_hip_contact_s* h, double factor, const double* x, double* y, hipStream_t solver_stream) {
  h->action.add(*h, factor, x, y, solver_stream);
}
}  // namespace mimi_hip

// NearestDistanceToSplines::AddSpline / PlantKdTree (nearest_distance.hpp:223-255): (re)upload the rigid spline and the
// sampled initial guesses.  Called at create time and whenever the caller moved the body and re-planted its tree.
static void upload_spline_body(mimi_hip_contact_s* h, const mimi_hip_spline_body* sp, int dim) {
  // NearestDistanceToSplines::AddSpline / PlantKdTree (nearest_distance.hpp:223-255)
  if (!sp) fail("body_kind spline without a spline description");
  if (sp->para_dim + 1 != dim) fail("boundary para_dim should be one smaller than dim.");   // :121-124
  for (int k = 0; k < sp->para_dim; ++k) {
    const int p = sp->degree[k], n_ctrl = sp->n_knots[k] - p - 1;
    if (p < 0 || p > kMaxBodyDegree) fail("spline body degree %d unsupported (<= %d)", p, kMaxBodyDegree);
    if (n_ctrl < p + 1) fail("spline body knot vector too short");
  }
  size_t n_ctrl = 1;
  for (int k = 0; k < sp->para_dim; ++k) n_ctrl *= (size_t)(sp->n_knots[k] - sp->degree[k] - 1);
  if (sp->weights)
    for (size_t a = 0; a < n_ctrl; ++a)
      if (!(sp->weights[a] > 0.0)) fail("spline body weights must be positive");
  int res = sp->kdtree_resolution > 1 ? sp->kdtree_resolution : 100;
  if (sp->para_dim == 2 && res > 1000) res = 1000;   // res^2 samples: the reference's kd-tree takes what it is given
  if (res > 1000000) res = 1000000;
  // weighted control points, samples and closed directions: the one set-up the tests' host harness runs too
  SplineBodyHost filled;
  const int degree[2] = {sp->degree[0], sp->degree[1]}, n_knots[2] = {sp->n_knots[0], sp->n_knots[1]};
  sb_fill_host(filled, sp->para_dim, dim, degree, n_knots, sp->knots, sp->control_points, sp->weights, res,
               sp->max_iterations);
  const SplineBodyDev& host = filled.dev;
  const std::vector<double>&ctrl_h = filled.ctrl_h, &sxi = filled.sample_xi, &sx = filled.sample_x;
  static const double unit_knots[2] = {0.0, 1.0};
  const int n_s = host.n_samples;
  h->spline = host;
  for (int k = 0; k < sp->para_dim; ++k) {
    h->sb_knots[k].assign(sp->knots[k], (size_t)sp->n_knots[k], h->stream);
    h->spline.knots[k] = h->sb_knots[k].ptr;
  }
  if (sp->para_dim == 1) {
    h->sb_knots[1].assign(unit_knots, 2, h->stream);
    h->spline.knots[1] = h->sb_knots[1].ptr;
  }
  h->sb_ctrl.assign(ctrl_h.data(), ctrl_h.size(), h->stream);
  h->sb_sample_xi.assign(sxi.data(), sxi.size(), h->stream);
  h->sb_sample_x.assign(sx.data(), sx.size(), h->stream);
  h->spline.ctrl_h = h->sb_ctrl.ptr;
  h->spline.sample_xi = h->sb_sample_xi.ptr;
  h->spline.sample_x = h->sb_sample_x.ptr;
  h->spline.n_samples = n_s;
}

static ContactArgs contact_args(mimi_hip_contact_s* h, const double* u) {
  ContactArgs a{};
  a.spline = h->spline;
  a.v = h->view();
  a.body_kind = h->body_kind;
  for (int i = 0; i < 8; ++i) a.body[i] = h->body[i];
  a.penalty = h->penalty;
  a.u = u;
  a.area = h->area.ptr;
  a.gap = h->gap.ptr;
  a.pressure = h->pressure.ptr;
  a.scalars = h->scalars.ptr;
  a.mode = h->mode;
  a.pt_area = h->pt_area.ptr;
  a.pt_gap = h->pt_gap.ptr;
  a.pt_scal = h->pt_scal.ptr;
  a.face_r = h->face_r.ptr;
  a.face_k = h->face_k.ptr;
  a.face_scal = h->face_scal.ptr;
  a.face_active = h->face_active.ptr;
  return a;
}

constexpr int kContactThreads = 128;   // of the one-thread-per-point and per-node kernels

// The kernels of pass 1 (mortar_contact.cpp:148-193), the one place that launches them: the points' gap and area shares, then
// their nodal sums and the area scalar -- or, gap_norm_only, the points' min(g, 0)^2 and their sum into the gap-norm scalar
static void contact_pass1_kernels(mimi_hip_contact_s* h, const ContactArgs& a, int gap_norm_only) {
  const int64_t npts = (int64_t)h->n_faces * h->n_q;
  const dim3 grid((unsigned)((npts + kContactThreads - 1) / kContactThreads));
  face_dispatch_dim(h->dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    launch(h->aug.on ? contact_gap_area_kernel<DIM, true> : contact_gap_area_kernel<DIM, false>, grid, dim3(kContactThreads), 0,
           h->stream, a, gap_norm_only);
  });
  if (!gap_norm_only)
    launch(contact_nodal_kernel, dim3((unsigned)((h->n_fnodes + 3) / 4)), dim3(256), 0, h->stream, h->n_fnodes, h->n_q, h->n_dof,
           h->adj_ptr.ptr, h->adj.ptr, h->pt_area.ptr, h->pt_gap.ptr, h->area.ptr, h->gap.ptr);   // (a wave per marked node, four per workgroup)
}

// the sum of pass 1's point scalars into the history scalar `slot`
static void contact_sum_points(mimi_hip_contact_s* h, int slot) {
  launch(face_sum_kernel, dim3(1), dim3(1024), 0, h->stream, (int64_t)h->n_faces * h->n_q, 1, 1, h->pt_scal.ptr,
         (const unsigned char*)nullptr, h->scalars.ptr + slot);
}

static void contact_pressure(mimi_hip_contact_s* h) {   // mortar_contact.cpp:253-257
  launch(h->aug.on ? contact_pressure_kernel<true> : contact_pressure_kernel<false>,
         dim3((unsigned)((h->n_fnodes + kContactThreads - 1) / kContactThreads)), dim3(kContactThreads), 0, h->stream, h->n_fnodes,
         h->area.ptr, h->gap.ptr, h->penalty, (const double*)h->aug.lambda.ptr, h->pressure.ptr);
}

// pass 1 (mortar_contact.cpp:148-193): nodal area / gap of this handle's faces; pressure not formed yet
static void contact_pass1(mimi_hip_contact_s* h, const double* u_dev) {
  // InitializeGapAreaPressure + last_* reset (mortar_contact.cpp:135-146,302-306)
  MH_HIP(hipMemsetAsync(h->scalars.ptr, 0, 6 * sizeof(double), h->stream));
  contact_pass1_kernels(h, contact_args(h, u_dev), 0);
  contact_sum_points(h, 0);
}

// The snapshot of the frozen-pressure tangent at u: pass 1 and the pressure with the handle's current body and penalty
// (the history scalars of the last Add* call are left alone), then the record of kernels_face_action.hpp -- with the
// consistent part of kernels_face_consistent.hpp when the handle is set to it, and with the friction part of
// kernels_face_friction_action.hpp when the friction action is on and mu > 0: the committed friction state is read, no trial
// state is written.  It is the analytic tangent whatever the tangent mode says.
static void contact_linearize(mimi_hip_contact_s* h, const double* u_dev) {
  const ContactArgs a = contact_args(h, u_dev);
  contact_pass1_kernels(h, a, 0);
  contact_pressure(h);
  const bool rough = h->friction_action && h->mu > 0.0;
  const FrictionArgs fa = rough ? friction_args(h, a) : FrictionArgs{};
  h->action.linearize(*h, u_dev, h->area.ptr, h->pressure.ptr, h->penalty, h->consistent_tangent, ContactBodyQuery{a},
                      rough ? &fa : nullptr, h->aug.on ? h->gap.ptr : nullptr);
}

// pressure from the nodal area / gap (mortar_contact.cpp:195-261), then pass 2: face residual vectors (+ tangent blocks)
// and their row gather (r_dev null: everything but the gather -- the evaluation of mimi_hip_contact_post_time_advance).
// With mu > 0 the friction kernels add to the face stores behind the frictionless ones and write the trial state.
static void contact_pass2(mimi_hip_contact_s* h, const double* u_dev, double* r_dev, double* A_dev, double gf, bool with_grad) {
  if (with_grad) h->reserve_face_k();
  const ContactArgs a = contact_args(h, u_dev);
  contact_pressure(h);
  // analytic tangent: one wave per face; reference-FD tangent: the face-per-thread kernel
  const bool fd_tangent = with_grad && h->mode == MIMI_HIP_TANGENT_REFERENCE_FD;
  const dim3 waves = face_wave_grid(h->n_faces), wave_threads(kFaceWaveThreads);
  face_dispatch_dim(h->dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    launch(contact_residual_wave_kernel<DIM>, waves, wave_threads, 0, h->stream, a);
    if (fd_tangent) launch(contact_residual_kernel<DIM>, dim3((unsigned)((h->n_faces + 63) / 64)), dim3(64), 0, h->stream, a, 1);
    else if (with_grad) launch(contact_tangent_kernel<DIM>, waves, wave_threads, 0, h->stream, a);
    if (h->mu > 0.0) {
      if (h->mode == MIMI_HIP_TANGENT_REFERENCE_FD) fail("friction has no reference-FD tangent");   // (refused where either is set)
      const FrictionArgs fa = friction_args(h, a);
      launch(contact_friction_kernel<DIM>, waves, wave_threads, 0, h->stream, fa);
      if (with_grad) launch(contact_friction_tangent_kernel<DIM>, waves, wave_threads, 0, h->stream, fa);
    }
  });
  if (h->mu > 0.0) {
    launch(face_sum_kernel, dim3(1), dim3(1024), 0, h->stream, (int64_t)h->n_faces, kFrictionScalars, kFrictionScalars, h->fr_face.ptr,
           (const unsigned char*)nullptr, h->fr_scalars.ptr);
    h->fr_trial = true;
  }
  // pressure integral and force of the active faces (last_pressure_ / last_force_), in a fixed order
  launch(face_sum_kernel, dim3(1), dim3(1024), 0, h->stream, (int64_t)h->n_faces, 1 + h->dim, 1 + h->dim, h->face_scal.ptr,
         (const unsigned char*)h->face_active.ptr, h->scalars.ptr + 1);
  if (r_dev) h->gather(r_dev, A_dev, gf, with_grad);
}

// which: 1 = pass 1 only (u), 2 = pass 2 only (u, r, A), 3 = both (the single-process call)
static void run_contact(mimi_hip_contact_s* h, const double* u, double* r, double* A, double gf, bool with_grad, int which = 3) {
  if ((which & 2) && !r) fail("null vector argument");
  h->run(u, r, A, with_grad, [&](const double* u_dev, double* r_dev, double* A_dev) {
    if (which & 1) contact_pass1(h, u_dev);
    if (which & 2) contact_pass2(h, u_dev, r_dev, A_dev, gf, with_grad);
  });
}

extern "C" {

int mimi_hip_contact_create(const mimi_hip_contact_tables* t, int device, mimi_hip_contact_t* out) {
  return guarded([&] {
    if (!t || !out) fail("null argument");
    const FaceTables ft = face_tables_of(*t);
    auto h = std::make_unique<mimi_hip_contact_s>();
    h->create(ft, device, 64, "marked boundary");
    h->body_kind = t->body_kind;
    for (int i = 0; i < 8; ++i) h->body[i] = t->body[i];
    h->penalty = t->penalty;
    if (t->body_kind == MIMI_HIP_BODY_SPLINE) {
      upload_spline_body(h.get(), t->spline, t->dim);
    } else if (t->body_kind != MIMI_HIP_BODY_SPHERE && t->body_kind != MIMI_HIP_BODY_PLANE) {
      fail("unknown rigid body kind %d", t->body_kind);
    }
    h->area.resize(h->n_fnodes);
    h->gap.resize(h->n_fnodes);
    h->pressure.resize(h->n_fnodes);
    h->scalars.resize(6);
    MH_HIP(hipMemsetAsync(h->pressure.ptr, 0, h->n_fnodes * sizeof(double), h->stream));
    const size_t npts = (size_t)t->n_faces * t->n_quad;
    h->pt_area.resize(npts * t->n_dof);
    h->pt_gap.resize(npts * t->n_dof);
    h->pt_scal.resize(npts);
    h->attach_csr(ft, "marked contact", "contact");
    *out = h.release();
  });
}

int mimi_hip_contact_destroy(mimi_hip_contact_t h) { return handle_destroy(h); }

int mimi_hip_contact_set_tangent_mode(mimi_hip_contact_t h, int mode) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (mode != MIMI_HIP_TANGENT_ANALYTIC && mode != MIMI_HIP_TANGENT_REFERENCE_FD) fail("bad tangent mode %d", mode);
    if (mode == MIMI_HIP_TANGENT_REFERENCE_FD) refuse_friction(h, "the reference-FD tangent mode");
    if (mode == MIMI_HIP_TANGENT_REFERENCE_FD && h->aug.on)
      fail("the reference-FD tangent mode is not available on an augmented contact handle: its tangent is the analytic one");
    h->mode = mode;
  });
}

int mimi_hip_contact_set_stream(mimi_hip_contact_t h, void* stream) { return handle_set_stream(h, stream); }
int mimi_hip_contact_synchronize(mimi_hip_contact_t h) { return handle_synchronize(h); }

int mimi_hip_contact_add_residual(mimi_hip_contact_t h, const double* u, double* r) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_contact(h, u, r, nullptr, 0.0, false);
  });
}

int mimi_hip_contact_add_residual_and_grad(mimi_hip_contact_t h, const double* u, double grad_factor, double* r,
                                           double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_contact(h, u, r, A_values, grad_factor, true);
  });
}

int mimi_hip_contact_linearize(mimi_hip_contact_t h, const double* u) {
  return guarded([&] {
    if (!h) fail("null handle");
    refuse_friction(h, "mimi_hip_contact_linearize", h->friction_action);
    h->run(u, nullptr, nullptr, false, [&](const double* u_dev, double*, double*) { contact_linearize(h, u_dev); });
  });
}

int mimi_hip_contact_apply_tangent(mimi_hip_contact_t h, double factor, const double* x, double* y) {
  return guarded([&] {
    if (h) refuse_friction(h, "mimi_hip_contact_apply_tangent", h->friction_action);
    boundary_apply_entry(h, "contact", factor, x, y);
  });
}

int64_t mimi_hip_contact_action_info(mimi_hip_contact_t h, int what) {
  if (h && what == MIMI_HIP_ACTION_INFO_CONSISTENT) return h->action.linearized && h->action.consistent ? 1 : 0;
  if (h && what == MIMI_HIP_ACTION_INFO_FRICTION) return h->action.linearized && h->action.friction ? 1 : 0;
  if (h && what == MIMI_HIP_ACTION_INFO_AUGMENTED) return h->action.linearized && h->action.augmented ? 1 : 0;
  return boundary_action_info(h, what);
}

int mimi_hip_contact_set_consistent_tangent(mimi_hip_contact_t h, int on) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (on) refuse_friction(h, "the consistent tangent", h->friction_action);
    h->consistent_tangent = on != 0;
  });
}

int mimi_hip_contact_set_friction_action(mimi_hip_contact_t h, int on) {
  return guarded([&] {
    if (!h) fail("null handle");
    h->friction_action = on != 0;
  });
}

int mimi_hip_contact_gap_norm(mimi_hip_contact_t h, const double* u, double* out) {
  return guarded([&] {
    if (!h || !out) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    Mirror<double> mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
    contact_pass1_kernels(h, contact_args(h, mu.dev), 1);
    contact_sum_points(h, 5);
    double g2 = 0;
    MH_HIP(hipMemcpyAsync(&g2, h->scalars.ptr + 5, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    *out = std::sqrt(g2);
  });
}

int mimi_hip_contact_last_history(mimi_hip_contact_t h, double* out5) {
  return guarded([&] {
    if (!h || !out5) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(out5, h->scalars.ptr, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_contact_update_body(mimi_hip_contact_t h, const mimi_hip_spline_body* spline, double penalty) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipStreamSynchronize(h->stream));
    if (spline) {
      if (h->body_kind != MIMI_HIP_BODY_SPLINE) fail("this contact handle has no spline body");
      upload_spline_body(h, spline, h->dim);
      MH_HIP(hipStreamSynchronize(h->stream));
    }
    if (penalty > 0.0) h->penalty = penalty;
  });
}

int mimi_hip_contact_gap_area(mimi_hip_contact_t h, const double* u) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_contact(h, u, nullptr, nullptr, 0.0, false, 1);
  });
}

int mimi_hip_contact_marked_nodes(mimi_hip_contact_t h, int32_t* out, int64_t capacity, int64_t* n) {
  return guarded([&] {
    if (!h) fail("null argument");
    h->copy_fnodes(out, capacity, n);
  });
}

int mimi_hip_contact_nodal(mimi_hip_contact_t h, int set, double* area, double* gap) {
  return guarded([&] {
    if (!h || !area || !gap) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->n_fnodes * sizeof(double);
    if (set) {
      MH_HIP(hipMemcpyAsync(h->area.ptr, area, bytes, hipMemcpyDefault, h->stream));
      MH_HIP(hipMemcpyAsync(h->gap.ptr, gap, bytes, hipMemcpyDefault, h->stream));
    } else {
      MH_HIP(hipMemcpyAsync(area, h->area.ptr, bytes, hipMemcpyDefault, h->stream));
      MH_HIP(hipMemcpyAsync(gap, h->gap.ptr, bytes, hipMemcpyDefault, h->stream));
    }
    if (!is_device_pointer(area) || !is_device_pointer(gap)) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_contact_add_residual_from_nodal(mimi_hip_contact_t h, const double* u, double grad_factor, double* r,
                                             double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_contact(h, u, r, A_values, grad_factor, A_values != nullptr, 2);
  });
}

int mimi_hip_contact_get_pressure(mimi_hip_contact_t h, double* out, int64_t capacity, int64_t* n) {
  return guarded([&] {
    if (!h || !n) fail("null argument");
    *n = h->n_fnodes;
    if (!out) return;
    if (capacity < h->n_fnodes) fail("pressure buffer too small");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(out, h->pressure.ptr, h->n_fnodes * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

// ---- Coulomb friction (kernels_face_friction.hpp) ------------------------------------------------------------------------
int mimi_hip_contact_set_friction(mimi_hip_contact_t h, double mu, double eps_t) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!(mu >= 0.0)) fail("friction coefficient %g: must be >= 0", mu);
    if (mu > 0.0 && !(eps_t > 0.0)) fail("tangential penalty %g: must be > 0 with friction", eps_t);
    if (mu > 0.0 && h->mode == MIMI_HIP_TANGENT_REFERENCE_FD)
      fail("friction (mu = %g) is not available in the reference-FD tangent mode: its tangent is the analytic one", mu);
    MH_HIP(hipSetDevice(h->device));
    if (mu > 0.0 && !h->fr_xi.ptr) friction_reset(h);
    h->mu = mu;
    h->eps_t = eps_t;
  });
}

int mimi_hip_contact_set_body_increment(mimi_hip_contact_t h, const double* d) {
  return guarded([&] {
    if (!h) fail("null handle");
    for (int i = 0; i < 3; ++i) h->body_inc[i] = (d && i < h->dim) ? d[i] : 0.0;
  });
}

int mimi_hip_contact_post_time_advance(mimi_hip_contact_t h, const double* u) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!(h->mu > 0.0)) fail("mimi_hip_contact_post_time_advance: the handle has no friction (set_friction with mu > 0 first)");
    MH_HIP(hipSetDevice(h->device));
    if (!u) {
      if (!h->fr_trial) fail("mimi_hip_contact_post_time_advance(h, NULL): no evaluation since create / reset_friction to commit");
      friction_commit(h);
      return;
    }
    h->run(u, nullptr, nullptr, false, [&](const double* u_dev, double*, double*) {
      contact_pass1(h, u_dev);
      contact_pass2(h, u_dev, nullptr, nullptr, 0.0, false);
      friction_commit(h);
    });
  });
}

int mimi_hip_contact_reset_friction(mimi_hip_contact_t h) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    if (h->fr_xi.ptr) friction_reset(h);
  });
}

int mimi_hip_contact_friction_history(mimi_hip_contact_t h, double* out6) {
  return guarded([&] {
    if (!h || !out6) fail("null argument");
    for (int i = 0; i < kFrictionScalars; ++i) out6[i] = 0.0;
    if (!h->fr_scalars.ptr) return;
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(out6, h->fr_scalars.ptr, kFrictionScalars * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_contact_friction_state(mimi_hip_contact_t h, double* xi, double* xbar, unsigned char* c) {
  return guarded([&] {
    if (!h) fail("null handle");
    const size_t n_q = h->n_q, dim = h->dim, npts = (size_t)h->n_faces * n_q;
    if (!h->fr_xi.ptr) {   // never had friction: the initial state
      for (size_t k = 0; k < npts * dim; ++k) {
        if (xi) xi[k] = 0.0;
        if (xbar) xbar[k] = 0.0;
      }
      for (size_t k = 0; c && k < npts; ++k) c[k] = 0;
      return;
    }
    MH_HIP(hipSetDevice(h->device));
    std::vector<double> a(npts * dim), b(npts * dim);
    MH_HIP(hipMemcpyAsync(a.data(), h->fr_xi.ptr, a.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipMemcpyAsync(b.data(), h->fr_xbar.ptr, b.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (c) MH_HIP(hipMemcpyAsync(c, h->fr_c.ptr, npts, hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    // device [face][i][q] -> caller [face][q][i]
    for (size_t f = 0; f < (size_t)h->n_faces; ++f)
      for (size_t i = 0; i < dim; ++i)
        for (size_t q = 0; q < n_q; ++q) {
          if (xi) xi[(f * n_q + q) * dim + i] = a[(f * dim + i) * n_q + q];
          if (xbar) xbar[(f * n_q + q) * dim + i] = b[(f * dim + i) * n_q + q];
        }
  });
}

// ---- augmented-Lagrangian mode (kernels_face_augmented.hpp) ---------------------------------------------------------------
int mimi_hip_contact_set_augmented(mimi_hip_contact_t h, int on) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (on && h->mode == MIMI_HIP_TANGENT_REFERENCE_FD)
      fail("the augmented mode is not available in the reference-FD tangent mode: its tangent is the analytic one");
    MH_HIP(hipSetDevice(h->device));
    h->aug.set(*h, on != 0);
  });
}

int mimi_hip_contact_lagrange(mimi_hip_contact_t h, int set, double* lambda) {
  return guarded([&] {
    if (!h || !lambda) fail("null argument");
    if (!h->aug.lambda.ptr) fail("mimi_hip_contact_lagrange: the handle was never set to the augmented mode (set_augmented first)");
    MH_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->n_fnodes * sizeof(double);
    if (set) {
      MH_HIP(hipMemcpyAsync(h->aug.lambda.ptr, lambda, bytes, hipMemcpyDefault, h->stream));
      h->aug.project(*h);
    } else {
      MH_HIP(hipMemcpyAsync(lambda, h->aug.lambda.ptr, bytes, hipMemcpyDefault, h->stream));
    }
    if (!is_device_pointer(lambda)) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_contact_update_lagrange(mimi_hip_contact_t h, const double* u, int apply, double* out4) {
  return guarded([&] {
    if (!h || !out4) fail("null argument");
    if (!h->aug.on) fail("mimi_hip_contact_update_lagrange: the handle is not in the augmented mode (set_augmented first)");
    h->run(u, nullptr, nullptr, false, [&](const double* u_dev, double*, double*) {
      // pass 1 as contact_linearize runs it: the history scalars of the last Add* call are left alone
      contact_pass1_kernels(h, contact_args(h, u_dev), 0);
      h->aug.update(*h, h->area.ptr, h->gap.ptr, h->penalty, apply != 0);
    });
    MH_HIP(hipMemcpyAsync(out4, h->aug.out4.ptr, kAugmentedNodeScalars * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"
