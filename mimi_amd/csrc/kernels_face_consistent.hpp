// The CONSISTENT mortar-contact tangent as a matrix-free action: kernels_face_action.hpp's frozen-pressure action plus the
// derivative of the nodal pressure p_i = eps G_i / A_i, which the reference's finite-difference Jacobian freezes
// (mortar_contact.cpp:281-294).  That term couples node a to every node that shares a face with a node that shares a face
// with a -- up to 2 p basis functions away per axis, outside the structured CSR pattern -- so it exists as an action only.
//   r(a,i)   = -sum_q w p_q N_a m_i,   p_q = sum_i N_i p_i,   A_i = sum_q w |m| N_i,   G_i = sum_q w |m| g_q N_i
//   dr(a,i)  = -sum_q w p_q N_a dm_i                  (frozen: the action of kernels_face_action.hpp)
//              -sum_q w dp_q N_a m_i                  (new)
//   dp_q = sum_i N_i dp_i,   dp_i = (eps dG_i - p_i dA_i) / A_i
//   dA_i = sum_q w (n.dm) N_i,   dG_i = sum_q w ((n.dm) g_q + |m| chi_q nu_q.dx_q) N_i,   dx_q = sum_b N_b v_b
// with g_q pass 1's gap (after min(., 0) and the angle rule), chi_q = [g_q != 0] and nu_q the body's unit normal at the
// closest point (the gradient of the gap).  The active set is frozen: the action is the exact derivative of the residual
// wherever no point sits on a switch.  A face whose nodal pressures are all zero has no chi point and its dA_i meet
// p_i = 0, so the recorded flags of the frozen record decide which faces run here as well.
//   record   on top of coef / tang / active (written by boundary_linearize_kernel as ever): per point g_q and chi_q nu_q,
//            per marked node A_i and p_i (copies: later evaluations overwrite the handle's), the penalty of that moment
//   action   face rates   one wave per face.  Lane = point (trips of 64): dx_q, dt, dm, n.dm, a_q = w (n.dm),
//                         b_q = w ((n.dm) g_q + |m| chi nu.dx_q); lane = local node c: face_dA[f][c] = sum_q a_q N_q[c],
//                         face_dG[f][c] = sum_q b_q N_q[c] over the points in ascending order
//            nodal        one thread per marked node: the sums over its incidences in the order of adj, dp_l
//            face action  stage 1 and 2 of boundary_action_kernel with g_i = c_q dm_i - w dp_q m_i
//            node sum     face_row_gather_kernel<DIM, 0> over the recorded flags
// One wave per face, four faces per workgroup, no LDS, no atomics: equal inputs give equal bytes.  The action's kernels run in
// registers only; the record kernel keeps the private arrays of the spline search in scratch, as pass 1 does.
// Only contact.hip includes this header.
#pragma once

#include "kernels_face_action.hpp"

namespace mimi_hip {
namespace {

struct ConsistentRecordArgs {
  int n_faces, n_dof, n_q;
  const int32_t* dofs;
  const int32_t* local;
  const double* N;
  const double* x_ref;
  const double* u;
  const double* pressure;    // [n_marked] of the linearisation
  double* gq;                // [n_faces][n_q]        g_q
  double* chinu;             // [n_faces][n_q][dim]   chi_q nu_q
};

// Body: nearest<DIM>(xq, true_g, distance, nu) -- the closest-point query of pass 1 with the body's unit normal.  (Four
// waves per SIMD asked for: left to a whole SIMD's registers the compiler keeps the spline search's arrays in 255 vector and
// 202 accumulator registers at one wave per SIMD; so they sit in scratch as in contact_gap_area_kernel, at 63 registers.)
template<int DIM, class Body>
__global__ __launch_bounds__(256, 4) void contact_consistent_record_kernel(ConsistentRecordArgs p, Body body) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n_faces) return;
  const int n_dof = p.n_dof, n_q = p.n_q;
  double pc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    pc = p.pressure[p.local[(int64_t)f * n_dof + lane]];
    const int64_t node = p.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.u[node * DIM + i] + p.x_ref[node * DIM + i];
  }
  if (__ballot(pc != 0.0) == 0) return;   // IsPressureZero: the flag boundary_linearize_kernel records
  // lane = point (a contact face holds at most a wave's 64: checked at create)
  const bool on = lane < n_q;
  const int64_t pt = (int64_t)f * n_q + (on ? lane : 0);
  const double* N = p.N + pt * n_dof;
  double xq[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xq[i] = 0.0;
  for (int c = 0; c < n_dof; ++c) {     // (the order of contact_gap_area_kernel: the same x_q, hence the same g_q)
#pragma unroll
    for (int i = 0; i < DIM; ++i) xq[i] = __builtin_fma(face_lane_read(xc[i], c), N[c], xq[i]);
  }
  double true_g, distance, nu[DIM];
  body.template nearest<DIM>(xq, true_g, distance, nu);
  double g = true_g < 0. ? true_g : 0.;
  const double ratio = fabs(true_g) / distance;
  if (acos(ratio < 1. ? ratio : 1.) > 1.e-5) g = 0.0;   // angle tolerance, mortar_contact.cpp:172-181
  if (on) {
    p.gq[pt] = g;
#pragma unroll
    for (int i = 0; i < DIM; ++i) p.chinu[pt * DIM + i] = g != 0.0 ? nu[i] : 0.0;
  }
}

struct ConsistentRatesArgs {
  int n_faces, n_dof, n_q;
  const int32_t* dofs;
  const double* N;
  const double* dN;
  const double* weight;
  const double* tang;
  const double* gq;
  const double* chinu;
  const unsigned char* active;
  const double* x;
  double* face_dA;           // [n_faces][n_dof]
  double* face_dG;           // [n_faces][n_dof]
};

// dm of the direction's tangents dt at the recorded tangents t, and m itself
template<int DIM>
MH_DEV void consistent_normal_rate(const double* t, const double* dt, double* m, double* dm) {
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

template<int DIM>
__global__ __launch_bounds__(256) void contact_consistent_rates_kernel(ConsistentRatesArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n_faces) return;
  if (!p.active[f]) return;   // (wave-uniform; the nodal sum skips the face)
  const int n_dof = p.n_dof, n_q = p.n_q;
  double xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    const int64_t node = p.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.x[node * DIM + i];
  }
  const int kc = lane < n_dof ? lane : 0;
  double dA = 0.0, dG = 0.0;
  for (int q0 = 0; q0 < n_q; q0 += 64) {
    // stage 1, lane = point q0 + lane: a_q, b_q
    double aq, bq;
    {
      const bool on = q0 + lane < n_q;
      const int64_t pt = (int64_t)f * n_q + (on ? q0 + lane : 0);
      const double* N = p.N + pt * n_dof;
      const double* dN = p.dN + pt * n_dof * (DIM - 1);
      double dx[DIM], dt[(DIM - 1) * DIM], t[(DIM - 1) * DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) dx[i] = 0.0;
#pragma unroll
      for (int kk = 0; kk < (DIM - 1) * DIM; ++kk) {
        dt[kk] = 0.0;
        t[kk] = p.tang[pt * ((DIM - 1) * DIM) + kk];
      }
      for (int c = 0; c < n_dof; ++c) {
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          const double x = face_lane_read(xc[i], c);
          dx[i] = __builtin_fma(x, N[c], dx[i]);
#pragma unroll
          for (int kk = 0; kk < DIM - 1; ++kk) dt[kk * DIM + i] = __builtin_fma(x, dN[kk * n_dof + c], dt[kk * DIM + i]);
        }
      }
      double m[DIM], dm[DIM];
      consistent_normal_rate<DIM>(t, dt, m, dm);
      double mm = 0.0, mdm = 0.0, nudx = 0.0;
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        mm += m[i] * m[i];
        mdm += m[i] * dm[i];
        nudx += p.chinu[pt * DIM + i] * dx[i];
      }
      const double len = sqrt(mm), ndm = mdm / len, w = p.weight[pt];
      aq = on ? w * ndm : 0.0;
      bq = on ? w * (ndm * p.gq[pt] + len * nudx) : 0.0;
    }
    // stage 2, lane = local node: the trip's points in ascending order
    const int n_trip = n_q - q0 < 64 ? n_q - q0 : 64;
    for (int q = 0; q < n_trip; ++q) {
      const double Nc = p.N[((int64_t)f * n_q + q0 + q) * n_dof + kc];
      dA = __builtin_fma(face_lane_read(aq, q), Nc, dA);
      dG = __builtin_fma(face_lane_read(bq, q), Nc, dG);
    }
  }
  if (lane < n_dof) {
    p.face_dA[(int64_t)f * n_dof + lane] = dA;
    p.face_dG[(int64_t)f * n_dof + lane] = dG;
  }
}

// dp_l = (eps dG_l - p_l dA_l) / A_l, one thread per marked node: its incidences in the order of adj, as contact_nodal_kernel
// and the row gather walk them; the faces the record holds inactive wrote nothing and add nothing
__global__ __launch_bounds__(256) void contact_consistent_nodal_kernel(int n_marked, int n_dof, const int32_t* __restrict__ adj_ptr,
                                                                       const int32_t* __restrict__ adj,
                                                                       const unsigned char* __restrict__ active,
                                                                       const double* __restrict__ face_dA,
                                                                       const double* __restrict__ face_dG,
                                                                       const double* __restrict__ area,
                                                                       const double* __restrict__ pressure, double penalty,
                                                                       double* __restrict__ dp) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_marked) return;
  double sA = 0.0, sG = 0.0;
  for (int t = adj_ptr[l]; t < adj_ptr[l + 1]; ++t) {
    const int ea = adj[t];
    const int64_t f = ea >> 6;
    if (!active[f]) continue;
    sA += face_dA[f * n_dof + (ea & 63)];
    sG += face_dG[f * n_dof + (ea & 63)];
  }
  dp[l] = (penalty * sG - pressure[l] * sA) / area[l];
}

struct ConsistentActionArgs {
  int n_faces, n_dof, n_q;
  const int32_t* dofs;
  const int32_t* local;
  const double* N;
  const double* dN;
  const double* weight;
  const double* coef;
  const double* tang;
  const unsigned char* active;
  const double* dp;          // [n_marked]
  double factor;
  const double* x;
  double* face_y;            // [n_faces][dim][n_dof]
};

template<int DIM>
__global__ __launch_bounds__(256) void contact_consistent_action_kernel(ConsistentActionArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n_faces) return;
  if (!p.active[f]) return;   // (wave-uniform; the node sum skips the face)
  const int n_dof = p.n_dof, n_q = p.n_q, NT = n_dof * DIM;
  double dpc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    dpc = p.dp[p.local[(int64_t)f * n_dof + lane]];
    const int64_t node = p.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.x[node * DIM + i];
  }
  const int k = lane < NT ? lane : 0, ki = k / n_dof, ka = k % n_dof;
  double Y = 0.0;
  for (int q0 = 0; q0 < n_q; q0 += 64) {
    // stage 1, lane = point q0 + lane: g = c_q dm - w dp_q m
    double g[DIM];
    {
      const bool on = q0 + lane < n_q;
      const int64_t pt = (int64_t)f * n_q + (on ? q0 + lane : 0);
      const double* N = p.N + pt * n_dof;
      const double* dN = p.dN + pt * n_dof * (DIM - 1);
      double dpq = 0.0, dt[(DIM - 1) * DIM], t[(DIM - 1) * DIM];
#pragma unroll
      for (int kk = 0; kk < (DIM - 1) * DIM; ++kk) {
        dt[kk] = 0.0;
        t[kk] = p.tang[pt * ((DIM - 1) * DIM) + kk];
      }
      for (int c = 0; c < n_dof; ++c) {
        dpq = __builtin_fma(N[c], face_lane_read(dpc, c), dpq);
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          const double x = face_lane_read(xc[i], c);
#pragma unroll
          for (int kk = 0; kk < DIM - 1; ++kk) dt[kk * DIM + i] = __builtin_fma(x, dN[kk * n_dof + c], dt[kk * DIM + i]);
        }
      }
      double m[DIM], dm[DIM];
      consistent_normal_rate<DIM>(t, dt, m, dm);
      const double cq = on ? p.coef[pt] : 0.0, wdp = on ? p.weight[pt] * dpq : 0.0;
#pragma unroll
      for (int i = 0; i < DIM; ++i) g[i] = cq * dm[i] - wdp * m[i];
    }
    // stage 2, lane = (i, a): the trip's points in ascending order
    const int n_trip = n_q - q0 < 64 ? n_q - q0 : 64;
    for (int q = 0; q < n_trip; ++q) {
      double gi = face_lane_read(g[0], q);
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double v = face_lane_read(g[ii], q);
        gi = ki == ii ? v : gi;
      }
      Y = __builtin_fma(gi, p.N[((int64_t)f * n_q + q0 + q) * n_dof + ka], Y);
    }
  }
  if (lane < NT) p.face_y[(int64_t)f * NT + lane] = p.factor * Y;   // [i][a]
}

// The record of a contact handle: BoundaryAction's, and on top of it the consistent part when the linearisation that made
// it was asked for one.  `consistent` is the record's own mode flag: what the handle is set to reaches it at the next
// linearize only.  With the flag off none of the buffers below exists and begin / add are BoundaryAction's.
struct ContactAction : BoundaryAction {
  bool consistent = false;
  double penalty = 0.0;                            // of the linearisation
  DeviceBuffer<double> gq, chinu, area, pressure;  // the record on top of coef / tang / active
  DeviceBuffer<double> face_dA, face_dG, dp;       // what the action builds on first use, like face_y

  int64_t bytes(const FaceSet& h) const {
    int64_t n = BoundaryAction::bytes(h);
    if (linearized && consistent) n += (int64_t)h.n_faces * h.n_q * (1 + h.dim) * (int64_t)sizeof(double) + 16 * (int64_t)h.n_fnodes;
    return n;
  }

  // the snapshot at u_dev on the handle's stream: the consistent part first (on), then BoundaryAction::linearize, whose
  // event then stands behind both.  area_now / pressure_now [n_marked]: the handle's nodal values at u_dev
  template<class Body>
  void linearize(FaceSet& h, const double* u_dev, const double* area_now, const double* pressure_now, double penalty_now, bool on,
                 const Body& body) {
    if (on) {
      const size_t npts = (size_t)h.n_faces * h.n_q, nb = (size_t)h.n_fnodes * sizeof(double);
      gq.resize(npts);
      chinu.resize(npts * h.dim);
      area.resize((size_t)h.n_fnodes);
      pressure.resize((size_t)h.n_fnodes);
      MH_HIP(hipMemcpyAsync(area.ptr, area_now, nb, hipMemcpyDeviceToDevice, h.stream));
      MH_HIP(hipMemcpyAsync(pressure.ptr, pressure_now, nb, hipMemcpyDeviceToDevice, h.stream));
      const ConsistentRecordArgs a{h.n_faces, h.n_dof, h.n_q, h.dofs.ptr, h.local.ptr, h.N.ptr, h.x_ref.ptr, u_dev, pressure_now, gq.ptr, chinu.ptr};
      const dim3 grid((unsigned)((h.n_faces + 3) / 4));
      if (h.dim == 2) launch(contact_consistent_record_kernel<2, Body>, grid, dim3(256), 0, h.stream, a, body);
      else launch(contact_consistent_record_kernel<3, Body>, grid, dim3(256), 0, h.stream, a, body);
      penalty = penalty_now;
    }
    consistent = on;
    BoundaryAction::linearize(h, u_dev, pressure_now, 0.0, -1.0);
  }

  void begin(FaceSet& h, hipStream_t s) {
    BoundaryAction::begin(h, s);
    if (!consistent) return;
    face_dA.resize((size_t)h.n_faces * h.n_dof);
    face_dG.resize((size_t)h.n_faces * h.n_dof);
    dp.resize((size_t)h.n_fnodes);
  }

  // dp [n_marked] of the direction x: the face rates and the nodal sums (a consistent record)
  void nodal_rates(FaceAssembly& h, const double* x, hipStream_t s) {
    const dim3 grid((unsigned)((h.n_faces + 3) / 4));
    const ConsistentRatesArgs r{h.n_faces, h.n_dof,   h.n_q,      h.dofs.ptr, h.N.ptr, h.dN.ptr,    h.weight.ptr,
                                tang.ptr,  gq.ptr,    chinu.ptr,  active.ptr, x,       face_dA.ptr, face_dG.ptr};
    if (h.dim == 2) launch(contact_consistent_rates_kernel<2>, grid, dim3(256), 0, s, r);
    else launch(contact_consistent_rates_kernel<3>, grid, dim3(256), 0, s, r);
    launch(contact_consistent_nodal_kernel, dim3((unsigned)((h.n_fnodes + 255) / 256)), dim3(256), 0, s, h.n_fnodes, h.n_dof,
           h.adj_ptr.ptr, h.adj.ptr, active.ptr, face_dA.ptr, face_dG.ptr, area.ptr, pressure.ptr, penalty, dp.ptr);
  }

  // y += factor K x over the recorded active faces, K the frozen or the consistent tangent as the record says
  void add(FaceAssembly& h, double factor, const double* x, double* y, hipStream_t s) {
    if (!consistent) {
      BoundaryAction::add(h, factor, x, y, s);
      return;
    }
    nodal_rates(h, x, s);
    const dim3 grid((unsigned)((h.n_faces + 3) / 4));
    const ConsistentActionArgs a{h.n_faces, h.n_dof,  h.n_q,      h.dofs.ptr, h.local.ptr, h.N.ptr, h.dN.ptr,   h.weight.ptr,
                                 coef.ptr,  tang.ptr, active.ptr, dp.ptr,     factor,      x,       face_y.ptr};
    if (h.dim == 2) launch(contact_consistent_action_kernel<2>, grid, dim3(256), 0, s, a);
    else launch(contact_consistent_action_kernel<3>, grid, dim3(256), 0, s, a);
    if (h.dim == 2) h.template gather_vector<2>(active.ptr, face_y.ptr, y, s);
    else h.template gather_vector<3>(active.ptr, face_y.ptr, y, s);
    MH_HIP(hipGetLastError());
  }
};

}  // namespace
}  // namespace mimi_hip
