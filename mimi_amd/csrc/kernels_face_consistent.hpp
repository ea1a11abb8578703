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
//   action   face rates   one wave per face.  Lane = point: dx_q, dt, dm, n.dm, a_q = w (n.dm),
//                         b_q = w ((n.dm) g_q + |m| chi nu.dx_q); lane = local node c: face_dA[f][c] = sum_q a_q N_q[c],
//                         face_dG[f][c] = sum_q b_q N_q[c] over the points in ascending order
//            nodal        one thread per marked node: the sums over its incidences in the order of adj, dp_l
//            face action  stage 1 and 2 of boundary_action_kernel with g_i = c_q dm_i - w dp_q m_i
//            node sum     face_row_gather_kernel<DIM, 0> over the recorded flags
// One wave per face, four faces per workgroup, no LDS, no atomics: equal inputs give equal bytes.  The action's kernels run in
// registers only; the record kernel keeps the private arrays of the spline search in scratch, as pass 1 does.
// The stages of the face kernels (wave index, node load, point stage, normal rate, point scatter) are face_wave.hpp's.
// A handle in the mode "augmented" (kernels_face_augmented.hpp) records with the launch flag `augmented`: g_q is the unclamped
// gap, chi_q = "the angle rule accepted the point", and dp_l = eps (dG_l - gt_l dA_l) / A_l, gt_l = G_l / A_l, on the nodes with
// p_l < 0 and 0 on the others -- the derivative of p_l = min(0, lambda_l + eps gt_l).  The record keeps G_l for it (the nodal
// kernel's `gap`, null in penalty mode); lambda_l is not needed.  Both flags are uniform over a launch, and their off-branches
// are the penalty law's text.
// Only contact.hip includes this header.
#pragma once

#include "kernels_face_action.hpp"

namespace mimi_hip {
namespace {

struct ConsistentRecordArgs {
  FaceView v;
  const double* u;
  const double* pressure;    // [n_marked] of the linearisation
  double* gq;                // [n_faces][n_q]        g_q
  double* chinu;             // [n_faces][n_q][dim]   chi_q nu_q
  int augmented;             // the unclamped gap, chi_q = accepted by the angle rule
};

// Body: nearest<DIM>(xq, true_g, distance, nu) -- the closest-point query of pass 1 with the body's unit normal.  (Four
// waves per SIMD asked for: left to a whole SIMD's registers the compiler keeps the spline search's arrays in 255 vector and
// 202 accumulator registers at one wave per SIMD; so they sit in scratch as in contact_gap_area_kernel, at 63 registers.)
template<int DIM, class Body>
__global__ __launch_bounds__(kFaceWaveThreads, 4) void contact_consistent_record_kernel(ConsistentRecordArgs p, Body body) {
  int lane, f;
  if (!face_wave_index(p.v, lane, f)) return;
  double xc[DIM];
  const double pc = face_load_nodes<DIM, true, kNodal>(p.v, f, lane, p.u, xc, p.pressure);
  if (__ballot(pc != 0.0) == 0) return;   // IsPressureZero: the flag boundary_linearize_kernel records
  // lane = point: x_q in the accumulation order of contact_gap_area_kernel (face_wave.hpp's contract), hence the same g_q
  const int64_t pt = face_lane_point(p.v, f, lane);
  double xq[DIM];
  face_point_stage<DIM, false, true, false>(p.v, pt, 0.0, xc, nullptr, xq, nullptr);
  double true_g, distance, nu[DIM];
  body.template nearest<DIM>(xq, true_g, distance, nu);
  const bool aug = p.augmented != 0;
  double g = (aug || true_g < 0.) ? true_g : 0.;
  const double ratio = fabs(true_g) / distance;
  const bool rejected = acos(ratio < 1. ? ratio : 1.) > 1.e-5;   // angle tolerance, mortar_contact.cpp:172-181
  if (rejected) g = 0.0;
  if (lane < p.v.n_q) {
    p.gq[pt] = g;
    const bool chi = aug ? !rejected : g != 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) p.chinu[pt * DIM + i] = chi ? nu[i] : 0.0;
  }
}

struct ConsistentRatesArgs {
  FaceView v;
  const double* tang;
  const double* gq;
  const double* chinu;
  const unsigned char* active;
  const double* x;
  double* face_dA;           // [n_faces][n_dof]
  double* face_dG;           // [n_faces][n_dof]
};

template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_consistent_rates_kernel(ConsistentRatesArgs p) {
  int lane, f;
  if (!face_wave_index(p.v, lane, f)) return;
  if (!p.active[f]) return;   // (wave-uniform; the nodal sum skips the face)
  const int n_dof = p.v.n_dof, n_q = p.v.n_q;
  double xc[DIM];
  face_load_nodes<DIM, false>(p.v, f, lane, p.x, xc);
  const int kc = lane < n_dof ? lane : 0;
  // stage 1, lane = point: a_q, b_q
  const bool on = lane < n_q;
  const int64_t pt = face_lane_point(p.v, f, lane);
  double dx[DIM], dt[(DIM - 1) * DIM], t[(DIM - 1) * DIM], m[DIM], dm[DIM];
  face_recorded_tangents<DIM>(p.tang, pt, t);
  face_point_stage<DIM, false, true, true>(p.v, pt, 0.0, xc, nullptr, dx, dt);
  face_normal_rate<DIM>(t, dt, m, dm);
  double mm = 0.0, mdm = 0.0, nudx = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    mm += m[i] * m[i];
    mdm += m[i] * dm[i];
    nudx += p.chinu[pt * DIM + i] * dx[i];
  }
  const double len = sqrt(mm), ndm = mdm / len, w = p.v.weight[pt];
  const double aq = on ? w * ndm : 0.0, bq = on ? w * (ndm * p.gq[pt] + len * nudx) : 0.0;
  // stage 2, lane = local node: the points in ascending order
  double dA = 0.0, dG = 0.0;
  for (int q = 0; q < n_q; ++q) {
    const double Nc = p.v.N[((int64_t)f * n_q + q) * n_dof + kc];
    dA = __builtin_fma(face_lane_read(aq, q), Nc, dA);
    dG = __builtin_fma(face_lane_read(bq, q), Nc, dG);
  }
  if (lane < n_dof) {
    p.face_dA[(int64_t)f * n_dof + lane] = dA;
    p.face_dG[(int64_t)f * n_dof + lane] = dG;
  }
}

// dp_l = (eps dG_l - p_l dA_l) / A_l, one thread per marked node: its incidences in the order of adj, as contact_nodal_kernel
// and the row gather walk them; the faces the record holds inactive wrote nothing and add nothing
// (gap != nullptr, a record of the augmented mode: `pressure` decides the node's branch and `gap` is the recorded G_l)
__global__ __launch_bounds__(256) void contact_consistent_nodal_kernel(int n_marked, int n_dof, const int32_t* __restrict__ adj_ptr,
                                                                       const int32_t* __restrict__ adj,
                                                                       const unsigned char* __restrict__ active,
                                                                       const double* __restrict__ face_dA,
                                                                       const double* __restrict__ face_dG,
                                                                       const double* __restrict__ area,
                                                                       const double* __restrict__ pressure,
                                                                       const double* __restrict__ gap, double penalty,
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
  if (gap) {
    dp[l] = pressure[l] < 0.0 ? (penalty * sG - gap[l] / area[l] * penalty * sA) / area[l] : 0.0;
  } else {
    dp[l] = (penalty * sG - pressure[l] * sA) / area[l];
  }
}

struct ConsistentActionArgs {
  FaceView v;
  const double* coef;
  const double* tang;
  const unsigned char* active;
  const double* dp;          // [n_marked]
  double factor;
  const double* x;
  double* face_y;            // [n_faces][dim][n_dof]
};

template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void contact_consistent_action_kernel(ConsistentActionArgs p) {
  int lane, f;
  if (!face_wave_index(p.v, lane, f)) return;
  if (!p.active[f]) return;   // (wave-uniform; the node sum skips the face)
  double xc[DIM];
  const double dpc = face_load_nodes<DIM, false, kNodal>(p.v, f, lane, p.x, xc, p.dp);
  const FaceEntry e = face_lane_entry<DIM>(p.v, lane);
  // stage 1, lane = point: g = c_q dm - w dp_q m
  const bool on = lane < p.v.n_q;
  const int64_t pt = face_lane_point(p.v, f, lane);
  double g[DIM], dpq, dt[(DIM - 1) * DIM], t[(DIM - 1) * DIM], m[DIM], dm[DIM];
  face_recorded_tangents<DIM>(p.tang, pt, t);
  face_point_stage<DIM, true, false, true>(p.v, pt, dpc, xc, &dpq, nullptr, dt);
  face_normal_rate<DIM>(t, dt, m, dm);
  const double cq = on ? p.coef[pt] : 0.0, wdp = on ? p.v.weight[pt] * dpq : 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) g[i] = cq * dm[i] - wdp * m[i];
  // stage 2, lane = (i, a)
  const double Y = face_scatter_points<DIM, true>(p.v, f, e, g);
  const int NT = p.v.n_dof * DIM;
  if (lane < NT) p.face_y[(int64_t)f * NT + lane] = p.factor * Y;   // [i][a]
}

// The record of a contact handle: BoundaryAction's, and on top of it the consistent part when the linearisation that made
// it was asked for one.  `consistent` is the record's own mode flag: what the handle is set to reaches it at the next
// linearize only.  With the flag off none of the buffers below exists and begin / add are BoundaryAction's.
struct ContactAction : BoundaryAction {
  bool consistent = false;
  bool augmented = false;                          // the handle's mode at the linearisation
  double penalty = 0.0;                            // of the linearisation
  DeviceBuffer<double> gq, chinu, area, pressure;  // the record on top of coef / tang / active
  DeviceBuffer<double> gap;                        // G_l (a consistent record of the augmented mode)
  DeviceBuffer<double> face_dA, face_dG, dp;       // what the action builds on first use, like face_y

  int64_t bytes(const FaceSet& h) const {
    int64_t n = BoundaryAction::bytes(h);
    if (linearized && consistent) n += (int64_t)h.n_faces * h.n_q * (1 + h.dim) * (int64_t)sizeof(double) + 16 * (int64_t)h.n_fnodes;
    if (linearized && consistent && augmented) n += 8 * (int64_t)h.n_fnodes;
    return n;
  }

  // the snapshot at u_dev on the handle's stream: the consistent part first (on), then BoundaryAction::linearize, whose
  // event then stands behind both.  area_now / pressure_now [n_marked]: the handle's nodal values at u_dev; gap_now: the
  // nodal sums G_l of the augmented mode, or nullptr (the handle is in penalty mode)
  template<class Body>
  void linearize(FaceSet& h, const double* u_dev, const double* area_now, const double* pressure_now, double penalty_now, bool on,
                 const Body& body, const double* gap_now = nullptr) {
    augmented = gap_now != nullptr;
    if (on) {
      const size_t npts = (size_t)h.n_faces * h.n_q, nb = (size_t)h.n_fnodes * sizeof(double);
      gq.resize(npts);
      chinu.resize(npts * h.dim);
      area.resize((size_t)h.n_fnodes);
      pressure.resize((size_t)h.n_fnodes);
      MH_HIP(hipMemcpyAsync(area.ptr, area_now, nb, hipMemcpyDeviceToDevice, h.stream));
      MH_HIP(hipMemcpyAsync(pressure.ptr, pressure_now, nb, hipMemcpyDeviceToDevice, h.stream));
      if (augmented) {
        gap.resize((size_t)h.n_fnodes);
        MH_HIP(hipMemcpyAsync(gap.ptr, gap_now, nb, hipMemcpyDeviceToDevice, h.stream));
      }
      const ConsistentRecordArgs a{h.view(), u_dev, pressure_now, gq.ptr, chinu.ptr, augmented ? 1 : 0};
      face_dispatch_dim(h.dim, [&](auto D) {
        launch(contact_consistent_record_kernel<decltype(D)::value, Body>, face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0,
               h.stream, a, body);
      });
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
    const ConsistentRatesArgs r{h.view(), tang.ptr, gq.ptr, chinu.ptr, active.ptr, x, face_dA.ptr, face_dG.ptr};
    face_dispatch_dim(h.dim, [&](auto D) {
      launch(contact_consistent_rates_kernel<decltype(D)::value>, face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0, s, r);
    });
    launch(contact_consistent_nodal_kernel, dim3((unsigned)((h.n_fnodes + 255) / 256)), dim3(256), 0, s, h.n_fnodes, h.n_dof,
           h.adj_ptr.ptr, h.adj.ptr, active.ptr, face_dA.ptr, face_dG.ptr, area.ptr, pressure.ptr,
           (const double*)(augmented ? gap.ptr : nullptr), penalty, dp.ptr);
  }

  // y += factor K x over the recorded active faces, K the frozen or the consistent tangent as the record says
  void add(FaceAssembly& h, double factor, const double* x, double* y, hipStream_t s) {
    if (!consistent) {
      BoundaryAction::add(h, factor, x, y, s);
      return;
    }
    nodal_rates(h, x, s);
    const ConsistentActionArgs a{h.view(), coef.ptr, tang.ptr, active.ptr, dp.ptr, factor, x, face_y.ptr};
    face_dispatch_dim(h.dim, [&](auto D) {
      launch(contact_consistent_action_kernel<decltype(D)::value>, face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0, s, a);
    });
    h.gather_vector(active.ptr, face_y.ptr, y, s);
  }
};

}  // namespace
}  // namespace mimi_hip
