// The matrix-free action of the two face tangents -- contact.hip (frozen nodal pressure, mortar_contact.cpp:263-295) and
// pressure.hip (follower pressure) -- without the per-face (n_dof dim)^2 blocks.  Both residuals are c_q N_a m_i with m the
// non-normalised normal of face_common.hpp (c_q = -w p_q for contact, contact.hip "analytic frozen-pressure tangent";
// c_q = w p_q for the follower load, pressure.hip), so both tangents are c_q N_a dm_i/dx_bj and
//   (K_face x)(a, i) = sum_q c_q N_a dm_i,   dm = dt_1 x t_2 + t_1 x dt_2 (3-D), (dt_y, -dt_x) (2-D),   dt_k = sum_b N_b,k x_b.
// Stands in for MortarContact::AddBoundaryResidualAndGrad (mortar_contact.cpp:353-421) followed by SparseMatrix::Mult.
//   linearize  one wave per face: per point c_q and the surface tangents t at u, per face the active flag -- the record
//              (n_faces n_q (1 + (dim - 1) dim) doubles + n_faces bytes); nothing of u is kept
//   action     one wave per face, four per workgroup.  Lane c holds node c's x, handed round by face_lane_read.  Stage 1,
//              lane = point (trips of 64): dt, dm, g = c_q dm.  Stage 2, lane = (i, a): y_f(a, i) += g_i(q) N_q[a] over the
//              trip's points in ascending order, so the bytes do not depend on the launch.  face_y [n_faces][dim][n_dof] is
//              a buffer of the record's owner, not the assembly's face_r.
//   node sum   face_row_gather_kernel<DIM, 0> over the RECORDED flags, in the order of the incidences.  No atomics.
// Registers only: the kernels are latency-bound like the face gather (face_common.hpp) and spend no LDS.
#pragma once

#include "face_common.hpp"

namespace mimi_hip {
namespace {

struct BoundaryLinearizeArgs {
  int n_faces, n_dof, n_q;
  const int32_t* dofs;       // [n_faces][n_dof] global node ids
  const int32_t* local;      // [n_faces][n_dof] index into `nodal`
  const double* N;           // [n_faces][n_q][n_dof]
  const double* dN;          // [n_faces][n_q][dim-1][n_dof]
  const double* weight;      // [n_faces][n_q]
  const double* x_ref;       // [n_nodes][dim]
  const double* u;
  const double* nodal;       // values at the face nodes, or nullptr: `value` everywhere
  double value;
  double sign;               // -1 contact, +1 follower pressure
  double* coef;              // [n_faces][n_q]               c_q = sign w p_q
  double* tang;              // [n_faces][n_q][dim-1][dim]   t at u
  unsigned char* active;     // [n_faces]                    some nodal value of the face is not zero (IsPressureZero)
};

template<int DIM>
__global__ __launch_bounds__(256) void boundary_linearize_kernel(BoundaryLinearizeArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n_faces) return;
  const int n_dof = p.n_dof, n_q = p.n_q;
  double pc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    pc = p.nodal ? p.nodal[p.local[(int64_t)f * n_dof + lane]] : p.value;
    const int64_t node = p.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.u[node * DIM + i] + p.x_ref[node * DIM + i];
  }
  const bool any = __ballot(pc != 0.0) != 0;
  if (lane == 0) p.active[f] = any ? 1 : 0;
  if (!any) return;
  for (int q0 = 0; q0 < n_q; q0 += 64) {
    const bool on = q0 + lane < n_q;
    const int64_t pt = (int64_t)f * n_q + (on ? q0 + lane : 0);
    const double* N = p.N + pt * n_dof;
    const double* dN = p.dN + pt * n_dof * (DIM - 1);
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
    if (!p.nodal) pq = p.value;
    if (on) {
      p.coef[pt] = p.sign * (p.weight[pt] * pq);
#pragma unroll
      for (int k = 0; k < (DIM - 1) * DIM; ++k) p.tang[pt * ((DIM - 1) * DIM) + k] = t[k];
    }
  }
}

struct BoundaryActionArgs {
  int n_faces, n_dof, n_q;
  const int32_t* dofs;
  const double* N;
  const double* dN;
  const double* coef;
  const double* tang;
  const unsigned char* active;
  double factor;
  const double* x;
  double* face_y;            // [n_faces][dim][n_dof]
};

template<int DIM>
__global__ __launch_bounds__(256) void boundary_action_kernel(BoundaryActionArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n_faces) return;
  if (!p.active[f]) return;   // (wave-uniform; the node sum skips the face)
  const int n_dof = p.n_dof, n_q = p.n_q, NT = n_dof * DIM;
  double xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    const int64_t node = p.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.x[node * DIM + i];
  }
  const int k = lane < NT ? lane : 0, ki = k / n_dof, ka = k % n_dof;
  double Y = 0.0;
  for (int q0 = 0; q0 < n_q; q0 += 64) {
    // stage 1, lane = point q0 + lane: g = c_q dm
    double g[DIM];
    {
      const bool on = q0 + lane < n_q;
      const int64_t pt = (int64_t)f * n_q + (on ? q0 + lane : 0);
      const double* dN = p.dN + pt * n_dof * (DIM - 1);
      double dt[(DIM - 1) * DIM];
#pragma unroll
      for (int kk = 0; kk < (DIM - 1) * DIM; ++kk) dt[kk] = 0.0;
      for (int c = 0; c < n_dof; ++c) {
#pragma unroll
        for (int i = 0; i < DIM; ++i) {
          const double x = face_lane_read(xc[i], c);
#pragma unroll
          for (int kk = 0; kk < DIM - 1; ++kk) dt[kk * DIM + i] = __builtin_fma(x, dN[kk * n_dof + c], dt[kk * DIM + i]);
        }
      }
      const double cq = on ? p.coef[pt] : 0.0;
      double dm[DIM];
      if constexpr (DIM == 2) {
        dm[0] = dt[1];
        dm[1] = -dt[0];
      } else {
        double t[6];
#pragma unroll
        for (int kk = 0; kk < 6; ++kk) t[kk] = p.tang[pt * 6 + kk];
        const double *t1 = t, *t2 = t + 3, *d1 = dt, *d2 = dt + 3;
        dm[0] = (d1[1] * t2[2] - d1[2] * t2[1]) + (t1[1] * d2[2] - t1[2] * d2[1]);
        dm[1] = (d1[2] * t2[0] - d1[0] * t2[2]) + (t1[2] * d2[0] - t1[0] * d2[2]);
        dm[2] = (d1[0] * t2[1] - d1[1] * t2[0]) + (t1[0] * d2[1] - t1[1] * d2[0]);
      }
#pragma unroll
      for (int i = 0; i < DIM; ++i) g[i] = cq * dm[i];
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

// The record of one handle and its launchers; contact.hip and pressure.hip hold one each beside their FaceAssembly.
struct BoundaryAction {
  DeviceBuffer<double> coef, tang, face_y;
  DeviceBuffer<unsigned char> active;
  bool linearized = false;
  hipEvent_t lin_event = nullptr;      // recorded behind the last linearize
  hipStream_t lin_stream = nullptr;    // the stream it ran on
  BoundaryAction() = default;
  BoundaryAction(const BoundaryAction&) = delete;
  BoundaryAction& operator=(const BoundaryAction&) = delete;
  ~BoundaryAction() {
    if (lin_event) (void)hipEventDestroy(lin_event);
  }

  int64_t bytes(const FaceSet& h) const {
    if (!linearized) return 0;
    const int64_t npts = (int64_t)h.n_faces * h.n_q;
    return npts * (1 + (h.dim - 1) * h.dim) * (int64_t)sizeof(double) + h.n_faces;
  }

  // the snapshot at u_dev, on the handle's stream.  nodal: values at the face nodes (nullptr: `value` everywhere)
  void linearize(FaceSet& h, const double* u_dev, const double* nodal, double value, double sign) {
    const size_t npts = (size_t)h.n_faces * h.n_q;
    coef.resize(npts);
    tang.resize(npts * (h.dim - 1) * h.dim);
    active.resize((size_t)h.n_faces);
    const BoundaryLinearizeArgs a{h.n_faces, h.n_dof, h.n_q, h.dofs.ptr, h.local.ptr, h.N.ptr, h.dN.ptr, h.weight.ptr, h.x_ref.ptr,
                                  u_dev,     nodal,   value, sign,       coef.ptr,    tang.ptr, active.ptr};
    const dim3 grid((unsigned)((h.n_faces + 3) / 4));
    if (h.dim == 2) launch(boundary_linearize_kernel<2>, grid, dim3(256), 0, h.stream, a);
    else launch(boundary_linearize_kernel<3>, grid, dim3(256), 0, h.stream, a);
    if (!lin_event) MH_HIP(hipEventCreateWithFlags(&lin_event, hipEventDisableTiming));
    MH_HIP(hipEventRecord(lin_event, h.stream));
    lin_stream = h.stream;
    linearized = true;
  }

  void require(const char* who) const {
    if (!linearized) fail("mimi_hip_%s_apply_tangent before any mimi_hip_%s_linearize", who, who);
  }

  // what the action builds on first use, and the wait of `s` on the last linearize
  void begin(FaceSet& h, hipStream_t s) {
    face_y.resize((size_t)h.n_faces * h.n_dof * h.dim);
    if (s != lin_stream) MH_HIP(hipStreamWaitEvent(s, lin_event, 0));
  }

  // y += factor K_face x over the recorded active faces; x, y on the device, everything on s
  void add(FaceAssembly& h, double factor, const double* x, double* y, hipStream_t s) {
    const BoundaryActionArgs a{h.n_faces, h.n_dof, h.n_q, h.dofs.ptr, h.N.ptr, h.dN.ptr, coef.ptr, tang.ptr, active.ptr, factor, x, face_y.ptr};
    const dim3 grid((unsigned)((h.n_faces + 3) / 4));
    if (h.dim == 2) launch(boundary_action_kernel<2>, grid, dim3(256), 0, s, a);
    else launch(boundary_action_kernel<3>, grid, dim3(256), 0, s, a);
    if (h.dim == 2) h.template gather_vector<2>(active.ptr, face_y.ptr, y, s);
    else h.template gather_vector<3>(active.ptr, face_y.ptr, y, s);
    MH_HIP(hipGetLastError());
  }
};

// the C entries mimi_hip_<who>_apply_tangent: host or device x / y through the handle's staging buffers
template<typename H>
void boundary_apply_entry(H* h, const char* who, double factor, const double* x, double* y) {
  if (!h) fail("null handle");
  if (!x || !y) fail("null vector argument");
  h->action.require(who);
  MH_HIP(hipSetDevice(h->device));
  Mirror<double> mx = Mirror<double>::in(x, h->n_vdofs, h->stage_u, h->stream);
  Mirror<double> my = Mirror<double>::inout(y, h->n_vdofs, h->stage_r, h->stream);
  h->action.begin(*h, h->stream);
  h->action.add(*h, factor, mx.dev, my.dev, h->stream);
  my.finish(h->stream);
  if (mx.host || my.host) MH_HIP(hipStreamSynchronize(h->stream));
}

// mimi_hip_<who>_action_info
template<typename H>
int64_t boundary_action_info(const H* h, int what) {
  if (!h) return -1;
  if (what == 0) return h->action.bytes(*h);
  if (what == 1) return h->face_k.ptr ? 1 : 0;
  return -1;
}

}  // namespace
}  // namespace mimi_hip
