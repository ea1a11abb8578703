// The matrix-free action of the two face tangents -- contact.hip (frozen nodal pressure, mortar_contact.cpp:263-295) and
// pressure.hip (follower pressure) -- without the per-face (n_dof dim)^2 blocks.  Both residuals are c_q N_a m_i with m the
// non-normalised normal of face_common.hpp (c_q = -w p_q for contact, contact.hip "analytic frozen-pressure tangent";
// c_q = w p_q for the follower load, pressure.hip), so both tangents are c_q N_a dm_i/dx_bj and
//   (K_face x)(a, i) = sum_q c_q N_a dm_i,   dm = dt_1 x t_2 + t_1 x dt_2 (3-D), (dt_y, -dt_x) (2-D),   dt_k = sum_b N_b,k x_b.
// Stands in for MortarContact::AddBoundaryResidualAndGrad (mortar_contact.cpp:353-421) followed by SparseMatrix::Mult.
//   linearize  one wave per face: per point c_q and the surface tangents t at u, per face the active flag -- the record
//              (n_faces n_q (1 + (dim - 1) dim) doubles + n_faces bytes); nothing of u is kept
//   action     one wave per face, four per workgroup.  Lane c holds node c's x, handed round by face_lane_read.  Stage 1,
//              lane = point: dt, dm, g = c_q dm.  Stage 2, lane = (i, a): y_f(a, i) += g_i(q) N_q[a] over the points in
//              ascending order, so the bytes do not depend on the launch.  face_y [n_faces][dim][n_dof] is a buffer of the
//              record's owner, not the assembly's face_r.
// The stages -- wave index, node load, point stage, normal rate, point scatter -- are face_wave.hpp's, shared with every
// other face kernel: the action forms the tangents' rate with the text that formed the recorded tangents.
//   node sum   face_row_gather_kernel<DIM, 0> over the RECORDED flags, in the order of the incidences.  No atomics.
// Registers only: the kernels are latency-bound like the face gather (face_common.hpp) and spend no LDS.
#pragma once

#include "face_common.hpp"

namespace mimi_hip {
namespace {

struct BoundaryLinearizeArgs {
  FaceView v;
  const double* u;
  const double* nodal;       // values at the face nodes, or nullptr: `value` everywhere
  double value;
  double sign;               // -1 contact, +1 follower pressure
  double* coef;              // [n_faces][n_q]               c_q = sign w p_q
  double* tang;              // [n_faces][n_q][dim-1][dim]   t at u
  unsigned char* active;     // [n_faces]                    some nodal value of the face is not zero (IsPressureZero)
};

template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void boundary_linearize_kernel(BoundaryLinearizeArgs p) {
  int lane, f;
  if (!face_wave_index(p.v, lane, f)) return;
  double xc[DIM];
  const double pc = face_load_nodes<DIM, true, kNodalOrValue>(p.v, f, lane, p.u, xc, p.nodal, p.value);
  const bool any = __ballot(pc != 0.0) != 0;
  if (lane == 0) p.active[f] = any ? 1 : 0;
  if (!any) return;
  const int64_t pt = face_lane_point(p.v, f, lane);
  double pq, t[(DIM - 1) * DIM];
  face_point_stage<DIM, true, false, true>(p.v, pt, pc, xc, &pq, nullptr, t);
  if (!p.nodal) pq = p.value;
  if (lane < p.v.n_q) {
    p.coef[pt] = p.sign * (p.v.weight[pt] * pq);
#pragma unroll
    for (int k = 0; k < (DIM - 1) * DIM; ++k) p.tang[pt * ((DIM - 1) * DIM) + k] = t[k];
  }
}

struct BoundaryActionArgs {
  FaceView v;
  const double* coef;
  const double* tang;
  const unsigned char* active;
  double factor;
  const double* x;
  double* face_y;            // [n_faces][dim][n_dof]
};

// the recorded tangents of the lane's point
template<int DIM>
MH_WAVE void face_recorded_tangents(const double* tang, int64_t pt, double* t) {
#pragma unroll
  for (int k = 0; k < (DIM - 1) * DIM; ++k) t[k] = tang[pt * ((DIM - 1) * DIM) + k];
}

template<int DIM>
__global__ __launch_bounds__(kFaceWaveThreads) void boundary_action_kernel(BoundaryActionArgs p) {
  int lane, f;
  if (!face_wave_index(p.v, lane, f)) return;
  if (!p.active[f]) return;   // (wave-uniform; the node sum skips the face)
  double xc[DIM];
  face_load_nodes<DIM, false>(p.v, f, lane, p.x, xc);
  const FaceEntry e = face_lane_entry<DIM>(p.v, lane);
  // stage 1, lane = point: g = c_q dm
  const int64_t pt = face_lane_point(p.v, f, lane);
  double g[DIM], t[(DIM - 1) * DIM], dt[(DIM - 1) * DIM], m[DIM], dm[DIM];
  face_recorded_tangents<DIM>(p.tang, pt, t);
  face_point_stage<DIM, false, false, true>(p.v, pt, 0.0, xc, nullptr, nullptr, dt);
  face_normal_rate<DIM>(t, dt, m, dm);
  const double cq = lane < p.v.n_q ? p.coef[pt] : 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) g[i] = cq * dm[i];
  // stage 2, lane = (i, a)
  const double Y = face_scatter_points<DIM, true>(p.v, f, e, g);
  const int NT = p.v.n_dof * DIM;
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
    const BoundaryLinearizeArgs a{h.view(), u_dev, nodal, value, sign, coef.ptr, tang.ptr, active.ptr};
    face_dispatch_dim(h.dim, [&](auto D) {
      launch(boundary_linearize_kernel<decltype(D)::value>, face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0, h.stream, a);
    });
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
    const BoundaryActionArgs a{h.view(), coef.ptr, tang.ptr, active.ptr, factor, x, face_y.ptr};
    face_dispatch_dim(h.dim, [&](auto D) {
      launch(boundary_action_kernel<decltype(D)::value>, face_wave_grid(h.n_faces), dim3(kFaceWaveThreads), 0, s, a);
    });
    h.gather_vector(active.ptr, face_y.ptr, y, s);
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
  if (what == MIMI_HIP_ACTION_INFO_BYTES) return h->action.bytes(*h);
  if (what == MIMI_HIP_ACTION_INFO_FACE_BLOCKS) return h->face_k.ptr ? 1 : 0;
  return -1;
}

}  // namespace
}  // namespace mimi_hip
