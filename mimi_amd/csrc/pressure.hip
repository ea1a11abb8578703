// C ABI + kernels of the follower-pressure boundary integrator: integrators::FollowerPressure.
//
// The reference's BCMarker stores pressure(bid, value) (utils/boundary_conditions.cpp:43-50) but never applies it
// (py/py_nonlinear_solid.cpp:221-283 wires up body force and traction only).  Here it is the follower load of a
// finite-strain solver, t = -p n da on the CURRENT surface, x = X + u:
//   a_k = sum_b x_b dN_b/dxi_k,  m = a_1 x a_2 (3-D) or (a_y, -a_x) (2-D)   (the non-normalised outward normal)
//   residual  r(a,i)      += sum_q w_q p_q N_a m_i                         (internal minus external force)
//   tangent   A(ai, bj)   += grad_factor sum_q w_q p_q N_a dm_i/dx_bj
//             dm/dx_b = N_b,1 (-[a_2]x) + N_b,2 ([a_1]x)  (3-D),   N_b,xi [[0, 1], [-1, 0]]  (2-D)
// p_q = p (uniform) or sum_a N_a p_a (values at the face's control points); neither depends on u, so the tangent is exact
// (and not symmetric).
//
// The pipeline is contact pass 2 (contact.hip) with a prescribed pressure: one wave per face stores the face residual
// vector and tangent block densely (pressure_face_kernel), then the row gather both share (face_common.hpp: one wave per
// CSR row of a face node walks the node's (face, local node) incidences in a fixed order into an LDS image of the row).
// No atomics on the assembly path: the same bits every run.  pressure_face_kernel has the stages of face_wave.hpp (wave index,
// node load, point stage, point scatter, node-pair loop) in its own text, see there; the face tables reach it as a FaceView and
// the matrix-free action shares the layer.
// The matrix-free action of the tangent (mimi_hip_follower_linearize / _apply_tangent, and the Krylov solvers' boundary
// terms through apply_seam.hpp) is kernels_face_action.hpp, shared with contact.hip: c_q = w p_q, no face tangent block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "apply_seam.hpp"
#include "common.hpp"
#include "face_common.hpp"
#include "kernels_face_action.hpp"

namespace mimi_hip {

struct PressureArgs {
  FaceView v;
  const double* nodal;       // [n_face_nodes] or nullptr: uniform
  double value;              // uniform pressure
  const double* u;
  double* face_r;            // [n_faces][dim][n_dof]
  double* face_k;            // [n_faces][(a, i)][(j, b)]
  double* face_scal;         // [n_faces][1 + dim]  current area, external force
  unsigned char* face_active;   // some pressure on the face is not zero
};

// One WAVE per face.  Lane c < n_dof holds node c (position, nodal pressure); lane q < n_q forms the point's pressure,
// tangents and normal from them by lane reads; lane k = i n_dof + a sums the residual entry over the points; lane 0 sums the
// face's area and force; with WITH_K, lane = node pair (a, b) accumulates its DIM x DIM tangent block over the points.
// (The kernel keeps its own stage text: written on face_wave.hpp's helpers it computed the same bytes with the same arithmetic
// instructions, but 4 to 23 instructions more of index arithmetic and branches, and no helper variant gave the old stream back.  Its
// tangent block is the expanded [a]x form with wpn folded into d1 and d2: another association, another rounding, than
// face_normal_column's.)
template<int DIM, int WITH_K>
__global__ __launch_bounds__(kFaceWaveThreads) void pressure_face_kernel(PressureArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.v.n_faces) return;
  const int n_dof = p.v.n_dof, n_q = p.v.n_q, NT = n_dof * DIM;
  double pc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    pc = p.nodal ? p.nodal[p.v.local[(int64_t)f * n_dof + lane]] : p.value;
    const int64_t node = p.v.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.u[node * DIM + i] + p.v.x_ref[node * DIM + i];
  }
  const bool active = __ballot(pc != 0.0) != 0;
  // stage 1, lane q: wq = w p(q), the tangents and the normal m
  double wq = 0.0, dA = 0.0, tq[(DIM - 1) * DIM], mq[DIM];
#pragma unroll
  for (int k = 0; k < (DIM - 1) * DIM; ++k) tq[k] = 0.0;
  {
    const int q = lane < n_q ? lane : 0;
    const int64_t pt = (int64_t)f * n_q + q;
    const double* N = p.v.N + pt * n_dof;
    const double* dN = p.v.dN + pt * n_dof * (DIM - 1);
    double pq = 0.0;
    for (int c = 0; c < n_dof; ++c) {
      pq = __builtin_fma(N[c], face_lane_read(pc, c), pq);
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double x = face_lane_read(xc[i], c);
#pragma unroll
        for (int k = 0; k < DIM - 1; ++k) tq[k * DIM + i] = __builtin_fma(x, dN[k * n_dof + c], tq[k * DIM + i]);
      }
    }
    if (!p.nodal) pq = p.value;
    face_normal<DIM>(tq, mq);
    double mm = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) mm += mq[i] * mq[i];
    wq = p.v.weight[pt] * pq;
    dA = p.v.weight[pt] * sqrt(mm);
  }
  // area and external force of the face, lane 0, in the order of the points
  {
    double area = 0.0, force[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) force[i] = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const double wpq = face_lane_read(wq, q);
#pragma unroll
      for (int i = 0; i < DIM; ++i) force[i] -= wpq * face_lane_read(mq[i], q);
      area += face_lane_read(dA, q);
    }
    if (lane == 0) {
      p.face_active[f] = active ? 1 : 0;
      p.face_scal[(int64_t)f * (1 + DIM)] = area;
#pragma unroll
      for (int i = 0; i < DIM; ++i) p.face_scal[(int64_t)f * (1 + DIM) + 1 + i] = force[i];
    }
  }
  if (!active) return;
  // lane k = i n_dof + a: r(a, i) = sum_q (w p m_i)_q N_q[a]
  {
    const int k = lane < NT ? lane : 0, i = k / n_dof, a = k % n_dof;
    double R = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const double wpq = face_lane_read(wq, q);
      double aw = face_lane_read(mq[0], q) * wpq;
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double v = face_lane_read(mq[ii], q) * wpq;
        aw = i == ii ? v : aw;
      }
      R = __builtin_fma(aw, p.v.N[((int64_t)f * n_q + q) * n_dof + a], R);
    }
    if (lane < NT) p.face_r[(int64_t)f * NT + lane] = R;      // [i][a]
  }
  if constexpr (WITH_K) {
    const int n_pairs = n_dof * n_dof;
    double* Kf = p.face_k + (int64_t)f * NT * NT;
    for (int pair0 = 0; pair0 < n_pairs; pair0 += 64) {
      const int pair = pair0 + lane;
      const bool on = pair < n_pairs;
      const int a = on ? pair / n_dof : 0, b = on ? pair % n_dof : 0;
      double acc[DIM * DIM];
#pragma unroll
      for (int k = 0; k < DIM * DIM; ++k) acc[k] = 0.0;
      for (int q = 0; q < n_q; ++q) {
        const int64_t pt = (int64_t)f * n_q + q;
        const double wpn = face_lane_read(wq, q) * p.v.N[pt * n_dof + a];
        const double* dN = p.v.dN + pt * n_dof * (DIM - 1);
        if constexpr (DIM == 2) {
          // dm_0 / dx_b1 = N_b,xi, dm_1 / dx_b0 = -N_b,xi
          const double d = wpn * dN[b];
          acc[0 * 2 + 1] += d;
          acc[1 * 2 + 0] -= d;
        } else {
          double t[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) t[k] = face_lane_read(tq[k], q);
          const double d1 = wpn * dN[b], d2 = wpn * dN[n_dof + b];
          // dm / dx_bj = d1 (e_j x a_2) + d2 (a_1 x e_j): column j of d1 [a_2]x^T + d2 [a_1]x
          const double* a1 = t;
          const double* a2 = t + 3;
          acc[0 * 3 + 1] += d1 * a2[2] - d2 * a1[2];
          acc[0 * 3 + 2] += -d1 * a2[1] + d2 * a1[1];
          acc[1 * 3 + 0] += -d1 * a2[2] + d2 * a1[2];
          acc[1 * 3 + 2] += d1 * a2[0] - d2 * a1[0];
          acc[2 * 3 + 0] += d1 * a2[1] - d2 * a1[1];
          acc[2 * 3 + 1] += -d1 * a2[0] + d2 * a1[0];
        }
      }
      if (on) {
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
          for (int j = 0; j < DIM; ++j) Kf[(a * DIM + i) * NT + j * n_dof + b] = acc[i * DIM + j];
      }
    }
  }
}

}  // namespace mimi_hip

using namespace mimi_hip;

struct mimi_hip_pressure_s : FaceAssembly {
  double value = 0.0;
  bool use_nodal = false;
  DeviceBuffer<double> nodal, scalars;   // nodal: pressure values at fnodes (the order of set_nodal)
  BoundaryAction action;                 // mimi_hip_follower_linearize / _apply_tangent (kernels_face_action.hpp)
};

// ---- the operator seam of the Krylov solvers (apply_seam.hpp) ----------------------------------------------------------------
namespace mimi_hip {
int64_t operator_size(const mimi_hip_pressure_s* h) { return h->n_vdofs; }
int operator_device(const mimi_hip_pressure_s* h) { return h->device; }
void operator_begin_solve(mimi_hip_pressure_s* h, hipStream_t solver_stream) {
  h->action.require("follower");
  MH_HIP(hipSetDevice(h->device));
  h->action.begin(*h, solver_stream);
}
void operator_add_action(mimi_hip_pressure_s* h, double factor, const double* x, double* y, hipStream_t solver_stream) {
  h->action.add(*h, factor, x, y, solver_stream);
}
}  // namespace mimi_hip

static void run_pressure(mimi_hip_pressure_s* h, const double* u, double* r, double* A, double gf, bool with_grad) {
  if (!r) fail("null vector argument");
  h->run(u, r, A, with_grad, [&](const double* u_dev, double* r_dev, double* A_dev) {
    if (with_grad) h->reserve_face_k();
    const PressureArgs a{h->view(), h->use_nodal ? h->nodal.ptr : nullptr, h->value, u_dev, h->face_r.ptr, h->face_k.ptr,
                         h->face_scal.ptr, h->face_active.ptr};
    face_dispatch_dim(h->dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      launch(with_grad ? pressure_face_kernel<DIM, 1> : pressure_face_kernel<DIM, 0>, face_wave_grid(h->n_faces), dim3(kFaceWaveThreads),
             0, h->stream, a);
    });
    // area and force of the faces (last_area_ / last_force_), in a fixed order
    launch(face_sum_kernel, dim3(1), dim3(1024), 0, h->stream, (int64_t)h->n_faces, 1 + h->dim, 1 + h->dim, h->face_scal.ptr,
           (const unsigned char*)nullptr, h->scalars.ptr);
    h->gather(r_dev, A_dev, gf, with_grad);
  });
}

extern "C" {

int mimi_hip_pressure_create(const mimi_hip_pressure_tables* t, int device, mimi_hip_pressure_t* out) {
  return guarded([&] {
    if (!t || !out) fail("null argument");
    const FaceTables ft = face_tables_of(*t);
    auto h = std::make_unique<mimi_hip_pressure_s>();
    h->create(ft, device, kFaceMaxQuad, "loaded boundary");
    h->nodal.resize(h->n_fnodes);
    h->scalars.resize(4);
    MH_HIP(hipMemsetAsync(h->scalars.ptr, 0, 4 * sizeof(double), h->stream));
    h->attach_csr(ft, "loaded face", "pressure");
    *out = h.release();
  });
}

int mimi_hip_pressure_destroy(mimi_hip_pressure_t h) { return handle_destroy(h); }
int mimi_hip_pressure_set_stream(mimi_hip_pressure_t h, void* stream) { return handle_set_stream(h, stream); }
int mimi_hip_pressure_synchronize(mimi_hip_pressure_t h) { return handle_synchronize(h); }

int mimi_hip_pressure_set_value(mimi_hip_pressure_t h, double p) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!std::isfinite(p)) fail("pressure must be finite");
    h->value = p;
    h->use_nodal = false;
  });
}

int mimi_hip_pressure_face_nodes(mimi_hip_pressure_t h, int32_t* out, int64_t capacity, int64_t* n) {
  return guarded([&] {
    if (!h) fail("null argument");
    h->copy_fnodes(out, capacity, n);
  });
}

int mimi_hip_pressure_set_nodal(mimi_hip_pressure_t h, const double* p, int64_t n) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!p) {
      h->use_nodal = false;
      return;
    }
    if (n != h->n_fnodes) fail("nodal pressure has %lld values, the faces have %d nodes", (long long)n, h->n_fnodes);
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(h->nodal.ptr, p, (size_t)n * sizeof(double), hipMemcpyDefault, h->stream));
    if (!is_device_pointer(p)) MH_HIP(hipStreamSynchronize(h->stream));
    h->use_nodal = true;
  });
}

int mimi_hip_pressure_add_residual(mimi_hip_pressure_t h, const double* u, double* r) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_pressure(h, u, r, nullptr, 0.0, false);
  });
}

int mimi_hip_pressure_add_residual_and_grad(mimi_hip_pressure_t h, const double* u, double grad_factor, double* r,
                                            double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_pressure(h, u, r, A_values, grad_factor, true);
  });
}

int mimi_hip_follower_linearize(mimi_hip_pressure_t h, const double* u) {
  return guarded([&] {
    if (!h) fail("null handle");
    h->run(u, nullptr, nullptr, false, [&](const double* u_dev, double*, double*) {
      h->action.linearize(*h, u_dev, h->use_nodal ? h->nodal.ptr : nullptr, h->value, 1.0);
    });
  });
}

int mimi_hip_follower_apply_tangent(mimi_hip_pressure_t h, double factor, const double* x, double* y) {
  return guarded([&] { boundary_apply_entry(h, "follower", factor, x, y); });
}

int64_t mimi_hip_follower_action_info(mimi_hip_pressure_t h, int what) { return boundary_action_info(h, what); }

int mimi_hip_pressure_last_history(mimi_hip_pressure_t h, double* out4) {
  return guarded([&] {
    if (!h || !out4) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    double s[4] = {0, 0, 0, 0};
    MH_HIP(hipMemcpyAsync(s, h->scalars.ptr, (1 + h->dim) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 4; ++k) out4[k] = s[k];
  });
}

}  // extern "C"
