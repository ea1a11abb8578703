// C ABI + kernels of the coupling surface: integrators::CouplingSurface.
//
// A partitioned fluid-structure coupling iterates the reference's fixed_point_solve2 / fixed_point_advance2 with its fluid
// partner before advance_time2 commits the step (py/py_solid.cpp:443-511, solvers/ode.cpp:81-186).  Every coupling
// iteration the partner needs the wet surface and hands back a traction; both run here, on the faces, quadrature rule and
// outward normal of the follower pressure (pressure.hip, splines.face_tables), for the configuration x = X + u:
//   points    x_q = sum_a N_a x_a,   n_q = m_q / |m_q|,   da_q = w_q |m_q|       (m_q = a_1 x a_2 or (a_y, -a_x))
//   load      f(a,i) += sum_q w_q |m_q| N_a(xi_q) t(q,i)                          (t: a traction per unit area of x)
// Points are face-major, point-minor.  Face pass: one WAVE per face, laid out as pressure_face_kernel -- lane c < n_dof holds
// node c, lane q < n_q forms its point from lane reads; the points mode writes the face's [n_q][dim] outputs as consecutive
// addresses of consecutive lanes, the load mode reads t the same way and sums lane k = (a, i) over the points in a fixed
// order into a dense face vector [n_faces][n_dof][dim] (the stages of face_wave.hpp, here in the kernel's own text).
// Node gather: one lane per (face node, component) walks the node's
// (face, local node) incidences in ascending face order.  No atomics: the same bits every run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <vector>

#include "common.hpp"
#include "face_common.hpp"

namespace mimi_hip {

struct SurfaceArgs {
  FaceView v;
  const double* u;         // [n_nodes][dim], nullptr: the reference configuration
  const double* t;         // [n_points][dim] (load mode)
  double* x_out;           // [n_points][dim] or nullptr (points mode)
  double* n_out;           // [n_points][dim] or nullptr
  double* w_out;           // [n_points] or nullptr
  double* face_f;          // [n_faces][n_dof][dim] (load mode)
};

MH_DEV double surface_shuffle(double v, int src) {   // the value lane src holds (src per lane; every lane active)
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// out[base + e] = component e % DIM of the point of lane e / DIM, for e < count = n_q DIM: lane e writes entry e
template<int DIM>
MH_DEV void surface_write_points(double* out, int64_t base, int count, const double* v, int lane) {
  for (int e0 = 0; e0 < count; e0 += 64) {
    const int e = e0 + lane;
    const int src = e < count ? e / DIM : 0, comp = e - (e / DIM) * DIM;
    double val = surface_shuffle(v[0], src);
#pragma unroll
    for (int i = 1; i < DIM; ++i) {
      const double w = surface_shuffle(v[i], src);
      val = comp == i ? w : val;
    }
    if (e < count) out[base + e] = val;
  }
}

// (The kernel keeps its own stage text, for the reason pressure_face_kernel does: on face_wave.hpp's helpers the same arithmetic
// came with 4 to 14 instructions more, and u may be null inside the node load.)
template<int DIM, int LOAD>
__global__ __launch_bounds__(kFaceWaveThreads) void surface_face_kernel(SurfaceArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.v.n_faces) return;   // the whole wave
  const int n_dof = p.v.n_dof, n_q = p.v.n_q;
  double xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    const int64_t node = p.v.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.u ? p.u[node * DIM + i] + p.v.x_ref[node * DIM + i] : p.v.x_ref[node * DIM + i];
  }
  // lane q: the position, the tangents (in pressure_face_kernel's order), the normal m and the area weight w |m|
  const int q = lane < n_q ? lane : 0;
  const int64_t pt = (int64_t)f * n_q + q;
  double xq[DIM], tq[(DIM - 1) * DIM], mq[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xq[i] = 0.0;
#pragma unroll
  for (int k = 0; k < (DIM - 1) * DIM; ++k) tq[k] = 0.0;
  {
    const double* N = p.v.N + pt * n_dof;
    const double* dN = p.v.dN + pt * n_dof * (DIM - 1);
    for (int c = 0; c < n_dof; ++c) {
      const double Nc = N[c];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double x = face_lane_read(xc[i], c);
        xq[i] = __builtin_fma(Nc, x, xq[i]);
#pragma unroll
        for (int k = 0; k < DIM - 1; ++k) tq[k * DIM + i] = __builtin_fma(x, dN[k * n_dof + c], tq[k * DIM + i]);
      }
    }
  }
  face_normal<DIM>(tq, mq);
  double mm = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) mm += mq[i] * mq[i];
  const double len = sqrt(mm), dA = p.v.weight[pt] * len;
  const int count = n_q * DIM;
  const int64_t base = (int64_t)f * count;
  if constexpr (!LOAD) {
    if (p.x_out) surface_write_points<DIM>(p.x_out, base, count, xq, lane);
    if (p.n_out) {
      double nq[DIM];
#pragma unroll
      for (int i = 0; i < DIM; ++i) nq[i] = mq[i] / len;
      surface_write_points<DIM>(p.n_out, base, count, nq, lane);
    }
    if (p.w_out && lane < n_q) p.w_out[pt] = dA;
  } else {
    // the face's t (count <= 75 doubles) read as consecutive addresses of consecutive lanes, then moved to lane q
    const double t0 = lane < count ? p.t[base + lane] : 0.0;
    const double t1 = lane + 64 < count ? p.t[base + 64 + lane] : 0.0;
    double wt[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const int s = q * DIM + i;
      const double a = surface_shuffle(t0, s & 63), b = surface_shuffle(t1, s & 63);
      wt[i] = dA * (s < 64 ? a : b);
    }
    // lane k = a DIM + i: f(a, i) = sum_q (w |m| t_i)_q N_q[a], the points in order
    const int NT = n_dof * DIM;
    const int k = lane < NT ? lane : 0, a = k / DIM, i = k - a * DIM;
    double F = 0.0;
    for (int qq = 0; qq < n_q; ++qq) {
      double v = face_lane_read(wt[0], qq);
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double w = face_lane_read(wt[ii], qq);
        v = i == ii ? w : v;
      }
      F = __builtin_fma(v, p.v.N[((int64_t)f * n_q + qq) * n_dof + a], F);
    }
    if (lane < NT) p.face_f[(int64_t)f * NT + lane] = F;
  }
}

// one lane per (face node l, component i): f[node, i] += the node's face entries, faces ascending
__global__ __launch_bounds__(256) void surface_gather_kernel(int dim, int n_dof, int64_t n_rows, const int32_t* __restrict__ fnodes,
                                                             const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj,
                                                             const double* __restrict__ face_f, double* __restrict__ f) {
  const int64_t R = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (R >= n_rows) return;
  const int l = (int)(R / dim), i = (int)(R - (int64_t)l * dim);
  const int NT = n_dof * dim;
  double s = 0.0;
  for (int t = adj_ptr[l]; t < adj_ptr[l + 1]; ++t) {
    const int64_t fc = adj[t] >> 6;
    s += face_f[fc * NT + (adj[t] & 63) * dim + i];
  }
  f[(int64_t)fnodes[l] * dim + i] += s;
}

}  // namespace mimi_hip

using namespace mimi_hip;

struct mimi_hip_surface_s : FaceSet {
  int64_t n_points = 0;
  DeviceBuffer<double> face_f;
  DeviceBuffer<double> stage_t, stage_f, stage_x, stage_n, stage_w;
};

static void launch_surface_face(const mimi_hip_surface_s* h, const SurfaceArgs& a, bool load) {
  face_dispatch_dim(h->dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    launch(load ? surface_face_kernel<DIM, 1> : surface_face_kernel<DIM, 0>, face_wave_grid(h->n_faces), dim3(kFaceWaveThreads), 0,
           h->stream, a);
  });
}

extern "C" {

int mimi_hip_surface_create(const mimi_hip_pressure_tables* t, int device, mimi_hip_surface_t* out) {
  return guarded([&] {
    if (!t || !out) fail("null argument");
    auto h = std::make_unique<mimi_hip_surface_s>();
    h->create(face_tables_of(*t), device, kFaceMaxQuad, "coupling");
    h->n_points = (int64_t)t->n_faces * t->n_quad;
    h->face_f.resize((size_t)t->n_faces * t->n_dof * t->dim);
    MH_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
  });
}

int mimi_hip_surface_destroy(mimi_hip_surface_t h) { return handle_destroy(h); }
int mimi_hip_surface_set_stream(mimi_hip_surface_t h, void* stream) { return handle_set_stream(h, stream); }
int mimi_hip_surface_synchronize(mimi_hip_surface_t h) { return handle_synchronize(h); }

int64_t mimi_hip_surface_n_points(mimi_hip_surface_t h) { return h ? h->n_points : -1; }

int mimi_hip_surface_points(mimi_hip_surface_t h, const double* u, double* x, double* normal, double* weight) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    const size_t nv = (size_t)h->n_points * h->dim;
    Mirror<double> mu, mx, mn, mw;
    if (u) mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
    if (x) mx = Mirror<double>::inout(x, nv, h->stage_x, h->stream);
    if (normal) mn = Mirror<double>::inout(normal, nv, h->stage_n, h->stream);
    if (weight) mw = Mirror<double>::inout(weight, h->n_points, h->stage_w, h->stream);
    launch_surface_face(h, SurfaceArgs{h->view(), mu.dev, nullptr, mx.dev, mn.dev, mw.dev, nullptr}, false);
    mx.finish(h->stream);
    mn.finish(h->stream);
    mw.finish(h->stream);
    if (mu.host || mx.host || mn.host || mw.host) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_surface_add_load(mimi_hip_surface_t h, const double* u, const double* t, double* f) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!t || !f) fail("null vector argument");
    MH_HIP(hipSetDevice(h->device));
    Mirror<double> mu;
    if (u) mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
    Mirror<double> mt = Mirror<double>::in(t, (size_t)h->n_points * h->dim, h->stage_t, h->stream);
    Mirror<double> mf = Mirror<double>::inout(f, h->n_vdofs, h->stage_f, h->stream);
    launch_surface_face(h, SurfaceArgs{h->view(), mu.dev, mt.dev, nullptr, nullptr, nullptr, h->face_f.ptr}, true);
    const int64_t rows = (int64_t)h->n_fnodes * h->dim;
    launch(surface_gather_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, h->dim, h->n_dof, rows,
           h->fnodes_dev.ptr, h->adj_ptr.ptr, h->adj.ptr, h->face_f.ptr, mf.dev);
    mf.finish(h->stream);
    if (mu.host || mt.host || mf.host) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"
