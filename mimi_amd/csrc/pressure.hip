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
// vector and tangent block densely, then one wave per CSR row of a face node walks the node's (face, local node)
// incidences in a fixed order into an LDS image of the row.  No atomics on the assembly path: the same bits every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "common.hpp"
#include "face_common.hpp"

namespace mimi_hip {

struct PressureArgs {
  int dim, n_faces, n_dof, n_q;
  const int32_t* dofs;       // [n_faces][n_dof] global node ids
  const int32_t* local;      // [n_faces][n_dof] index into the face nodes (nodal pressure)
  const double* N;           // [n_faces][n_q][n_dof]
  const double* dN;          // [n_faces][n_q][dim-1][n_dof]
  const double* weight;      // [n_faces][n_q]
  const double* x_ref;       // [n_nodes][dim]
  const int64_t* rowptr;
  const int32_t* pair_pos;   // [n_faces][n_dof][n_dof]: position of column node b in the row of node a, from the row start
  const double* nodal;       // [n_face_nodes] or nullptr: uniform
  double value;              // uniform pressure
  const double* u;
  double* r;
  double* A;
  double grad_factor;
  double* face_r;            // [n_faces][dim][n_dof]
  double* face_k;            // [n_faces][(a, i)][(j, b)]
  double* face_scal;         // [n_faces][1 + dim]  current area, external force
  unsigned char* face_active;   // some pressure on the face is not zero
};

// One WAVE per face.  Lane c < n_dof holds node c (position, nodal pressure); lane q < n_q forms the point's pressure,
// tangents and normal from them by lane reads; lane k = i n_dof + a sums the residual entry over the points; lane 0 sums the
// face's area and force; with WITH_K, lane = node pair (a, b) accumulates its DIM x DIM tangent block over the points.
template<int DIM, int WITH_K>
__global__ __launch_bounds__(256) void pressure_face_kernel(PressureArgs p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.n_faces) return;
  const int n_dof = p.n_dof, n_q = p.n_q, NT = n_dof * DIM;
  double pc = 0.0, xc[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) xc[i] = 0.0;
  if (lane < n_dof) {
    pc = p.nodal ? p.nodal[p.local[(int64_t)f * n_dof + lane]] : p.value;
    const int64_t node = p.dofs[(int64_t)f * n_dof + lane];
#pragma unroll
    for (int i = 0; i < DIM; ++i) xc[i] = p.u[node * DIM + i] + p.x_ref[node * DIM + i];
  }
  const bool active = __ballot(pc != 0.0) != 0;
  // stage 1, lane q: wq = w p(q), the tangents and the normal m
  double wq = 0.0, dA = 0.0, tq[(DIM - 1) * DIM], mq[DIM];
#pragma unroll
  for (int k = 0; k < (DIM - 1) * DIM; ++k) tq[k] = 0.0;
  {
    const int q = lane < n_q ? lane : 0;
    const int64_t pt = (int64_t)f * n_q + q;
    const double* N = p.N + pt * n_dof;
    const double* dN = p.dN + pt * n_dof * (DIM - 1);
    double pq = 0.0;
    for (int c = 0; c < n_dof; ++c) {
      pq = __builtin_fma(N[c], pressure_lane_read(pc, c), pq);
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double x = pressure_lane_read(xc[i], c);
#pragma unroll
        for (int k = 0; k < DIM - 1; ++k) tq[k * DIM + i] = __builtin_fma(x, dN[k * n_dof + c], tq[k * DIM + i]);
      }
    }
    if (!p.nodal) pq = p.value;
    pressure_normal<DIM>(tq, mq);
    double mm = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) mm += mq[i] * mq[i];
    wq = p.weight[pt] * pq;
    dA = p.weight[pt] * sqrt(mm);
  }
  // area and external force of the face, lane 0, in the order of the points
  {
    double area = 0.0, force[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) force[i] = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const double wpq = pressure_lane_read(wq, q);
#pragma unroll
      for (int i = 0; i < DIM; ++i) force[i] -= wpq * pressure_lane_read(mq[i], q);
      area += pressure_lane_read(dA, q);
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
      const double wpq = pressure_lane_read(wq, q);
      double aw = pressure_lane_read(mq[0], q) * wpq;
#pragma unroll
      for (int ii = 1; ii < DIM; ++ii) {
        const double v = pressure_lane_read(mq[ii], q) * wpq;
        aw = i == ii ? v : aw;
      }
      R = __builtin_fma(aw, p.N[((int64_t)f * n_q + q) * n_dof + a], R);
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
        const double wpn = pressure_lane_read(wq, q) * p.N[pt * n_dof + a];
        const double* dN = p.dN + pt * n_dof * (DIM - 1);
        if constexpr (DIM == 2) {
          // dm_0 / dx_b1 = N_b,xi, dm_1 / dx_b0 = -N_b,xi
          const double d = wpn * dN[b];
          acc[0 * 2 + 1] += d;
          acc[1 * 2 + 0] -= d;
        } else {
          double t[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) t[k] = pressure_lane_read(tq[k], q);
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

// One wave per CSR row (face node l, component i): the node's (face, local node) incidences in face order, row (a, i) of
// every active face block added into an LDS image of the row through the pair positions (lane = column node b: distinct
// positions within an instruction), then the image added to the caller's values in one coalesced pass; the residual
// entry likewise.  Rows none of whose faces is active are left untouched.  The image is sized to the longest face row
// (row_cap doubles per wave, dynamic LDS): the walk is latency-bound, and at degree 2 (375 entries) a CU holds twice
// the waves it holds with contact's fixed 1056-entry image.
constexpr int PG_WAVES = 4;
constexpr int PG_MAX_ROW = 1056;   // (2 p + 1)^3 neighbours x 3 at p = 3 is 1029
template<int DIM, int WITH_K>
__global__ __launch_bounds__(64 * PG_WAVES) void pressure_gather_kernel(PressureArgs p, int n_fnodes, const int32_t* __restrict__ fnodes,
                                                                        const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj,
                                                                        int row_cap) {
  extern __shared__ double img_all[];   // [PG_WAVES][row_cap] with WITH_K, else empty
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t R = (int64_t)blockIdx.x * PG_WAVES + wave;
  if (R >= (int64_t)n_fnodes * DIM) return;
  const int l = (int)(R / DIM), i = (int)(R % DIM);
  const int a_beg = adj_ptr[l], a_end = adj_ptr[l + 1];
  bool any = false;
  for (int t = a_beg; t < a_end; ++t) any = any || p.face_active[adj[t] >> 6];
  if (!any) return;
  const int64_t row = (int64_t)fnodes[l] * DIM + i;
  const int NT = p.n_dof * DIM;
  if constexpr (WITH_K) {
    double* img = img_all + wave * row_cap;
    const int64_t beg = p.rowptr[row];
    const int len = (int)(p.rowptr[row + 1] - beg);
    for (int k = lane; k < len; k += 64) img[k] = 0.0;
    __builtin_amdgcn_wave_barrier();
    for (int t = a_beg; t < a_end; ++t) {
      const int64_t f = adj[t] >> 6;
      const int a = adj[t] & 63;
      if (!p.face_active[f]) continue;
      const double* Kr = p.face_k + (f * NT + (a * DIM + i)) * (int64_t)NT;   // row (a, i): [j][b]
      for (int b = lane; b < p.n_dof; b += 64) {
        const int32_t off = p.pair_pos[(f * p.n_dof + a) * p.n_dof + b];
#pragma unroll
        for (int j = 0; j < DIM; ++j) img[off + j] += Kr[j * p.n_dof + b];
      }
      __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
    for (int k = lane; k < len; k += 64) p.A[beg + k] += p.grad_factor * img[k];
  }
  if (lane == 0) {
    double rs = 0.0;
    for (int t = a_beg; t < a_end; ++t) {
      const int64_t f = adj[t] >> 6;
      if (p.face_active[f]) rs += p.face_r[f * NT + i * p.n_dof + (adj[t] & 63)];
    }
    p.r[row] += rs;
  }
}

// out[k] = sum_f in[f * stride + k] (k < n_out): ONE workgroup, every thread a fixed subset of the faces, then a
// fixed-shape tree -- the same bits every run
__global__ __launch_bounds__(1024) void pressure_sum_kernel(int64_t n, int stride, int n_out, const double* __restrict__ in,
                                                            double* __restrict__ out) {
  __shared__ double part[1024];
  for (int k = 0; k < n_out; ++k) {
    double s = 0.0;
    for (int64_t f = threadIdx.x; f < n; f += 1024) s += in[f * stride + k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
      if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = part[0];
    __syncthreads();
  }
}

// create time: position of (row node a, column node b) of every face relative to the start of a's CSR row (component 0);
// a pair missing from the pattern sets *status (every such thread stores the same value)
__global__ void pressure_pair_pos_kernel(int n_faces, int n_dof, int dim, const int32_t* dofs, const int64_t* rowptr,
                                         const int32_t* col, int32_t* pair_pos, int* status) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n_faces * n_dof * n_dof) return;
  const int b = idx % n_dof, a = (idx / n_dof) % n_dof;
  const int64_t f = idx / ((int64_t)n_dof * n_dof);
  const int64_t row = (int64_t)dofs[f * n_dof + a] * dim;
  const int32_t target = dofs[f * n_dof + b] * dim;
  int64_t lo = rowptr[row], hi = rowptr[row + 1];
  const int64_t base = lo;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < target) lo = mid + 1; else hi = mid;
  }
  if (lo >= rowptr[row + 1] || col[lo] != target) {
    *status = 4;
    pair_pos[idx] = 0;
    return;
  }
  pair_pos[idx] = (int32_t)(lo - base);
}

}  // namespace mimi_hip

using namespace mimi_hip;

struct mimi_hip_pressure_s {
  int device = 0, dim = 0, n_faces = 0, n_dof = 0, n_q = 0, n_fnodes = 0, row_cap = 0;
  int64_t n_nodes = 0, n_vdofs = 0, nnz = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  double value = 0.0;
  bool use_nodal = false;
  DeviceBuffer<int32_t> dofs, local, pair_pos, adj_ptr, adj, fnodes_dev;
  DeviceBuffer<double> N, dN, weight, x_ref, nodal, scalars, face_r, face_k, face_scal;
  DeviceBuffer<unsigned char> face_active;
  DeviceBuffer<int64_t> rowptr_own;
  const int64_t* rowptr = nullptr;
  DeviceBuffer<double> stage_u, stage_r, stage_A;
  DeviceBuffer<int> status;
  std::vector<int32_t> face_nodes;   // sorted global node ids of the faces (index of a nodal pressure value -> node)
  ~mimi_hip_pressure_s() {
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

template<typename F>
static int guarded_p(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return 1;
  }
}

static PressureArgs pressure_args(mimi_hip_pressure_s* h, const double* u, double* r, double* A, double gf) {
  PressureArgs a{};
  a.dim = h->dim;
  a.n_faces = h->n_faces;
  a.n_dof = h->n_dof;
  a.n_q = h->n_q;
  a.dofs = h->dofs.ptr;
  a.local = h->local.ptr;
  a.N = h->N.ptr;
  a.dN = h->dN.ptr;
  a.weight = h->weight.ptr;
  a.x_ref = h->x_ref.ptr;
  a.rowptr = h->rowptr;
  a.pair_pos = h->pair_pos.ptr;
  a.nodal = h->use_nodal ? h->nodal.ptr : nullptr;
  a.value = h->value;
  a.u = u;
  a.r = r;
  a.A = A;
  a.grad_factor = gf;
  a.face_r = h->face_r.ptr;
  a.face_k = h->face_k.ptr;
  a.face_scal = h->face_scal.ptr;
  a.face_active = h->face_active.ptr;
  return a;
}

template<int DIM>
static void launch_pressure(mimi_hip_pressure_s* h, const PressureArgs& a, bool with_grad) {
  const unsigned bf = (unsigned)((h->n_faces + 3) / 4);
  if (with_grad) hipLaunchKernelGGL((pressure_face_kernel<DIM, 1>), dim3(bf), dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL((pressure_face_kernel<DIM, 0>), dim3(bf), dim3(256), 0, h->stream, a);
  // area and force of the faces (last_area_ / last_force_), in a fixed order
  hipLaunchKernelGGL(pressure_sum_kernel, dim3(1), dim3(1024), 0, h->stream, (int64_t)h->n_faces, 1 + DIM, 1 + DIM,
                     h->face_scal.ptr, h->scalars.ptr);
  const unsigned bg = (unsigned)(((int64_t)h->n_fnodes * DIM + PG_WAVES - 1) / PG_WAVES);
  if (with_grad)
    hipLaunchKernelGGL((pressure_gather_kernel<DIM, 1>), dim3(bg), dim3(64 * PG_WAVES), PG_WAVES * h->row_cap * sizeof(double),
                       h->stream, a, h->n_fnodes, h->fnodes_dev.ptr, h->adj_ptr.ptr, h->adj.ptr, h->row_cap);
  else
    hipLaunchKernelGGL((pressure_gather_kernel<DIM, 0>), dim3(bg), dim3(64 * PG_WAVES), 0, h->stream, a, h->n_fnodes,
                       h->fnodes_dev.ptr, h->adj_ptr.ptr, h->adj.ptr, 0);
}

static void run_pressure(mimi_hip_pressure_s* h, const double* u, double* r, double* A, double gf, bool with_grad) {
  MH_HIP(hipSetDevice(h->device));
  if (!u || !r || (with_grad && !A)) fail("null vector argument");
  Mirror<double> mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
  Mirror<double> mr = Mirror<double>::inout(r, h->n_vdofs, h->stage_r, h->stream);
  Mirror<double> mA;
  if (with_grad) mA = Mirror<double>::inout(A, h->nnz, h->stage_A, h->stream);
  if (with_grad && !h->face_k.ptr) {
    const size_t nt = (size_t)h->n_dof * h->dim;
    h->face_k.resize((size_t)h->n_faces * nt * nt);
  }
  const PressureArgs a = pressure_args(h, mu.dev, mr.dev, mA.dev, gf);
  if (h->dim == 2) launch_pressure<2>(h, a, with_grad);
  else launch_pressure<3>(h, a, with_grad);
  MH_HIP(hipGetLastError());
  mr.finish(h->stream);
  if (with_grad) mA.finish(h->stream);
  if (mu.host || mr.host || mA.host) MH_HIP(hipStreamSynchronize(h->stream));
}

extern "C" {

int mimi_hip_pressure_create(const mimi_hip_pressure_tables* t, int device, mimi_hip_pressure_t* out) {
  return guarded_p([&] {
    if (!t || !out) fail("null argument");
    if (t->dim != 2 && t->dim != 3) fail("Unsupported Dim: %d", t->dim);
    if (t->n_dof < 1 || t->n_dof > kPressureMaxDof) fail("face n_dof %d out of range [1,%d]", t->n_dof, kPressureMaxDof);
    if (t->n_faces < 1) fail("no loaded boundary faces");
    if (t->n_quad < 1 || t->n_quad > kPressureMaxQuad) fail("face quadrature points %d out of range [1,%d]", t->n_quad, kPressureMaxQuad);
    if (!t->dofs || !t->N || !t->dN_dxi || !t->weight || !t->x_ref) fail("null table");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
      fail("libmimi_hip: no HIP device visible -- this library has no CPU fallback");
    auto h = std::make_unique<mimi_hip_pressure_s>();
    h->device = device;
    MH_HIP(hipSetDevice(device));
    MH_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    h->dim = t->dim;
    h->n_faces = t->n_faces;
    h->n_dof = t->n_dof;
    h->n_q = t->n_quad;
    h->n_nodes = t->n_nodes;
    h->n_vdofs = t->n_nodes * t->dim;
    const size_t nfd = (size_t)t->n_faces * t->n_dof;
    std::vector<int32_t> dofs(nfd);
    if (is_device_pointer(t->dofs))
      MH_HIP(hipMemcpy(dofs.data(), t->dofs, nfd * sizeof(int32_t), hipMemcpyDeviceToHost));
    else
      std::copy(t->dofs, t->dofs + nfd, dofs.begin());
    for (int32_t d : dofs)
      if (d < 0 || d >= t->n_nodes) fail("face node id %d out of range [0,%lld)", d, (long long)t->n_nodes);
    if (t->n_faces >= (1 << 25)) fail("too many boundary faces for the incidence encoding");
    // the face nodes, sorted and unique (the order of the nodal pressure values and of the row gather), and their
    // (face, local node) incidences, faces ascending: the summation order of the gather
    const FaceIncidences inc = face_incidences(dofs, t->n_dof);
    const std::vector<int32_t>& fnodes = inc.fnodes;
    h->n_fnodes = (int)fnodes.size();
    h->face_nodes = fnodes;
    h->dofs.assign(dofs.data(), nfd, h->stream);
    h->local.assign(inc.local.data(), nfd, h->stream);
    const size_t npts = (size_t)t->n_faces * t->n_quad;
    h->N.assign(t->N, npts * t->n_dof, h->stream);
    h->dN.assign(t->dN_dxi, npts * t->n_dof * (t->dim - 1), h->stream);
    h->weight.assign(t->weight, npts, h->stream);
    h->x_ref.assign(t->x_ref, (size_t)t->n_nodes * t->dim, h->stream);
    h->nodal.resize(h->n_fnodes);
    h->scalars.resize(4);
    MH_HIP(hipMemsetAsync(h->scalars.ptr, 0, 4 * sizeof(double), h->stream));
    h->adj_ptr.assign(inc.adj_ptr.data(), inc.adj_ptr.size(), h->stream);
    h->adj.assign(inc.adj.data(), inc.adj.size(), h->stream);
    h->fnodes_dev.assign(fnodes.data(), fnodes.size(), h->stream);
    h->face_r.resize(nfd * t->dim);
    h->face_scal.resize((size_t)t->n_faces * (1 + t->dim));
    h->face_active.resize((size_t)t->n_faces);
    MH_HIP(hipMemsetAsync(h->face_active.ptr, 0, (size_t)t->n_faces, h->stream));
    h->status.resize(1);
    MH_HIP(hipMemsetAsync(h->status.ptr, 0, sizeof(int), h->stream));
    if (!t->csr_rowptr || !t->csr_col) fail("csr_rowptr / csr_col must be given");
    if (is_device_pointer(t->csr_rowptr)) {
      h->rowptr = t->csr_rowptr;
    } else {
      h->rowptr_own.assign(t->csr_rowptr, h->n_vdofs + 1, h->stream);
      h->rowptr = h->rowptr_own.ptr;
    }
    MH_HIP(hipMemcpy(&h->nnz, h->rowptr + h->n_vdofs, sizeof(int64_t), hipMemcpyDeviceToHost));
    {
      // the gather keeps the CSR row of a face dof in LDS (PG_MAX_ROW doubles): a longer row is refused here
      std::vector<int64_t> rp_host;
      const int64_t* rp = t->csr_rowptr;
      if (is_device_pointer(t->csr_rowptr)) {
        rp_host.resize((size_t)h->n_vdofs + 1);
        MH_HIP(hipMemcpy(rp_host.data(), t->csr_rowptr, rp_host.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        rp = rp_host.data();
      }
      int64_t longest = 0;
      for (int32_t node : fnodes)
        for (int i = 0; i < t->dim; ++i) {
          const int64_t row = (int64_t)node * t->dim + i;
          longest = std::max(longest, rp[row + 1] - rp[row]);
        }
      if (longest > PG_MAX_ROW)
        fail("a CSR row of a loaded face dof holds %lld entries; the pressure gather supports at most %d", (long long)longest, PG_MAX_ROW);
      h->row_cap = (int)((longest + 7) / 8 * 8);   // PG_WAVES x row_cap doubles of LDS per workgroup: <= 33 KB
    }
    DeviceBuffer<int32_t> col_tmp;
    const int32_t* col_dev = t->csr_col;
    if (!is_device_pointer(t->csr_col)) {
      col_tmp.assign(t->csr_col, h->nnz, h->stream);
      col_dev = col_tmp.ptr;
    }
    const int64_t total = (int64_t)nfd * t->n_dof;
    h->pair_pos.resize(total);
    hipLaunchKernelGGL(pressure_pair_pos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, t->n_faces,
                       t->n_dof, t->dim, h->dofs.ptr, h->rowptr, col_dev, h->pair_pos.ptr, h->status.ptr);
    MH_HIP(hipGetLastError());
    int st = 0;
    MH_HIP(hipMemcpyAsync(&st, h->status.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    if (st) fail("CSR pattern does not contain a boundary element's dof block");
    *out = h.release();
  });
}

int mimi_hip_pressure_destroy(mimi_hip_pressure_t h) {
  return guarded_p([&] {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
  });
}

int mimi_hip_pressure_set_stream(mimi_hip_pressure_t h, void* stream) {
  return guarded_p([&] {
    if (!h) fail("null handle");
    h->stream = stream == MIMI_HIP_STREAM_NULL ? nullptr : (stream ? reinterpret_cast<hipStream_t>(stream) : h->own_stream);
  });
}

int mimi_hip_pressure_synchronize(mimi_hip_pressure_t h) {
  return guarded_p([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_pressure_set_value(mimi_hip_pressure_t h, double p) {
  return guarded_p([&] {
    if (!h) fail("null handle");
    if (!std::isfinite(p)) fail("pressure must be finite");
    h->value = p;
    h->use_nodal = false;
  });
}

int mimi_hip_pressure_face_nodes(mimi_hip_pressure_t h, int32_t* out, int64_t capacity, int64_t* n) {
  return guarded_p([&] {
    if (!h || !n) fail("null argument");
    *n = h->n_fnodes;
    if (!out) return;
    if (capacity < h->n_fnodes) fail("node buffer too small");
    std::copy(h->face_nodes.begin(), h->face_nodes.end(), out);
  });
}

int mimi_hip_pressure_set_nodal(mimi_hip_pressure_t h, const double* p, int64_t n) {
  return guarded_p([&] {
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
  return guarded_p([&] {
    if (!h) fail("null handle");
    run_pressure(h, u, r, nullptr, 0.0, false);
  });
}

int mimi_hip_pressure_add_residual_and_grad(mimi_hip_pressure_t h, const double* u, double grad_factor, double* r,
                                            double* A_values) {
  return guarded_p([&] {
    if (!h) fail("null handle");
    run_pressure(h, u, r, A_values, grad_factor, true);
  });
}

int mimi_hip_pressure_last_history(mimi_hip_pressure_t h, double* out4) {
  return guarded_p([&] {
    if (!h || !out4) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    double s[4] = {0, 0, 0, 0};
    MH_HIP(hipMemcpyAsync(s, h->scalars.ptr, (1 + h->dim) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 4; ++k) out4[k] = s[k];
  });
}

}  // extern "C"
