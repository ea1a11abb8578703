// What the boundary-face integrators share -- contact.hip (integrators::MortarContact), pressure.hip (integrators::
// FollowerPressure) and surface.hip (integrators::CouplingSurface):
//   device   the size limits of a face, the one-workgroup fixed-order sum, the pair positions of the face blocks in the CSR
//            rows, and the row gather of the dense face residual vectors and tangent blocks through an LDS image of the row
//            (the wave-per-face stages of the face kernels themselves are face_wave.hpp's);
//   host     FaceSet (a handle's face tables on the device and the face-node incidence lists that give every node gather
//            its fixed summation order; surface.hip stops here) and FaceAssembly (a FaceSet attached to a CSR pattern,
//            with the dense face stores, their gather and the u / r / A mirroring of an assembly call).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "face_wave.hpp"

namespace mimi_hip {

constexpr int kFaceMaxDof = 16;    // nodes of a face: (p + 1)^2 at degree 3
constexpr int kFaceMaxQuad = 25;   // points of a face: (p + 2)^2 at degree 3 (rule 2 p + 3); contact allows a wave's 64
constexpr int kFaceGatherWaves = 4;
constexpr int kFaceMaxRow = 1056;  // (2 p + 1)^3 neighbours x 3 at p = 3 is 1029

static_assert(kFaceMaxQuad <= 64, "face_wave.hpp: a lane holds one point of the face");

// calls f(integral_constant DIM): the one dimension switch of the face files
template<class F>
void face_dispatch_dim(int dim, F&& f) {
  if (dim == 2) f(std::integral_constant<int, 2>{}); else f(std::integral_constant<int, 3>{});
}

// Kernels and the host code that launches them: each translation unit that includes this header has its own copy (its
// own code object), hence the unnamed namespace.
namespace {

// out[k] = sum_i in[i * stride + k] (k < n_out), optionally over the rows with flag[i] != 0: ONE workgroup, every thread a
// fixed subset of the rows, then a fixed-shape tree -- the same bits every run
__global__ __launch_bounds__(1024) void face_sum_kernel(int64_t n, int stride, int n_out, const double* __restrict__ in,
                                                        const unsigned char* __restrict__ flag, double* __restrict__ out) {
  __shared__ double part[1024];
  for (int k = 0; k < n_out; ++k) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
      if (!flag || flag[i]) s += in[i * stride + k];
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
// a pair missing from the pattern sets *status (a plain store: every such thread stores the same value)
__global__ void face_pair_pos_kernel(int n_faces, int n_dof, int dim, const int32_t* dofs, const int64_t* rowptr,
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

struct FaceGatherArgs {
  int n_dof;
  const int64_t* rowptr;
  const int32_t* pair_pos;           // [n_faces][n_dof][n_dof]: position of column node b in the row of node a, from the row start
  const unsigned char* face_active;  // [n_faces]
  const double* face_r;              // [n_faces][dim][n_dof]
  const double* face_k;              // [n_faces][(a, i)][(j, b)]
  double* r;
  double* A;
  double grad_factor;
};

// The sums the reference forms under a mutex (mortar_contact.cpp:338-341,400-408), without atomics: one wave per CSR row
// (face node l, component i); the wave walks the node's (face, local node) incidences in face order, adds row (a, i) of
// every ACTIVE face block into an LDS image of the CSR row through the pair positions (lane = column node b: distinct
// positions within an instruction), then adds the image to the caller's values in one coalesced pass; the residual entry
// likewise.  Rows none of whose faces is active are left untouched.  The image is sized to the longest face row (row_cap
// doubles per wave, dynamic LDS): the walk is latency-bound, and at degree 2 (375 entries) a CU holds twice the waves it
// holds with a 1056-entry image.
template<int DIM, int WITH_K>
__global__ __launch_bounds__(64 * kFaceGatherWaves) void face_row_gather_kernel(FaceGatherArgs p, int n_fnodes, const int32_t* __restrict__ fnodes,
                                                                                const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj,
                                                                                int row_cap) {
  extern __shared__ double img_all[];   // [kFaceGatherWaves][row_cap] with WITH_K, else empty
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t R = (int64_t)blockIdx.x * kFaceGatherWaves + wave;
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

// the fields mimi_hip_contact_tables and mimi_hip_pressure_tables have in common
struct FaceTables {
  int dim, n_faces, n_dof, n_quad;
  int64_t n_nodes;
  const int32_t* dofs;
  const double *N, *dN_dxi, *weight, *x_ref;
  const int64_t* csr_rowptr;
  const int32_t* csr_col;
};

template<typename T>
FaceTables face_tables_of(const T& t) {
  return {t.dim, t.n_faces, t.n_dof, t.n_quad, t.n_nodes, t.dofs, t.N, t.dN_dxi, t.weight, t.x_ref, t.csr_rowptr, t.csr_col};
}

// The faces of one handle on its device: the five tables, the sizes, the sorted face nodes (the marked nodes of the
// reference's contact, mortar_contact.cpp:41-76: sorted unique dofs -> 0 .. n_fnodes - 1) and their incidences.
struct FaceSet : StreamHandle {
  int dim = 0, n_faces = 0, n_dof = 0, n_q = 0, n_fnodes = 0;
  int64_t n_nodes = 0, n_vdofs = 0;
  DeviceBuffer<int32_t> dofs, local, adj_ptr, adj, fnodes_dev;
  DeviceBuffer<double> N, dN, weight, x_ref, stage_u;
  std::vector<int32_t> fnodes;

  // checks t, opens the handle on `device` and uploads; `what` names the faces in the messages ("marked boundary", ...)
  void create(const FaceTables& t, int device, int max_quad, const char* what) {
    if (t.dim != 2 && t.dim != 3) fail("Unsupported Dim: %d", t.dim);
    if (t.n_dof < 1 || t.n_dof > kFaceMaxDof) fail("face n_dof %d out of range [1,%d]", t.n_dof, kFaceMaxDof);
    if (t.n_faces < 1) fail("no %s faces", what);
    if (t.n_faces >= (1 << 25)) fail("too many %s faces for the incidence encoding", what);
    if (t.n_quad < 1 || t.n_quad > max_quad) fail("face quadrature points %d out of range [1,%d]", t.n_quad, max_quad);   // (max_quad <= 64: face_wave.hpp rests on a lane per point)
    if (!t.dofs || !t.N || !t.dN_dxi || !t.weight || !t.x_ref) fail("null table");
    open(device);
    dim = t.dim;
    n_faces = t.n_faces;
    n_dof = t.n_dof;
    n_q = t.n_quad;
    n_nodes = t.n_nodes;
    n_vdofs = t.n_nodes * t.dim;
    const size_t nfd = (size_t)t.n_faces * t.n_dof, npts = (size_t)t.n_faces * t.n_quad;
    const std::vector<int32_t> dofs_h = to_host(t.dofs, nfd);
    for (int32_t d : dofs_h)
      if (d < 0 || d >= t.n_nodes) fail("face node id %d out of range [0,%lld)", d, (long long)t.n_nodes);
    FaceIncidences inc = face_incidences(dofs_h, t.n_dof);
    n_fnodes = (int)inc.fnodes.size();
    dofs.assign(dofs_h.data(), nfd, stream);
    local.assign(inc.local.data(), nfd, stream);
    N.assign(t.N, npts * t.n_dof, stream);
    dN.assign(t.dN_dxi, npts * t.n_dof * (t.dim - 1), stream);
    weight.assign(t.weight, npts, stream);
    x_ref.assign(t.x_ref, (size_t)t.n_nodes * t.dim, stream);
    adj_ptr.assign(inc.adj_ptr.data(), inc.adj_ptr.size(), stream);
    adj.assign(inc.adj.data(), inc.adj.size(), stream);
    fnodes_dev.assign(inc.fnodes.data(), inc.fnodes.size(), stream);
    fnodes = std::move(inc.fnodes);
  }

  FaceView view() const { return {n_faces, n_dof, n_q, dofs.ptr, local.ptr, N.ptr, dN.ptr, weight.ptr, x_ref.ptr}; }

  // the C entries that list the face nodes (out == NULL: count only)
  void copy_fnodes(int32_t* out, int64_t capacity, int64_t* n) const {
    if (!n) fail("null argument");
    *n = n_fnodes;
    if (!out) return;
    if (capacity < n_fnodes) fail("node buffer too small");
    std::copy(fnodes.begin(), fnodes.end(), out);
  }
};

// A FaceSet that assembles into a CSR pattern: the dense per-face stores of the atomic-free assembly and their row gather.
struct FaceAssembly : FaceSet {
  int row_cap = 0;                   // doubles of the row image per wave: the longest row of a face dof, rounded up to 8
  int64_t nnz = 0;
  DeviceBuffer<int64_t> rowptr_own;
  const int64_t* rowptr = nullptr;   // device; the caller's when it is there already
  DeviceBuffer<int32_t> pair_pos;
  DeviceBuffer<double> face_r, face_k, face_scal, stage_r, stage_A;   // face_k: sized by the first tangent assembly
  DeviceBuffer<unsigned char> face_active;

  // after create(): `rows` ("marked contact", "loaded face") and `who` ("contact", "pressure") word the refusal of a row
  // that does not fit the image
  void attach_csr(const FaceTables& t, const char* rows, const char* who) {
    if (!t.csr_rowptr || !t.csr_col) fail("csr_rowptr / csr_col must be given");
    const std::vector<int64_t> rp = to_host(t.csr_rowptr, (size_t)n_vdofs + 1);
    if (is_device_pointer(t.csr_rowptr)) {
      rowptr = t.csr_rowptr;
    } else {
      rowptr_own.assign(rp.data(), rp.size(), stream);
      rowptr = rowptr_own.ptr;
    }
    nnz = rp[n_vdofs];
    // the gather keeps the CSR row of a face dof in LDS: a caller's pattern with a longer row (multi-patch, degree >= 4)
    // is refused here instead of overflowing the image at assembly time
    int64_t longest = 0;
    for (int32_t node : fnodes)
      for (int i = 0; i < dim; ++i) {
        const int64_t row = (int64_t)node * dim + i;
        longest = std::max(longest, rp[row + 1] - rp[row]);
      }
    if (longest > kFaceMaxRow)
      fail("a CSR row of a %s dof holds %lld entries; the %s gather supports at most %d", rows, (long long)longest, who, kFaceMaxRow);
    row_cap = (int)((longest + 7) / 8 * 8);   // kFaceGatherWaves x row_cap doubles of LDS per workgroup: <= 33 KB
    DeviceBuffer<int32_t> col_tmp;
    const int32_t* col_dev = t.csr_col;
    if (!is_device_pointer(t.csr_col)) {
      col_tmp.assign(t.csr_col, nnz, stream);
      col_dev = col_tmp.ptr;
    }
    DeviceBuffer<int> status;
    status.resize(1);
    MH_HIP(hipMemsetAsync(status.ptr, 0, sizeof(int), stream));
    const int64_t total = (int64_t)n_faces * n_dof * n_dof;
    pair_pos.resize(total);
    launch(face_pair_pos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n_faces, n_dof, dim, dofs.ptr, rowptr,
           col_dev, pair_pos.ptr, status.ptr);
    int st = 0;
    MH_HIP(hipMemcpyAsync(&st, status.ptr, sizeof(int), hipMemcpyDeviceToHost, stream));
    MH_HIP(hipStreamSynchronize(stream));
    if (st) fail("CSR pattern does not contain a boundary element's dof block");
    face_r.resize((size_t)n_faces * n_dof * dim);
    face_scal.resize((size_t)n_faces * (1 + dim));
    face_active.resize((size_t)n_faces);
    MH_HIP(hipMemsetAsync(face_active.ptr, 0, (size_t)n_faces, stream));
  }

  void reserve_face_k() {
    const size_t nt = (size_t)n_dof * dim;
    if (!face_k.ptr) face_k.resize((size_t)n_faces * nt * nt);
  }

  // r (and, with_grad, A) += the rows of the face nodes, from face_r / face_k of the active faces.  (The two gathers are
  // templates so that a source that gathers nothing -- surface.hip -- holds no gather kernel.)
  template<int = 0>
  void gather(double* r, double* A, double grad_factor, bool with_grad) {
    const FaceGatherArgs a{n_dof, rowptr, pair_pos.ptr, face_active.ptr, face_r.ptr, face_k.ptr, r, A, grad_factor};
    face_dispatch_dim(dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      const dim3 grid((unsigned)(((int64_t)n_fnodes * DIM + kFaceGatherWaves - 1) / kFaceGatherWaves)), block(64 * kFaceGatherWaves);
      if (with_grad)
        launch(face_row_gather_kernel<DIM, 1>, grid, block, kFaceGatherWaves * row_cap * sizeof(double), stream, a, n_fnodes,
               fnodes_dev.ptr, adj_ptr.ptr, adj.ptr, row_cap);
      else
        launch(face_row_gather_kernel<DIM, 0>, grid, block, 0, stream, a, n_fnodes, fnodes_dev.ptr, adj_ptr.ptr, adj.ptr, 0);
    });
  }

  // y += the node sums of a dense face vector [n_faces][dim][n_dof] over the faces flagged in `active`, on stream s: the
  // gather above without K, for callers that keep flags and vectors of their own (kernels_face_action.hpp)
  template<int = 0>
  void gather_vector(const unsigned char* active, const double* face_vec, double* y, hipStream_t s) {
    const FaceGatherArgs a{n_dof, rowptr, pair_pos.ptr, active, face_vec, nullptr, y, nullptr, 0.0};
    face_dispatch_dim(dim, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      const dim3 grid((unsigned)(((int64_t)n_fnodes * DIM + kFaceGatherWaves - 1) / kFaceGatherWaves));
      launch(face_row_gather_kernel<DIM, 0>, grid, dim3(64 * kFaceGatherWaves), 0, s, a, n_fnodes, fnodes_dev.ptr, adj_ptr.ptr,
             adj.ptr, 0);
    });
  }

  // One assembly call: u mirrored in, r (when given) and, with_grad, A mirrored in and out around
  // launch(u_dev, r_dev, A_dev); synchronous when any of them lives on the host.
  template<typename Launch>
  void run(const double* u, double* r, double* A, bool with_grad, Launch&& launch) {
    MH_HIP(hipSetDevice(device));
    if (!u || (with_grad && !A)) fail("null vector argument");
    Mirror<double> mu = Mirror<double>::in(u, n_vdofs, stage_u, stream), mr, mA;
    if (r) mr = Mirror<double>::inout(r, n_vdofs, stage_r, stream);
    if (with_grad) mA = Mirror<double>::inout(A, nnz, stage_A, stream);
    launch(mu.dev, mr.dev, mA.dev);
    MH_HIP(hipGetLastError());
    mr.finish(stream);
    mA.finish(stream);
    if (mu.host || mr.host || mA.host) MH_HIP(hipStreamSynchronize(stream));
  }
};

}  // namespace
}  // namespace mimi_hip
