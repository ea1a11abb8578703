// C ABI + kernels of the periodic fold: the reference's BCMarker::PeriodicBoundary (utils/boundary_conditions.cpp:152-159),
// applied there through NURBSExtension::ConnectBoundaries (py/py_nonlinear_solid.cpp:34-62).
//
// The integrators keep assembling into the patch's ordinary, unwrapped structured CSR (so a degree-2/3 patch stays on the
// two-phase tensor kernels).  P is the 0/1 map from the folded (periodic) dofs to the unwrapped ones, given per node by
// node_map[n_nodes_u] -> folded node (component-wise in the byVDIM numbering: vdof n dim + c -> node_map[n] dim + c):
//   expand   u_u = P u_f
//   fold     r_f += P^T r_u,   A_f = A_base + P^T A_u P
// Set-up: the copies of every folded node (ascending unwrapped index, on the host: one pass over the nodes), the folded
// pattern (each folded row is the sorted union of its source rows' columns mapped through node_map, two passes: count,
// then fill) and each unwrapped entry's place in its folded row.  The fold: one wave per folded row, the row image in LDS,
// the sources in ascending order, each source's entries added through the per-entry place map.  Within one source the
// places are distinct -- except where a source row's window wraps onto itself (a periodic direction with fewer nodes than
// the window), which set-up flags; such a row is added by one lane.  No atomics: the same bits every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "apply_seam.hpp"
#include "common.hpp"

namespace mimi_hip {

constexpr uint32_t kFoldDup = 0x80000000u;    // set-up: "an earlier entry of the gathered row has this column"
constexpr int FOLD_WAVES = 4;
constexpr int FOLD_MAX_ROW = 4096;           // doubles of a folded row image (a degree-3 3-D row holds at most 1029)
constexpr int FOLD_MAX_GATHER = 16384;       // columns of all source rows of one folded row (8 x 1029 at degree 3)

struct FoldSetup {
  int dim;
  int64_t n_f, n_u;
  const int32_t* node_map;   // [n_nodes_u]
  const int32_t* copy_ptr;   // [n_nodes_f + 1]
  const int32_t* copies;     // [n_nodes_u], ascending within a folded node
  const int64_t* rowptr_u;
  const int32_t* col_u;
  const int64_t* rowptr_f;   // fill pass only
  int64_t* count_f;          // count pass: entries of every folded row
  int32_t* col_f;            // fill pass
  int32_t* entry_pos;        // fill pass: [nnz_u] place in the folded row
  unsigned char* serial;     // [n_f] a source adds twice to one place
  int* status;               // a column index outside [0, n_u)
};

// One wave per folded row R = (F, c): the mapped columns of every source row (F's copies in ascending order) in LDS, then
// every entry is marked when an earlier one has the same column (O(L^2) over the L gathered columns: set-up only, L is
// a few hundred).  Count pass: the row's distinct columns; fill pass: place of an entry = number of distinct columns below
// its own, the first entry of each column writes the folded col.
template<int FILL>
__global__ __launch_bounds__(64) void fold_pattern_kernel(FoldSetup s) {
  extern __shared__ uint32_t g[];
  const int lane = threadIdx.x;
  const int64_t R = blockIdx.x;
  if (R >= s.n_f) return;
  const int dim = s.dim;
  const int64_t F = R / dim;
  const int c = (int)(R % dim);
  const int t0 = s.copy_ptr[F], t1 = s.copy_ptr[F + 1];
  int L = 0;
  for (int t = t0; t < t1; ++t) {
    const int64_t row = (int64_t)s.copies[t] * dim + c;
    const int64_t beg = s.rowptr_u[row];
    const int len = (int)(s.rowptr_u[row + 1] - beg);
    for (int k = lane; k < len; k += 64) {
      int32_t col = s.col_u[beg + k];
      if (col < 0 || col >= s.n_u) {
        *s.status = 1;
        col = 0;
      }
      g[L + k] = (uint32_t)(s.node_map[col / dim] * dim + col % dim);
    }
    L += len;
  }
  __builtin_amdgcn_wave_barrier();
  // duplicate marks (the comparisons read the column bits only: a concurrent mark of another entry does not change them)
  bool serial = false;
  int n_first = 0;
  {
    int off = 0;
    for (int t = t0; t < t1; ++t) {
      const int64_t row = (int64_t)s.copies[t] * dim + c;
      const int len = (int)(s.rowptr_u[row + 1] - s.rowptr_u[row]);
      for (int k = lane; k < len; k += 64) {
        const int e = off + k;
        const uint32_t v = g[e] & ~kFoldDup;
        bool dup = false;
        for (int q = 0; q < e; ++q) {
          if ((g[q] & ~kFoldDup) == v) {
            dup = true;
            serial = serial || q >= off;
          }
        }
        if (dup) g[e] = v | kFoldDup;
        else ++n_first;
      }
      off += len;
    }
  }
  __builtin_amdgcn_wave_barrier();
  const bool any_serial = __ballot(serial) != 0;
  if constexpr (!FILL) {
    for (int o = 32; o > 0; o >>= 1) n_first += __shfl_xor(n_first, o);
    if (lane == 0) {
      s.count_f[R] = n_first;
      s.serial[R] = any_serial ? 1 : 0;
    }
  } else {
    const int64_t begf = s.rowptr_f[R];
    int off = 0;
    for (int t = t0; t < t1; ++t) {
      const int64_t row = (int64_t)s.copies[t] * dim + c;
      const int64_t beg = s.rowptr_u[row];
      const int len = (int)(s.rowptr_u[row + 1] - beg);
      for (int k = lane; k < len; k += 64) {
        const uint32_t w = g[off + k];
        const uint32_t v = w & ~kFoldDup;
        int pos = 0;
        for (int q = 0; q < L; ++q) {
          const uint32_t x = g[q];
          pos += (!(x & kFoldDup) && x < v) ? 1 : 0;
        }
        s.entry_pos[beg + k] = pos;
        if (!(w & kFoldDup)) s.col_f[begf + pos] = (int32_t)v;
      }
      off += len;
    }
  }
}

struct FoldArgs {
  int dim;
  int64_t n_f;
  const int32_t* copy_ptr;
  const int32_t* copies;
  const int64_t* rowptr_u;
  const int64_t* rowptr_f;
  const int32_t* entry_pos;
  const unsigned char* serial;
  const double* r_u;
  double* r_f;
  const double* A_u;
  const double* A_base;      // nullptr: A_f = P^T A_u P
  double* A_f;
};

// r_f += P^T r_u and A_f = A_base + P^T A_u P, one wave per folded row (FOLD_WAVES rows per workgroup, row_cap doubles of
// LDS each): the base row into the image, each source row added in ascending order of the copies, the image stored in
// one coalesced pass.  The residual entry by lane 0 in the same order.
template<int WITH_R>
__global__ __launch_bounds__(64 * FOLD_WAVES) void fold_matrix_kernel(FoldArgs a, int row_cap) {
  extern __shared__ double img_all[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t R = (int64_t)blockIdx.x * FOLD_WAVES + wave;
  if (R >= a.n_f) return;
  const int dim = a.dim;
  const int64_t F = R / dim;
  const int c = (int)(R % dim);
  const int t0 = a.copy_ptr[F], t1 = a.copy_ptr[F + 1];
  double* img = img_all + wave * row_cap;
  const int64_t begf = a.rowptr_f[R];
  const int lenf = (int)(a.rowptr_f[R + 1] - begf);
  for (int k = lane; k < lenf; k += 64) img[k] = a.A_base ? a.A_base[begf + k] : 0.0;
  __builtin_amdgcn_wave_barrier();
  const bool serial = a.serial[R] != 0;
  for (int t = t0; t < t1; ++t) {
    const int64_t row = (int64_t)a.copies[t] * dim + c;
    const int64_t beg = a.rowptr_u[row];
    const int len = (int)(a.rowptr_u[row + 1] - beg);
    if (!serial) {
      for (int k = lane; k < len; k += 64) img[a.entry_pos[beg + k]] += a.A_u[beg + k];
    } else if (lane == 0) {
      for (int k = 0; k < len; ++k) img[a.entry_pos[beg + k]] += a.A_u[beg + k];
    }
    __builtin_amdgcn_wave_barrier();
  }
  for (int k = lane; k < lenf; k += 64) a.A_f[begf + k] = img[k];
  if constexpr (WITH_R) {
    if (lane == 0) {
      double s = a.r_f[R];
      for (int t = t0; t < t1; ++t) s += a.r_u[(int64_t)a.copies[t] * dim + c];
      a.r_f[R] = s;
    }
  }
}

// r_f += P^T r_u, one thread per folded row, the copies in ascending order
__global__ __launch_bounds__(256) void fold_residual_kernel(FoldArgs a) {
  const int64_t R = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (R >= a.n_f) return;
  const int dim = a.dim;
  const int64_t F = R / dim;
  const int c = (int)(R % dim);
  double s = a.r_f[R];
  for (int t = a.copy_ptr[F]; t < a.copy_ptr[F + 1]; ++t) s += a.r_u[(int64_t)a.copies[t] * dim + c];
  a.r_f[R] = s;
}

// u_u = P u_f, one thread per unwrapped dof
__global__ __launch_bounds__(256) void fold_expand_kernel(int dim, int64_t n_u, const int32_t* __restrict__ node_map,
                                                          const double* __restrict__ u_f, double* __restrict__ u_u) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_u) return;
  const int64_t n = i / dim;
  u_u[i] = u_f[(int64_t)node_map[n] * dim + (i - n * dim)];
}

}  // namespace mimi_hip

using namespace mimi_hip;

struct mimi_hip_fold_s : StreamHandle {
  int dim = 0, row_cap = 0;
  int64_t n_nodes_u = 0, n_nodes_f = 0, n_u = 0, n_f = 0, nnz_u = 0, nnz_f = 0, n_serial = 0;
  DeviceBuffer<int32_t> node_map, copy_ptr, copies, col_f, entry_pos;
  DeviceBuffer<int64_t> rowptr_u, rowptr_f;
  DeviceBuffer<unsigned char> serial;
  DeviceBuffer<double> stage_uf, stage_uu, stage_ru, stage_rf, stage_Au, stage_Ab, stage_Af;
};

// apply_seam.hpp: what the folded product of the Krylov solvers reads of the handle
namespace mimi_hip {
int operator_device(const mimi_hip_fold_s* h) { return h->device; }
OperatorFold operator_fold(const mimi_hip_fold_s* h) {
  return OperatorFold{h->dim, h->n_nodes_u, h->n_nodes_f, h->node_map.ptr, h->copy_ptr.ptr, h->copies.ptr};
}
}  // namespace mimi_hip

extern "C" {

int mimi_hip_fold_create(int32_t dim, int64_t n_nodes_u, const int64_t* node_map, const int64_t* rowptr_u,
                         const int32_t* col_u, int device, mimi_hip_fold_t* out) {
  return guarded([&] {
    if (!out || !node_map || !rowptr_u || !col_u) fail("null argument");
    if (dim < 1 || dim > 3) fail("Unsupported Dim: %d", dim);
    if (n_nodes_u < 1 || n_nodes_u * dim >= ((int64_t)1 << 31)) fail("n_nodes_u %lld out of range", (long long)n_nodes_u);
    auto h = std::make_unique<mimi_hip_fold_s>();
    h->open(device);
    h->dim = dim;
    h->n_nodes_u = n_nodes_u;
    h->n_u = n_nodes_u * dim;
    // the node map and the copies of every folded node (a counting sort: ascending unwrapped index within a node)
    const std::vector<int64_t> map = to_host(node_map, (size_t)n_nodes_u);
    int64_t n_nodes_f = 0;
    for (int64_t m : map) {
      if (m < 0 || m >= n_nodes_u) fail("node_map value %lld out of range [0,%lld)", (long long)m, (long long)n_nodes_u);
      n_nodes_f = std::max(n_nodes_f, m + 1);
    }
    std::vector<int32_t> map32(map.begin(), map.end()), cptr((size_t)n_nodes_f + 1, 0), copies((size_t)n_nodes_u);
    for (int64_t m : map) ++cptr[m + 1];
    for (int64_t F = 0; F < n_nodes_f; ++F) {
      if (cptr[F + 1] == 0) fail("node_map is not onto [0,%lld): folded node %lld has no copy", (long long)n_nodes_f, (long long)F);
      cptr[F + 1] += cptr[F];
    }
    {
      std::vector<int32_t> fill(cptr.begin(), cptr.end() - 1);
      for (int64_t n = 0; n < n_nodes_u; ++n) copies[fill[map[n]]++] = (int32_t)n;
    }
    h->n_nodes_f = n_nodes_f;
    h->n_f = n_nodes_f * dim;
    h->node_map.assign(map32.data(), map32.size(), h->stream);
    h->copy_ptr.assign(cptr.data(), cptr.size(), h->stream);
    h->copies.assign(copies.data(), copies.size(), h->stream);
    // the unwrapped pattern: rowptr kept, col read at set-up only
    const std::vector<int64_t> rp = to_host(rowptr_u, (size_t)h->n_u + 1);
    if (rp[0] != 0) fail("rowptr_u[0] must be 0");
    h->nnz_u = rp[h->n_u];
    int64_t gather = 0;
    for (int64_t F = 0; F < n_nodes_f; ++F)
      for (int c = 0; c < dim; ++c) {
        int64_t L = 0;
        for (int t = cptr[F]; t < cptr[F + 1]; ++t) {
          const int64_t row = (int64_t)copies[t] * dim + c;
          if (rp[row + 1] < rp[row]) fail("rowptr_u is not non-decreasing");
          L += rp[row + 1] - rp[row];
        }
        gather = std::max(gather, L);
      }
    if (gather > FOLD_MAX_GATHER)
      fail("the source rows of a folded row hold %lld entries; the fold supports at most %d", (long long)gather, FOLD_MAX_GATHER);
    h->rowptr_u.assign(rp.data(), rp.size(), h->stream);
    DeviceBuffer<int32_t> col_tmp;
    const int32_t* col_dev = col_u;
    if (!is_device_pointer(col_u)) {
      col_tmp.assign(col_u, (size_t)h->nnz_u, h->stream);
      col_dev = col_tmp.ptr;
    }
    h->serial.resize((size_t)h->n_f);
    DeviceBuffer<int64_t> count_f;
    count_f.resize((size_t)h->n_f);
    FoldSetup s{};
    s.dim = dim;
    s.n_f = h->n_f;
    s.n_u = h->n_u;
    s.node_map = h->node_map.ptr;
    s.copy_ptr = h->copy_ptr.ptr;
    s.copies = h->copies.ptr;
    s.rowptr_u = h->rowptr_u.ptr;
    s.col_u = col_dev;
    s.count_f = count_f.ptr;
    s.serial = h->serial.ptr;
    DeviceBuffer<int> status;
    status.resize(1);
    MH_HIP(hipMemsetAsync(status.ptr, 0, sizeof(int), h->stream));
    s.status = status.ptr;
    const size_t lds = (size_t)std::max<int64_t>(gather, 1) * sizeof(uint32_t);
    ensure_dynamic_lds((const void*)fold_pattern_kernel<0>, (int)lds);
    ensure_dynamic_lds((const void*)fold_pattern_kernel<1>, (int)lds);
    hipLaunchKernelGGL((fold_pattern_kernel<0>), dim3((unsigned)h->n_f), dim3(64), lds, h->stream, s);
    MH_HIP(hipGetLastError());
    // the folded rowptr (a prefix sum of ~10^6 counts, on the host)
    std::vector<int64_t> cnt((size_t)h->n_f), rpf((size_t)h->n_f + 1, 0);
    std::vector<unsigned char> ser((size_t)h->n_f);
    int st = 0;
    MH_HIP(hipMemcpyAsync(&st, status.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipMemcpyAsync(cnt.data(), count_f.ptr, cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipMemcpyAsync(ser.data(), h->serial.ptr, ser.size(), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    if (st) fail("col_u holds a column outside [0,%lld)", (long long)h->n_u);
    int64_t longest = 0;
    for (int64_t R = 0; R < h->n_f; ++R) {
      rpf[R + 1] = rpf[R] + cnt[R];
      longest = std::max(longest, cnt[R]);
      h->n_serial += ser[R];
    }
    if (longest > FOLD_MAX_ROW)
      fail("a folded row holds %lld entries; the fold supports at most %d", (long long)longest, FOLD_MAX_ROW);
    h->nnz_f = rpf[h->n_f];
    h->row_cap = (int)((longest + 7) / 8 * 8);
    h->rowptr_f.assign(rpf.data(), rpf.size(), h->stream);
    h->col_f.resize((size_t)std::max<int64_t>(h->nnz_f, 1));
    h->entry_pos.resize((size_t)std::max<int64_t>(h->nnz_u, 1));
    s.rowptr_f = h->rowptr_f.ptr;
    s.col_f = h->col_f.ptr;
    s.entry_pos = h->entry_pos.ptr;
    hipLaunchKernelGGL((fold_pattern_kernel<1>), dim3((unsigned)h->n_f), dim3(64), lds, h->stream, s);
    MH_HIP(hipGetLastError());
    MH_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
  });
}

int64_t mimi_hip_fold_info(mimi_hip_fold_t h, int what) {
  if (!h) return -1;
  switch (what) {
    case MIMI_HIP_FOLD_INFO_N_NODES_F: return h->n_nodes_f;
    case MIMI_HIP_FOLD_INFO_NNZ_F: return h->nnz_f;
    case MIMI_HIP_FOLD_INFO_NNZ_U: return h->nnz_u;
    case MIMI_HIP_FOLD_INFO_ROW_CAPACITY: return h->row_cap;
    case MIMI_HIP_FOLD_INFO_SERIAL_ROWS: return h->n_serial;
    default: return -1;
  }
}

int mimi_hip_fold_pattern(mimi_hip_fold_t h, int64_t* rowptr_f, int32_t* col_f) {
  return guarded([&] {
    if (!h || !rowptr_f) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipMemcpyAsync(rowptr_f, h->rowptr_f.ptr, ((size_t)h->n_f + 1) * sizeof(int64_t), hipMemcpyDefault, h->stream));
    if (col_f && h->nnz_f)
      MH_HIP(hipMemcpyAsync(col_f, h->col_f.ptr, (size_t)h->nnz_f * sizeof(int32_t), hipMemcpyDefault, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_fold_set_stream(mimi_hip_fold_t h, void* stream) { return handle_set_stream(h, stream); }
int mimi_hip_fold_synchronize(mimi_hip_fold_t h) { return handle_synchronize(h); }
int mimi_hip_fold_destroy(mimi_hip_fold_t h) { return handle_destroy(h); }

int mimi_hip_fold_expand(mimi_hip_fold_t h, const double* u_f, double* u_u) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!u_f || !u_u) fail("null vector argument");
    MH_HIP(hipSetDevice(h->device));
    Mirror<double> mf = Mirror<double>::in(u_f, h->n_f, h->stage_uf, h->stream);
    Mirror<double> mu = Mirror<double>::inout(u_u, h->n_u, h->stage_uu, h->stream);
    hipLaunchKernelGGL(fold_expand_kernel, dim3((unsigned)((h->n_u + 255) / 256)), dim3(256), 0, h->stream, h->dim, h->n_u,
                       h->node_map.ptr, mf.dev, mu.dev);
    MH_HIP(hipGetLastError());
    mu.finish(h->stream);
    if (mf.host || mu.host) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_fold_add(mimi_hip_fold_t h, const double* r_u, double* r_f, const double* A_u, const double* A_base,
                      double* A_f) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!r_u != !r_f) fail("r_u and r_f must both be given or both be NULL");
    if (A_u && !A_f) fail("A_f must be given with A_u");
    if (!r_u && !A_u) return;
    MH_HIP(hipSetDevice(h->device));
    FoldArgs a{};
    a.dim = h->dim;
    a.n_f = h->n_f;
    a.copy_ptr = h->copy_ptr.ptr;
    a.copies = h->copies.ptr;
    a.rowptr_u = h->rowptr_u.ptr;
    a.rowptr_f = h->rowptr_f.ptr;
    a.entry_pos = h->entry_pos.ptr;
    a.serial = h->serial.ptr;
    Mirror<double> mru, mrf, mAu, mAb, mAf;
    if (r_u) {
      mru = Mirror<double>::in(r_u, h->n_u, h->stage_ru, h->stream);
      mrf = Mirror<double>::inout(r_f, h->n_f, h->stage_rf, h->stream);
      a.r_u = mru.dev;
      a.r_f = mrf.dev;
    }
    if (A_u) {
      mAu = Mirror<double>::in(A_u, h->nnz_u, h->stage_Au, h->stream);
      if (A_base == A_f) {
        mAf = Mirror<double>::inout(A_f, h->nnz_f, h->stage_Af, h->stream);
        a.A_base = mAf.dev;
      } else {
        // a host A_f that is not also the base is written whole: nothing to upload
        if (A_base) mAb = Mirror<double>::in(A_base, h->nnz_f, h->stage_Ab, h->stream);
        if (is_device_pointer(A_f)) {
          mAf.dev = A_f;
        } else {
          h->stage_Af.resize((size_t)h->nnz_f);
          mAf.dev = h->stage_Af.ptr;
          mAf.host = A_f;
          mAf.count = (size_t)h->nnz_f;
        }
        a.A_base = mAb.dev;
      }
      a.A_u = mAu.dev;
      a.A_f = mAf.dev;
      const size_t lds = (size_t)FOLD_WAVES * h->row_cap * sizeof(double);
      const unsigned blocks = (unsigned)((h->n_f + FOLD_WAVES - 1) / FOLD_WAVES);
      if (r_u) {
        ensure_dynamic_lds((const void*)fold_matrix_kernel<1>, (int)lds);
        hipLaunchKernelGGL((fold_matrix_kernel<1>), dim3(blocks), dim3(64 * FOLD_WAVES), lds, h->stream, a, h->row_cap);
      } else {
        ensure_dynamic_lds((const void*)fold_matrix_kernel<0>, (int)lds);
        hipLaunchKernelGGL((fold_matrix_kernel<0>), dim3(blocks), dim3(64 * FOLD_WAVES), lds, h->stream, a, h->row_cap);
      }
    } else {
      hipLaunchKernelGGL(fold_residual_kernel, dim3((unsigned)((h->n_f + 255) / 256)), dim3(256), 0, h->stream, a);
    }
    MH_HIP(hipGetLastError());
    if (r_u) mrf.finish(h->stream);
    if (A_u) mAf.finish(h->stream);
    if (mru.host || mrf.host || mAu.host || mAb.host || mAf.host) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"
