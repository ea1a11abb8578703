// Construction of a domain integrator handle (included by domain.hip): status word, material state, CSR set-up and pair
// positions, and the steps of mimi_hip_domain_create_bspline -- 1-D tables, geometry, connectivity, recognition of the
// structured pattern -- plus the closed-form pattern itself (mimi_hip_bspline_sparsity*).
#pragma once

#include "kernels_general.hpp"
#include "kernels_setup.hpp"
#include "tensor_dispatch.hpp"

namespace mimi_hip {

inline void check_status(mimi_hip_domain_s* h) {
  MH_HIP(hipMemcpyAsync(h->status_host, h->status_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MH_HIP(hipStreamSynchronize(h->stream));
  const int s = *h->status_host;
  if (s) {
    MH_HIP(hipMemsetAsync(h->status_dev, 0, sizeof(int), h->stream));
    if (s & 1) fail("ScalarSolve: root not bracketed by input bounds.");          // solvers/newton.hpp:81-93
    if (s & 2) fail("ScalarSolve: failed to converge in allotted iterations.");   // solvers/newton.hpp:120-132
    if (s & 4) fail("CSR pattern does not contain an element's dof block");
    if (s & 8) fail("geometry map has a non-positive Jacobian determinant");
    fail("device status %d", s);
  }
}

inline void init_common(mimi_hip_domain_s* h, int device, const mimi_hip_material* material) {
  h->open(device);
  h->mat = make_material_dev(*material);
  h->general_two_phase_failed = env_general_no_two_phase();
  MH_HIP(hipMalloc(reinterpret_cast<void**>(&h->status_dev), sizeof(int)));
  MH_HIP(hipMemsetAsync(h->status_dev, 0, sizeof(int), h->stream));
  MH_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->status_host), sizeof(int), hipHostMallocDefault));
  *h->status_host = 0;
}

inline void init_state(mimi_hip_domain_s* h) {
  h->n_pts = (int64_t)h->n_el * h->n_q;
  const int kind = h->mat.m.kind;
  if (!material_has_state(kind)) return;
  // CreateState (materials.cpp:120-133 J2Linear, 151-166 J2, 185-208 J2Simo, 225-252 J2Log): zero matrices / eqps,
  // T = initial; J2Simo: be_old = F_old = I; J2Log: Fp_inv = I
  const int dd = h->dim * h->dim;
  h->eqps.resize(h->n_pts);
  h->temperature.resize(h->n_pts);
  h->plastic_strain.resize(h->n_pts * dd);
  MH_HIP(hipMemsetAsync(h->eqps.ptr, 0, h->n_pts * sizeof(double), h->stream));
  MH_HIP(hipMemsetAsync(h->plastic_strain.ptr, 0, h->n_pts * dd * sizeof(double), h->stream));
  const bool two = kind == MIMI_HIP_MAT_J2LINEAR || kind == MIMI_HIP_MAT_J2SIMO;
  if (two) {
    h->state2.resize(h->n_pts * dd);
    MH_HIP(hipMemsetAsync(h->state2.ptr, 0, h->n_pts * dd * sizeof(double), h->stream));
  }
  // (both host arrays live until the synchronisation at the end: the copies are asynchronous)
  std::vector<double> T(h->n_pts, kind == MIMI_HIP_MAT_J2LINEAR ? 0.0 : h->mat.m.initial_temperature), ones;
  MH_HIP(hipMemcpyAsync(h->temperature.ptr, T.data(), h->n_pts * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (kind == MIMI_HIP_MAT_J2SIMO || kind == MIMI_HIP_MAT_J2LOG) {
    ones.assign(h->n_pts, 1.0);
    for (int i = 0; i < h->dim; ++i) {
      const size_t c = (size_t)i * (h->dim + 1);   // diagonal component of the SoA [component][point] layout
      MH_HIP(hipMemcpyAsync(h->plastic_strain.ptr + c * h->n_pts, ones.data(), h->n_pts * sizeof(double), hipMemcpyHostToDevice, h->stream));
      if (kind == MIMI_HIP_MAT_J2SIMO)
        MH_HIP(hipMemcpyAsync(h->state2.ptr + c * h->n_pts, ones.data(), h->n_pts * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
  }
  MH_HIP(hipStreamSynchronize(h->stream));
}

// the closed-form pattern of a patch with n[d] nodes of degree p[d] per direction (directions beyond dim: one node, degree
// 0); no prefix sums and every row required until the caller says otherwise
inline SparsityDev sparsity_dev(int dim, const int32_t* n, const int32_t* p) {
  SparsityDev S{};
  S.dim = dim;
  for (int d = 0; d < 3; ++d) {
    S.n[d] = d < dim ? n[d] : 1;
    S.p[d] = d < dim ? p[d] : 0;
    S.prefix[d] = nullptr;
  }
  return S;
}

// the CSR columns where kernels can read them: the caller's array, or a copy of it in `tmp`
inline const int32_t* device_columns(mimi_hip_domain_s* h, const int32_t* col, DeviceBuffer<int32_t>& tmp) {
  if (is_device_pointer(col)) return col;
  tmp.assign(col, h->nnz, h->stream);
  return tmp.ptr;
}

// pair_pos[e][a][b]: offset of column dofs[b] * dim inside row dofs[a] * dim (what the general and colour kernels scatter
// through); col = the CSR columns, host or device
inline void build_pair_pos(mimi_hip_domain_s* h, const int32_t* col) {
  DeviceBuffer<int32_t> col_tmp;
  const int32_t* col_dev = device_columns(h, col, col_tmp);
  const int64_t total = (int64_t)h->n_el * h->n_dof * h->n_dof;
  h->pair_pos.resize(total);
  launch(pair_pos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->n_el, h->n_dof, h->dim, h->dofs.ptr,
         h->rowptr, col_dev, h->pair_pos.ptr, h->status_dev);
  check_status(h);
}

// Handles whose CSR is the (possibly permuted) structured pattern do not build pair_pos at create time: the two-phase
// kernels never use it.  The fallback kernels get it here, from columns regenerated out of the pattern's closed form.
inline void ensure_pair_pos(mimi_hip_domain_s* h) {
  if (h->pair_pos.ptr) return;
  if (!(h->structured_csr || h->structured_perm)) fail("pair positions were not built for this handle");
  const SparsityDev S = sparsity_dev(h->dim, h->n_ctrl, h->degree);
  DeviceBuffer<int32_t> col;
  col.resize((size_t)h->nnz);
  const dim3 per_node((unsigned)((h->n_nodes + 3) / 4));
  if (h->structured_csr) {
    const int64_t n_rows = h->n_vdofs;
    launch(structured_col_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, h->stream, S, n_rows, h->rowptr, col.ptr, 0, h->status_dev);
  } else if (h->degree[0] == 3) {
    launch(permuted_col_kernel<uint16_t, 343>, per_node, dim3(256), 0, h->stream, S, (int64_t)h->n_nodes, h->node_ids.ptr, h->rowptr,
           h->nbr_pos16.ptr, col.ptr);
  } else {
    launch(permuted_col_kernel<unsigned char, 125>, per_node, dim3(256), 0, h->stream, S, (int64_t)h->n_nodes, h->node_ids.ptr, h->rowptr,
           h->nbr_pos.ptr, col.ptr);
  }
  build_pair_pos(h, col.ptr);
  MH_HIP(hipStreamSynchronize(h->stream));
}

inline void setup_csr(mimi_hip_domain_s* h, const int64_t* rowptr, const int32_t* col, bool need_pair_pos) {
  if (!rowptr || !col) fail("csr_rowptr / csr_col must be given");
  // rowptr: keep a device copy unless it already lives there
  if (is_device_pointer(rowptr)) {
    h->rowptr = rowptr;
  } else {
    h->rowptr_own.assign(rowptr, h->n_vdofs + 1, h->stream);
    h->rowptr = h->rowptr_own.ptr;
  }
  int64_t nnz = 0;
  MH_HIP(hipMemcpyAsync(&nnz, h->rowptr + h->n_vdofs, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  MH_HIP(hipStreamSynchronize(h->stream));
  h->nnz = nnz;
  if (need_pair_pos) build_pair_pos(h, col);
}

inline PatchDev patch_dev(mimi_hip_domain_s* h, const double* ctrl) {
  PatchDev P{};
  const int dim = h->dim;
  P.dim = dim;
  for (int d = 0; d < 3; ++d) {
    P.p[d] = d < dim ? h->degree[d] : 0;
    P.nq[d] = d < dim ? h->nq1[d] : 1;
    P.n_ctrl[d] = d < dim ? h->n_ctrl[d] : 1;
    P.box_begin[d] = d < dim ? h->el_begin[d] : 0;
    P.box_n[d] = d < dim ? h->el_end[d] - h->el_begin[d] : 1;
    P.B[d] = d < dim ? h->tab1d.ptr + h->tab_off_B[d] : nullptr;
    P.D[d] = d < dim ? h->tab1d.ptr + h->tab_off_D[d] : nullptr;
    P.W[d] = d < dim ? h->tab1d.ptr + h->tab_off_W[d] : nullptr;
    P.first[d] = d < dim ? h->first1d.ptr + h->first_off[d] : nullptr;
  }
  P.ctrl = ctrl;
  P.node_ids = h->node_ids.ptr;
  P.n_dof = h->n_dof;
  P.n_q = h->n_q;
  P.n_el = h->n_el;
  return P;
}

// element connectivity, and with gptr / wptr the reference-layout tables (utils/precomputed.cpp:316-321) from the compact
// geometry
inline void launch_expand_tables(mimi_hip_domain_s* h, const PatchDev& P) {
  const int64_t total = (int64_t)h->n_el * h->n_q * h->n_dof;
  auto kernel = h->dim == 2 ? expand_tables_kernel<2> : expand_tables_kernel<3>;
  launch(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, P, h->geo.ptr, h->dofs.ptr, h->dN_dX.ptr, h->wdet.ptr);
}

// ---- mimi_hip_domain_create_bspline, step by step --------------------------------------------------------------------

// the 1-D tables of every direction and what follows from them: degrees, sizes, the element box
inline void make_patch_tables(mimi_hip_domain_s* h, const mimi_hip_bspline_patch* p, Tables1D t1[3]) {
  const int dim = h->dim;
  int pmax = 0;
  for (int d = 0; d < dim; ++d) pmax = std::max(pmax, p->degree[d]);
  if (pmax < 1 || pmax > 3) fail("degree %d unsupported (1..3)", pmax);
  // precomputed.cpp:284-290: order = 2*GetOrder()+3 when negative; order/2+1 points / direction
  const int order = p->quadrature_order < 0 ? 2 * pmax + 3 : p->quadrature_order;
  const int nq = order / 2 + 1;
  std::vector<double> w1d[3];
  if (p->weights) {
    int64_t nc[3] = {1, 1, 1};
    for (int d = 0; d < dim; ++d) nc[d] = p->n_knots[d] - p->degree[d] - 1;
    factorise_nurbs_weights(p->weights, dim, nc, w1d);
  }
  h->n_nodes = 1;
  h->n_dof = 1;
  h->n_q = 1;
  for (int d = 0; d < dim; ++d) {
    if (p->degree[d] < 1 || p->degree[d] > 3) fail("degree %d unsupported (1..3)", p->degree[d]);
    t1[d] = make_tables_1d(p->knots[d], p->n_knots[d], p->degree[d], nq, p->weights ? w1d[d].data() : nullptr);
    h->degree[d] = p->degree[d];
    h->nq1[d] = nq;
    h->n_ctrl[d] = t1[d].n_ctrl;
    h->el_total[d] = t1[d].n_spans;
    h->n_nodes *= t1[d].n_ctrl;
    h->n_dof *= p->degree[d] + 1;
    h->n_q *= nq;
  }
  if (h->n_q > 125) fail("n_quad %d out of range", h->n_q);
  bool whole = true;
  for (int d = 0; d < 3; ++d) whole = whole && p->element_begin[d] == 0 && p->element_end[d] == 0;
  h->n_el = 1;
  for (int d = 0; d < dim; ++d) {
    h->el_begin[d] = whole ? 0 : p->element_begin[d];
    h->el_end[d] = whole ? h->el_total[d] : p->element_end[d];
    if (h->el_begin[d] < 0 || h->el_end[d] > h->el_total[d] || h->el_begin[d] >= h->el_end[d])
      fail("element box [%d,%d) invalid in direction %d (%d spans)", h->el_begin[d], h->el_end[d], d, h->el_total[d]);
    h->n_el *= h->el_end[d] - h->el_begin[d];
  }
  h->n_vdofs = h->n_nodes * dim;
}

// 1-D tables -> one device buffer:  per direction B, D, W ; first[] in a second buffer
inline void upload_tables_1d(mimi_hip_domain_s* h, const Tables1D t1[3]) {
  std::vector<double> tab;
  std::vector<int32_t> first;
  h->first_is_identity = true;
  for (int d = 0; d < h->dim; ++d) {
    h->tab_off_B[d] = tab.size();
    tab.insert(tab.end(), t1[d].B.begin(), t1[d].B.end());
    h->tab_off_D[d] = tab.size();
    tab.insert(tab.end(), t1[d].D.begin(), t1[d].D.end());
    h->tab_off_W[d] = tab.size();
    tab.insert(tab.end(), t1[d].w.begin(), t1[d].w.end());
    h->first_off[d] = first.size();
    first.insert(first.end(), t1[d].first.begin(), t1[d].first.end());
    for (int k = 0; k < (int)t1[d].first.size(); ++k) h->first_is_identity = h->first_is_identity && (t1[d].first[k] == k);
  }
  h->tab1d.assign(tab.data(), tab.size(), h->stream);
  h->first1d.assign(first.data(), first.size(), h->stream);
}

// dxi/dX and w det per quadrature point, from the control points
inline void compute_geometry(mimi_hip_domain_s* h, const PatchDev& P) {
  const int64_t npts = (int64_t)h->n_el * h->n_q;
  h->geo.resize((size_t)npts * (h->dim * h->dim + 1));
  auto kernel = h->dim == 2 ? geometry_kernel<2> : geometry_kernel<3>;
  launch(kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, h->stream, P, h->geo.ptr, h->status_dev);
  check_status(h);
}

// element connectivity (always) + reference-layout tables (general path / FD mode only)
inline void build_connectivity(mimi_hip_domain_s* h, const PatchDev& P, bool keep_general) {
  h->dofs.resize((size_t)h->n_el * h->n_dof);
  if (keep_general) {
    const int64_t npts = (int64_t)h->n_el * h->n_q;
    h->dN_dX.resize((size_t)npts * h->n_dof * h->dim);
    h->wdet.resize((size_t)npts);
    launch_expand_tables(h, P);
  } else {
    const int64_t total = (int64_t)h->n_el * h->n_dof;
    launch(connectivity_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, P, h->dofs.ptr);
  }
  MH_HIP(hipStreamSynchronize(h->stream));
}

// what the two pattern recognisers share: the caller's columns on the device, a clean status word, the recognising kernel
// (check(columns): it raises the status word on a mismatch), the verdict read back, the status word clean again
template<class Check>
bool csr_matches(mimi_hip_domain_s* h, const int32_t* csr_col, Check&& check) {
  DeviceBuffer<int32_t> col_tmp;
  const int32_t* col_dev = device_columns(h, csr_col, col_tmp);
  MH_HIP(hipMemsetAsync(h->status_dev, 0, sizeof(int), h->stream));
  check(col_dev);
  MH_HIP(hipMemcpyAsync(h->status_host, h->status_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MH_HIP(hipStreamSynchronize(h->stream));
  const bool same = *h->status_host == 0;
  MH_HIP(hipMemsetAsync(h->status_dev, 0, sizeof(int), h->stream));
  return same;
}

// lexicographic numbering + the closed-form pattern => CSR positions are arithmetic
inline bool recognise_structured(mimi_hip_domain_s* h, const int32_t* csr_col, const Tables1D t1[3]) {
  SparsityDev S = sparsity_dev(h->dim, h->n_ctrl, h->degree);
  DeviceBuffer<int64_t> prefix[3];
  for (int d = 0; d < 3; ++d) {
    std::vector<int64_t> pre(S.n[d] + 1, 0);
    prefix[d].assign(pre.data(), pre.size(), h->stream);  // unused by the check kernel
    S.prefix[d] = prefix[d].ptr;
    // a row-sliced pattern must hold the rows of every node this handle's elements touch
    S.req_lo[d] = t1[d].first[h->el_begin[d]];
    S.req_hi[d] = t1[d].first[h->el_end[d] - 1] + h->degree[d] + 1;
  }
  S.partial = 1;
  return csr_matches(h, csr_col, [&](const int32_t* col) {
    const int64_t n_rows = h->n_vdofs;
    launch(structured_col_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, h->stream, S, n_rows, h->rowptr,
           const_cast<int32_t*>(col), 1, h->status_dev);
  });
}

// permuted numbering (node_ids given): is the caller's CSR the permuted structured pattern?  Leaves the rank of each window
// neighbour inside its row (nbr_pos / nbr_pos16)
inline bool recognise_permuted(mimi_hip_domain_s* h, const int32_t* csr_col) {
  const SparsityDev S = sparsity_dev(h->dim, h->n_ctrl, h->degree);
  const int64_t n_nodes = h->n_nodes;
  const dim3 grid((unsigned)((n_nodes + 3) / 4));
  return csr_matches(h, csr_col, [&](const int32_t* col) {
    if (h->degree[0] == 3) {
      h->nbr_pos16.resize((size_t)n_nodes * 343);
      launch(permuted_window_kernel<uint16_t, 343>, grid, dim3(256), 0, h->stream, S, n_nodes, h->node_ids.ptr, h->rowptr, col,
             h->nbr_pos16.ptr, h->status_dev);
    } else {
      h->nbr_pos.resize((size_t)n_nodes * 125);
      launch(permuted_window_kernel<unsigned char, 125>, grid, dim3(256), 0, h->stream, S, n_nodes, h->node_ids.ptr, h->rowptr, col,
             h->nbr_pos.ptr, h->status_dev);
    }
  });
}

// which of the two structured patterns, if any, the caller's CSR is (3-D only; MIMI_HIP_NO_STRUCTURED=1: neither)
inline void recognise_pattern(mimi_hip_domain_s* h, const mimi_hip_bspline_patch* p, const Tables1D t1[3]) {
  h->structured_csr = h->structured_perm = false;
  if (h->dim != 3) return;
  if (!p->node_ids) {
    if (!env_no_structured()) h->structured_csr = recognise_structured(h, p->csr_col, t1);
    return;
  }
  const int* deg = h->degree;
  const bool degree3 = deg[0] == 3 && deg[1] == 3 && deg[2] == 3;
  if (((deg[0] <= 2 && deg[1] <= 2 && deg[2] <= 2) || degree3) && !env_no_structured())
    h->structured_perm = recognise_permuted(h, p->csr_col);
}

// ---- mimi_hip_bspline_sparsity / _rows ---------------------------------------------------------------------------------

// keeps the row lengths of the nodes in [node_begin, node_end), drops the others; the scan runs on the host (n_rows + 1
// integers, set-up only)
inline void slice_rowptr(const SparsityDev& S, int64_t n_nodes, const int32_t* node_begin, const int32_t* node_end, int64_t* rp_dev) {
  const int dim = S.dim;
  const int64_t n_rows = n_nodes * dim;
  for (int d = 0; d < dim; ++d)
    if (node_begin[d] < 0 || node_end[d] > S.n[d] || node_begin[d] >= node_end[d])
      fail("node box [%d,%d) invalid in direction %d (%d nodes)", node_begin[d], node_end[d], d, S.n[d]);
  const std::vector<int64_t> full = to_host(rp_dev, (size_t)n_rows + 1);
  std::vector<int64_t> local(n_rows + 1, 0);
  for (int64_t A = 0; A < n_nodes; ++A) {
    const int Am[3] = {(int)(A % S.n[0]), (int)((A / S.n[0]) % S.n[1]), (int)(A / ((int64_t)S.n[0] * S.n[1]))};
    bool in = true;
    for (int d = 0; d < dim; ++d) in = in && Am[d] >= node_begin[d] && Am[d] < node_end[d];
    for (int i = 0; i < dim; ++i) {
      const int64_t r = A * dim + i;
      local[r + 1] = local[r] + (in ? full[r + 1] - full[r] : 0);
    }
  }
  MH_HIP(hipMemcpy(rp_dev, local.data(), (n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
}

// node_begin / node_end == nullptr: every row; else only the rows of the nodes in that box (others get zero length)
inline int bspline_sparsity(int32_t dim, const int32_t n_nodes_dir[3], const int32_t degree[3], const int32_t* node_begin,
                            const int32_t* node_end, int device, int64_t* rowptr, int32_t* col, int64_t* nnz_out) {
  return guarded([&] {
    if (dim != 2 && dim != 3) fail("Unsupported Dim: %d", dim);
    if ((node_begin == nullptr) != (node_end == nullptr)) fail("node_begin and node_end go together");
    if (!rowptr || !nnz_out) fail("null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) fail("libmimi_hip: no HIP device visible");
    MH_HIP(hipSetDevice(device));
    SparsityDev S = sparsity_dev(dim, n_nodes_dir, degree);
    int64_t n_nodes = 1;
    DeviceBuffer<int64_t> prefix[3];
    for (int d = 0; d < 3; ++d) {
      n_nodes *= S.n[d];
      std::vector<int64_t> pre(S.n[d] + 1, 0);
      for (int A = 0; A < S.n[d]; ++A) {
        const int lo = std::max(A - S.p[d], 0), hi = std::min(A + S.p[d], S.n[d] - 1);
        pre[A + 1] = pre[A] + (hi - lo + 1);
      }
      prefix[d].assign(pre.data(), pre.size(), nullptr);
      S.prefix[d] = prefix[d].ptr;
    }
    const int64_t n_rows = n_nodes * dim;
    DeviceBuffer<int64_t> rp_tmp;
    int64_t* rp_dev = rowptr;
    const bool rp_host = !is_device_pointer(rowptr);
    if (rp_host) {
      rp_tmp.resize(n_rows + 1);
      rp_dev = rp_tmp.ptr;
    }
    launch(structured_rowptr_kernel, dim3((unsigned)((n_nodes + 1 + 255) / 256)), dim3(256), 0, nullptr, S, n_nodes, rp_dev);
    if (node_begin) slice_rowptr(S, n_nodes, node_begin, node_end, rp_dev);
    int64_t nnz = 0;
    MH_HIP(hipMemcpy(&nnz, rp_dev + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost));
    *nnz_out = nnz;
    if (rp_host) MH_HIP(hipMemcpy(rowptr, rp_dev, (n_rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (col) {
      DeviceBuffer<int32_t> col_tmp;
      int32_t* col_dev = col;
      const bool col_host = !is_device_pointer(col);
      if (col_host) {
        col_tmp.resize(nnz);
        col_dev = col_tmp.ptr;
      }
      launch(structured_col_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, nullptr, S, n_rows, rp_dev, col_dev, 0, (int*)nullptr);
      MH_HIP(hipDeviceSynchronize());
      if (col_host) MH_HIP(hipMemcpy(col, col_dev, nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    MH_HIP(hipDeviceSynchronize());
  });
}

}  // namespace mimi_hip
