// Dispatch of what a handle computes per node beside its assemblies: the field output, the linear forms and the matrix-free
// tangent action, on top of domain_dispatch.hpp (its tables, adjacency and switches): the element kernel of the handle's
// route, then (nodal fields, body force, action) node_gather_kernel over the handle's adjacency.
#pragma once

#include "domain_dispatch.hpp"
#include "kernels_diagonal.hpp"

namespace mimi_hip {

// ---- field output (kernels_fields.hpp) ---------------------------------------------------------------------------------

// by_material_family with neo-Hookean as a family of its own (FIELD_NEOHOOKEAN)
template<class F>
void by_field_family(int kind, F&& f) {
  if (kind == MIMI_HIP_MAT_NEOHOOKEAN) f(std::integral_constant<int, FIELD_NEOHOOKEAN>{});
  else by_material_family(kind, f);
}

// N[e][q][a] of the general route's nodal form: the caller's on a flat-table handle, expanded from the 1-D tables on a
// patch handle
inline void ensure_shape_values(mimi_hip_domain_s* h) {
  if (h->shape_N.ptr) return;
  if (!h->geo.ptr)
    fail("nodal field on a flat-table handle: the tables carry no shape values, give them with mimi_hip_domain_set_shape_values");
  const int64_t total = (int64_t)h->n_el * h->n_q * h->n_dof;
  h->shape_N.resize((size_t)total);
  by_dim(h, [&](auto D) {
    launch(expand_shape_kernel<decltype(D)::value>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, patch_dev(h, nullptr),
           h->shape_N.ptr);
  });
}

// sum[node][c < ncomp] (+ weight[node] when stride == ncomp + 1 and a weight is given) += the element pieces [e][a][stride]
// over the handle's adjacency: one thread per (node, column)
inline void launch_node_gather(mimi_hip_domain_s* h, int stride, int ncomp, const double* pieces, double* sum, double* weight,
                               hipStream_t stream) {
  const NodeAdjacency na = node_adjacency(h);
  const int64_t n_nodes = h->n_vdofs / h->dim;
  launch(node_gather_kernel, dim3((unsigned)((n_nodes * stride + 255) / 256)), dim3(256), 0, stream, n_nodes, h->n_dof, stride, ncomp,
         na.ptr, na.adj, pieces, sum, weight);
}

template<int DIM, int P>
void launch_field_tensor_dp(mimi_hip_domain_s* h, const TensorArgs& a, const FieldArgs& fa) {
  by_field_family(h->mat.m.kind, [&](auto K) {
    launch(field_tensor_kernel<DIM, P, decltype(K)::value>, dim3((unsigned)h->n_el), dim3(FieldShape<DIM, P>::THREADS),
           (size_t)FieldShape<DIM, P>::total(fa.ncomp + 1) * sizeof(double), h->stream, a, fa);
  });
}

// the element kernel of the handle's route: the tensor kernel for every tensor_usable handle (no per-point table is built),
// the general kernel otherwise
inline void launch_field(mimi_hip_domain_s* h, const double* u, FieldArgs fa) {
  const DomainCall c{u};
  if (tensor_usable(h)) {
    const TensorArgs a = tensor_args(h, c);
    by_dim_degree(h, [&](auto D, auto Pd) { launch_field_tensor_dp<decltype(D)::value, decltype(Pd)::value>(h, a, fa); });
    return;
  }
  ensure_general_tables(h);
  if (fa.nodal) {
    ensure_shape_values(h);
    fa.N = h->shape_N.ptr;
  }
  const GeneralArgs a = general_args(h, c);
  const size_t lds = ((size_t)h->n_dof * h->dim + (size_t)(h->dim * h->dim + 1) * h->n_q) * sizeof(double);
  by_field_family(h->mat.m.kind, [&](auto K) {
    by_dim(h, [&](auto D) {
      launch(field_general_kernel<decltype(D)::value, decltype(K)::value>, dim3((unsigned)h->n_el), dim3(256), lds, h->stream, a, fa);
    });
  });
}

// what a field call checks before anything runs; returns the field's components
inline int field_begin(mimi_hip_domain_s* h, const double* u, int field, FieldArgs& fa) {
  MH_HIP(hipSetDevice(h->device));
  const int ncomp = field_components(field, h->dim);
  if (ncomp < 0) fail("unknown field id %d", field);
  const bool of_state = field == MIMI_HIP_FIELD_EQPS || field == MIMI_HIP_FIELD_TEMPERATURE;
  if (of_state && !material_has_state(h->mat.m.kind)) fail("material has no state");
  if (!of_state && !u) fail("null vector argument");
  fa = FieldArgs{};
  fa.field = field;
  fa.ncomp = ncomp;
  fa.need_F = of_state ? 0 : 1;
  return ncomp;
}

// out[e][q][c], overwritten
inline void run_point_field(mimi_hip_domain_s* h, const double* u, int field, double* out, int64_t capacity) {
  FieldArgs fa;
  const int ncomp = field_begin(h, u, field, fa);
  if (!out) fail("null argument");
  const int64_t need = h->n_pts * ncomp;
  if (capacity < need) fail("field buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
  Mirror<double> mu;
  if (fa.need_F) mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
  const bool out_host = !is_device_pointer(out);
  if (out_host) h->stage_f.resize((size_t)need);
  fa.out = out_host ? h->stage_f.ptr : out;
  launch_field(h, mu.dev, fa);
  if (out_host) MH_HIP(hipMemcpyAsync(out, fa.out, (size_t)need * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out_host || mu.host) check_status(h);  // synchronous for host-resident arguments
}

// sum[A][c] += ..., weight[A] += ... : element pieces, then one thread per (node, component) over the adjacency
inline void run_nodal_field(mimi_hip_domain_s* h, const double* u, int field, double* sum, double* weight) {
  FieldArgs fa;
  const int ncomp = field_begin(h, u, field, fa);
  if (!sum) fail("null argument");
  const int64_t n_nodes = h->n_vdofs / h->dim;
  Mirror<double> mu, mw;
  if (fa.need_F) mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
  Mirror<double> ms = Mirror<double>::inout(sum, (size_t)n_nodes * ncomp, h->stage_f, h->stream);
  if (weight) mw = Mirror<double>::inout(weight, (size_t)n_nodes, h->stage_w, h->stream);
  h->field_pieces.resize((size_t)h->n_el * h->n_dof * (ncomp + 1));
  fa.nodal = 1;
  fa.out = h->field_pieces.ptr;
  launch_field(h, mu.dev, fa);
  launch_node_gather(h, ncomp + 1, ncomp, h->field_pieces.ptr, ms.dev, mw.dev, h->stream);
  ms.finish(h->stream);
  if (weight) mw.finish(h->stream);
  if (mu.host || ms.host || mw.host) check_status(h);
}

// ---- linear forms (kernels_forms.hpp) ----------------------------------------------------------------------------------

template<int DIM, int P>
void launch_form_tensor_dp(mimi_hip_domain_s* h, int kind, const TensorArgs& a, const FormArgs& fa) {
  const int64_t n = (int64_t)fa.node_n[0] * fa.node_n[1] * fa.node_n[2];
  auto kernel = kind == FORM_MASS ? form_tensor_kernel<DIM, P, FORM_MASS> : form_tensor_kernel<DIM, P, FORM_DIFFUSION>;
  launch(kernel, dim3((unsigned)n), dim3(FormShape<DIM, P>::THREADS), 0, h->stream, a, fa);
}

inline void launch_form_tensor(mimi_hip_domain_s* h, int kind, double factor, double* A) {
  const TensorArgs a = tensor_args(h, DomainCall{});
  FormArgs fa{};
  fa.factor = factor;
  fa.A = A;
  fa.node_ids = h->node_ids.ptr;
  fa.pos_mode = h->structured_csr ? 0 : h->structured_perm ? (h->degree[0] == 3 ? 2 : 1) : 3;
  if (fa.pos_mode == 3 && !h->pair_pos.ptr) fail("pair positions were not built for this handle");
  const std::vector<int32_t> first = to_host(h->first1d.ptr, h->first1d.count);
  for (int d = 0; d < 3; ++d) {
    fa.node_lo[d] = 0;
    fa.node_n[d] = 1;
    if (d >= h->dim) continue;
    fa.node_lo[d] = first[h->first_off[d] + h->el_begin[d]];
    fa.node_n[d] = first[h->first_off[d] + h->el_end[d] - 1] + h->degree[d] + 1 - fa.node_lo[d];
  }
  by_dim_degree(h, [&](auto D, auto Pd) { launch_form_tensor_dp<decltype(D)::value, decltype(Pd)::value>(h, kind, a, fa); });
}

inline void launch_form_general(mimi_hip_domain_s* h, int kind, double factor, double* A) {
  if (kind == FORM_MASS && !h->shape_N.ptr && !h->geo.ptr) ensure_shape_values(h);   // (fails before anything is built)
  ensure_general_tables(h);
  if (kind == FORM_MASS) ensure_shape_values(h);
  if (longest_row(h) > GG_MAX_ROW) fail("mass / diffusion form: a CSR row of %lld entries is longer than the row image (%d)", (long long)longest_row(h), GG_MAX_ROW);
  const NodeAdjacency na = node_adjacency(h);
  const int64_t n_nodes = h->n_vdofs / h->dim;
  by_dim(h, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    launch(kind == FORM_MASS ? form_general_kernel<DIM, FORM_MASS> : form_general_kernel<DIM, FORM_DIFFUSION>,
           dim3((unsigned)((n_nodes + GG_WAVES - 1) / GG_WAVES)), dim3(64 * GG_WAVES), 0, h->stream, n_nodes, h->n_dof, h->n_q, h->rowptr, na.ptr,
           na.adj, (const int32_t*)h->pair_pos.ptr, (const double*)h->shape_N.ptr, (const double*)h->dN_dX.ptr, (const double*)h->wdet.ptr,
           factor, A);
  });
}

// A_values += factor * (mass | diffusion form); A host or device
inline void run_form(mimi_hip_domain_s* h, int kind, double factor, double* A_values) {
  MH_HIP(hipSetDevice(h->device));
  if (!A_values) fail("null argument");
  Mirror<double> mA = Mirror<double>::inout(A_values, h->nnz, h->stage_A, h->stream);
  if (tensor_usable(h)) launch_form_tensor(h, kind, factor, mA.dev);
  else launch_form_general(h, kind, factor, mA.dev);
  mA.finish(h->stream);
  if (mA.host) check_status(h);   // synchronous for host-resident arguments
}

// r += b (x) lumped weight; b on the host, r host or device
inline void run_body_force(mimi_hip_domain_s* h, const double* b, double* r) {
  MH_HIP(hipSetDevice(h->device));
  if (!b || !r) fail("null argument");
  const int64_t n_nodes = h->n_vdofs / h->dim;
  Mirror<double> mr = Mirror<double>::inout(r, h->n_vdofs, h->stage_r, h->stream);
  // the nodal field output with no component: element pieces of w det N_a alone, gathered into a zeroed weight.  (The field
  // named is det F without u: the point routine returns det 0 = 0 before it reads any state or material, and with ncomp 0
  // nothing of it is staged -- the field kernels run as they are.)
  FieldArgs fa{};
  fa.field = MIMI_HIP_FIELD_DET_F;
  fa.ncomp = 0;
  fa.nodal = 1;
  h->field_pieces.resize((size_t)h->n_el * h->n_dof);
  fa.out = h->field_pieces.ptr;
  launch_field(h, nullptr, fa);
  h->lumped_w.resize((size_t)n_nodes);
  MH_HIP(hipMemsetAsync(h->lumped_w.ptr, 0, (size_t)n_nodes * sizeof(double), h->stream));
  launch_node_gather(h, 1, 0, h->field_pieces.ptr, nullptr, h->lumped_w.ptr, h->stream);
  by_dim(h, [&](auto D) {
    launch(form_body_force_kernel<decltype(D)::value>, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, h->stream, n_nodes,
           (const double*)h->lumped_w.ptr, b[0], b[1], h->dim == 3 ? b[2] : 0.0, mr.dev);
  });
  mr.finish(h->stream);
  if (mr.host) check_status(h);
}

// ---- tangent action (kernels_apply.hpp) ----------------------------------------------------------------------------------

// the kernel family an action runs on, with the codes of last_family: the tensor route for every tensor_usable handle
inline int apply_family_of(const mimi_hip_domain_s* h) {
  if (tensor_small(h)) return MIMI_HIP_FAMILY_TENSOR_SMALL;
  if (tensor_usable(h)) return h->degree[0] == 3 ? MIMI_HIP_FAMILY_TENSOR_P3_TWO_PHASE : MIMI_HIP_FAMILY_TENSOR_P2_TWO_PHASE;
  return MIMI_HIP_FAMILY_GENERAL;
}

// the one switch over what a linearisation leaves: the neo-Hookean action recomputes, every other material has the record
inline bool apply_recomputes(const mimi_hip_domain_s* h) { return h->mat.m.kind == MIMI_HIP_MAT_NEOHOOKEAN; }

// what every kernel of kernels_apply.hpp reads of the handle; the coefficients are the action's own
inline ApplyArgs apply_args(const mimi_hip_domain_s* h, const double* x, const double* u_lin) {
  ApplyArgs aa{};
  aa.x = x;
  aa.u_lin = u_lin;
  aa.rec = h->lin_rec.ptr;
  aa.pieces = h->scratch_r.ptr;
  aa.N = h->shape_N.ptr;
  aa.n_pts = h->n_pts;
  aa.n_el = h->n_el;
  return aa;
}

template<int DIM, int P, int MODE, int FAMILY = 0>
void launch_apply_tensor_dp(mimi_hip_domain_s* h, const TensorArgs& a, const ApplyArgs& aa, hipStream_t stream) {
  using S = ApplyShape<DIM, P, MODE>;
  launch(apply_tensor_kernel<DIM, P, MODE, FAMILY>, dim3((unsigned)((h->n_el + S::EPW - 1) / S::EPW)), dim3(S::THREADS),
         (size_t)S::total * S::EPW * sizeof(double), stream, a, aa);
}

template<int MODE, int FAMILY = 0>
void launch_apply_general(mimi_hip_domain_s* h, const ApplyArgs& aa, hipStream_t stream) {
  const GeneralArgs a = general_args(h, DomainCall{});
  const size_t lds = ((size_t)2 * h->n_dof * h->dim + (size_t)h->dim * (h->dim + 1) * h->n_q) * sizeof(double);
  by_dim(h, [&](auto D) { launch(apply_general_kernel<decltype(D)::value, MODE, FAMILY>, dim3((unsigned)h->n_el), dim3(256), lds, stream, a, aa); });
}

// what an action needs beyond the handle's own tables, built on h->stream at first use; true when something was launched
inline bool apply_prepare(mimi_hip_domain_s* h, double density) {
  MH_HIP(hipSetDevice(h->device));
  bool built = false;
  if (!tensor_usable(h)) {
    // (the mass term on a flat-table handle fails here like add_mass, before anything is built)
    if (density != 0.0 && !h->shape_N.ptr) {
      ensure_shape_values(h);
      built = true;
    }
    if (!h->dN_dX.ptr) built = true;
    ensure_general_tables(h);
  }
  if (!h->adj_ptr.ptr) built = true;
  node_adjacency(h);
  const size_t need = (size_t)h->n_el * h->n_dof * h->dim;
  if (h->scratch_r.count < need) {
    MH_HIP(hipStreamSynchronize(h->stream));   // (nothing in flight reads the pieces that are released)
    h->scratch_r.resize(need);
  }
  return built;
}

inline void apply_check(const mimi_hip_domain_s* h, double stiffness, const char* who = "mimi_hip_domain_apply_tangent") {
  if (stiffness != 0.0 && !h->linearized)
    fail("%s with a stiffness coefficient before any mimi_hip_domain_linearize on this handle", who);
}

// y += density M x + stiffness K(u_lin) x + viscosity C x on `stream`; x, y on the device; apply_prepare has run
inline void launch_apply(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, const double* x, double* y,
                         hipStream_t stream) {
  h->integrated = false;   // the element pieces of an earlier mimi_hip_domain_integrate are overwritten
  ApplyArgs aa = apply_args(h, x, h->lin_u.ptr);
  aa.density = density;
  aa.stiffness = stiffness;
  aa.viscosity = viscosity;
  const bool recompute = apply_recomputes(h);
  if (tensor_usable(h)) {
    const TensorArgs a = tensor_args(h, DomainCall{});
    by_dim_degree(h, [&](auto D, auto Pd) {
      constexpr int DIM = decltype(D)::value, P = decltype(Pd)::value;
      if (recompute) launch_apply_tensor_dp<DIM, P, APPLY_NEOHOOKEAN>(h, a, aa, stream);
      else launch_apply_tensor_dp<DIM, P, APPLY_RECORD>(h, a, aa, stream);
    });
  } else {
    if (recompute) launch_apply_general<APPLY_NEOHOOKEAN>(h, aa, stream); else launch_apply_general<APPLY_RECORD>(h, aa, stream);
  }
  launch_node_gather(h, h->dim, h->dim, h->scratch_r.ptr, y, nullptr, stream);
  h->apply_family = apply_family_of(h);
}

inline void run_apply_tangent(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, const double* x, double* y) {
  MH_HIP(hipSetDevice(h->device));
  if (!x || !y) fail("null vector argument");
  apply_check(h, stiffness);
  apply_prepare(h, density);
  Mirror<double> mx = Mirror<double>::in(x, h->n_vdofs, h->stage_x, h->stream);
  Mirror<double> my = Mirror<double>::inout(y, h->n_vdofs, h->stage_r, h->stream);
  launch_apply(h, density, stiffness, viscosity, mx.dev, my.dev, h->stream);
  my.finish(h->stream);
  if (mx.host || my.host) check_status(h);   // synchronous for host-resident arguments
}

// ---- tangent diagonal (kernels_diagonal.hpp) -----------------------------------------------------------------------------

// apply_prepare, and the element pieces [n_el][n_dof][ncomp]; true when something was launched
inline bool diagonal_prepare(mimi_hip_domain_s* h, double density, int block) {
  const bool built = apply_prepare(h, density);
  const size_t need = (size_t)h->n_el * h->n_dof * (block ? h->dim * h->dim : h->dim);
  if (h->scratch_r.count < need) {
    MH_HIP(hipStreamSynchronize(h->stream));   // (nothing in flight reads the pieces that are released)
    h->scratch_r.resize(need);
  }
  return built;
}

// d += the diagonal (block == 0: [A][i]) or the node blocks (block != 0: [A][i][j]) of density M + stiffness K(u_lin) +
// viscosity C on `stream`; d on the device; diagonal_prepare has run
inline void launch_diagonal(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, int block, double* d,
                            hipStream_t stream) {
  h->integrated = false;   // the element pieces of an earlier mimi_hip_domain_integrate are overwritten
  DiagonalArgs da{};
  da.density = density;
  da.stiffness = stiffness;
  da.viscosity = viscosity;
  da.u_lin = h->lin_u.ptr;
  da.rec = h->lin_rec.ptr;
  da.pieces = h->scratch_r.ptr;
  da.N = h->shape_N.ptr;
  da.n_pts = h->n_pts;
  da.n_el = h->n_el;
  da.block = block ? 1 : 0;
  const bool recompute = apply_recomputes(h);
  if (tensor_usable(h)) {
    const TensorArgs a = tensor_args(h, DomainCall{});
    by_dim_degree(h, [&](auto D, auto Pd) {
      constexpr int DIM = decltype(D)::value, P = decltype(Pd)::value;
      auto go = [&](auto M) {
        using S = DiagonalShape<DIM, P, decltype(M)::value>;
        launch(diagonal_tensor_kernel<DIM, P, decltype(M)::value>, dim3((unsigned)((h->n_el + S::EPW - 1) / S::EPW)), dim3(S::THREADS),
               (size_t)S::total * S::EPW * sizeof(double), stream, a, da);
      };
      if (recompute) go(std::integral_constant<int, APPLY_NEOHOOKEAN>{}); else go(std::integral_constant<int, APPLY_RECORD>{});
    });
  } else {
    const GeneralArgs a = general_args(h, DomainCall{});
    // (the record route keeps nothing per point in LDS)
    const size_t lds = ((size_t)h->n_dof * h->dim + (recompute ? (size_t)(h->dim * h->dim + 1) * h->n_q : 0)) * sizeof(double);
    if (lds > 64 * 1024)
      fail("tangent diagonal: an element of %d nodes and %d points needs %zu bytes of LDS, a workgroup has 65536", h->n_dof, h->n_q, lds);
    by_dim(h, [&](auto D) {
      constexpr int DIM = decltype(D)::value;
      launch(recompute ? diagonal_general_kernel<DIM, APPLY_NEOHOOKEAN> : diagonal_general_kernel<DIM, APPLY_RECORD>, dim3((unsigned)h->n_el),
             dim3(256), lds, stream, a, da);
    });
  }
  const int ncomp = block ? h->dim * h->dim : h->dim;
  launch_node_gather(h, ncomp, ncomp, h->scratch_r.ptr, d, nullptr, stream);
}

inline void run_tangent_diagonal(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, int block, double* d) {
  MH_HIP(hipSetDevice(h->device));
  if (!d) fail("null vector argument");
  apply_check(h, stiffness, "mimi_hip_domain_tangent_diagonal");
  diagonal_prepare(h, density, block);
  Mirror<double> md = Mirror<double>::inout(d, (size_t)h->n_vdofs * (block ? h->dim : 1), h->stage_f, h->stream);
  launch_diagonal(h, density, stiffness, viscosity, block, md.dev, h->stream);
  md.finish(h->stream);
  if (md.host) check_status(h);   // synchronous for host-resident arguments
}

// the snapshot of the tangent at u: committed state, the dt of set_dt; no state changes
inline void run_linearize(mimi_hip_domain_s* h, const double* u) {
  MH_HIP(hipSetDevice(h->device));
  if (!u) fail("null vector argument");
  // (an action launched by a solver on another stream has ended with its solve: nothing reads what is overwritten here)
  if (apply_recomputes(h)) {
    h->lin_u.resize((size_t)h->n_vdofs);
    MH_HIP(hipMemcpyAsync(h->lin_u.ptr, u, (size_t)h->n_vdofs * sizeof(double), hipMemcpyDefault, h->stream));
    if (!is_device_pointer(u)) MH_HIP(hipStreamSynchronize(h->stream));   // (the caller may overwrite u on return)
  } else {
    Mirror<double> mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
    const int d4 = h->dim * h->dim * h->dim * h->dim;
    h->lin_rec.resize((size_t)h->n_pts * d4);
    const ApplyArgs aa = apply_args(h, nullptr, mu.dev);
    if (tensor_usable(h)) {
      const TensorArgs a = tensor_args(h, DomainCall{});
      by_dim_degree(h, [&](auto D, auto Pd) {
        by_material_family(h->mat.m.kind, [&](auto K) {
          launch_apply_tensor_dp<decltype(D)::value, decltype(Pd)::value, APPLY_LINEARIZE, decltype(K)::value>(h, a, aa, h->stream);
        });
      });
    } else {
      ensure_general_tables(h);
      by_material_family(h->mat.m.kind, [&](auto K) { launch_apply_general<APPLY_LINEARIZE, decltype(K)::value>(h, aa, h->stream); });
    }
    if (mu.host) check_status(h);
  }
  if (!h->lin_event) MH_HIP(hipEventCreateWithFlags(&h->lin_event, hipEventDisableTiming));
  MH_HIP(hipEventRecord(h->lin_event, h->stream));
  h->linearized = true;
}

}  // namespace mimi_hip
