// Dispatch of one call of the domain integrator: the general kernels and their row gather, the small-element tensor kernels,
// the choice between them and the two-phase tensor kernels (tensor_dispatch.hpp), the field output, the linear forms and the
// matrix-free tangent action.
// Every function reads the call from its DomainCall; the handle keeps only what outlives a call.
#pragma once

#include "domain_create.hpp"
#include "kernels_apply.hpp"
#include "kernels_fields.hpp"
#include "kernels_forms.hpp"
#include "tensor_dispatch.hpp"

namespace mimi_hip {

// reference-layout tables (utils/precomputed.cpp:316-321) from the compact geometry, on demand
inline void ensure_general_tables(mimi_hip_domain_s* h) {
  ensure_pair_pos(h);
  if (h->dN_dX.ptr) return;
  if (!h->geo.ptr) fail("no tables to integrate with");
  const int64_t npts = (int64_t)h->n_el * h->n_q;
  h->dN_dX.resize((size_t)npts * h->n_dof * h->dim);
  h->wdet.resize((size_t)npts);
  launch_expand_tables(h, patch_dev(h, nullptr));
}

inline GeneralArgs general_args(mimi_hip_domain_s* h, const DomainCall& c) {
  GeneralArgs a{};
  a.n_el = h->n_el;
  a.n_dof = h->n_dof;
  a.n_q = h->n_q;
  a.dofs = h->dofs.ptr;
  a.dN_dX = h->dN_dX.ptr;
  a.wdet = h->wdet.ptr;
  a.rowptr = h->rowptr;
  a.pair_pos = h->pair_pos.ptr;
  a.u = c.u;
  a.r = c.r;
  a.A = c.A;
  a.grad_factor = c.grad_factor;
  a.dt = h->dt;
  a.mat = h->mat;
  a.state = StateView{h->eqps.ptr, h->temperature.ptr, h->plastic_strain.ptr, h->n_pts, h->state2.ptr};
  a.status = h->status_dev;
  return a;
}

// calls f(integral_constant DIM, integral_constant P) for a tensor_usable handle (tensor_supported: one degree, 1..3)
template<class F>
void by_dim_degree(const mimi_hip_domain_s* h, F&& f) {
  auto by_degree = [&](auto D) {
    switch (h->degree[0]) {
    case 1: f(D, std::integral_constant<int, 1>{}); break;
    case 2: f(D, std::integral_constant<int, 2>{}); break;
    default: f(D, std::integral_constant<int, 3>{}); break;
    }
  };
  if (h->dim == 2) by_degree(std::integral_constant<int, 2>{}); else by_degree(std::integral_constant<int, 3>{});
}

// node -> incident (element << 6 | local node) lists of the general row gather
inline void fill_adjacency(mimi_hip_domain_s* h, DeviceBuffer<int64_t>& adj_ptr, DeviceBuffer<int32_t>& adj_out) {
  const size_t n = (size_t)h->n_el * h->n_dof;
  const std::vector<int32_t> dofs = to_host(h->dofs.ptr, n);
  const int64_t n_nodes = h->n_vdofs / h->dim;
  std::vector<int64_t> ptr(n_nodes + 1, 0);
  for (size_t k = 0; k < n; ++k) ++ptr[dofs[k] + 1];
  for (int64_t v = 0; v < n_nodes; ++v) ptr[v + 1] += ptr[v];
  std::vector<int32_t> adj(n);
  std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
  for (size_t k = 0; k < n; ++k) adj[fill[dofs[k]]++] = (int32_t)(((k / h->n_dof) << 6) | (k % h->n_dof));
  adj_ptr.assign(ptr.data(), ptr.size(), h->stream);
  adj_out.assign(adj.data(), adj.size(), h->stream);
}

inline void build_adjacency(mimi_hip_domain_s* h) { fill_adjacency(h, h->adj_ptr, h->adj); }

// two-phase general path: element blocks / residual vectors densely into scratch_k / scratch_r, then
// general_gather_kernel.  Needs n_el * n_tdof^2 doubles (77 GB at 128 x 128 x 16 p = 3) and the node -> element adjacency;
// falls back to the atomics when the scratch does not fit (MIMI_HIP_GENERAL_NO_TWO_PHASE=1 forces that)
inline bool ensure_general_two_phase(mimi_hip_domain_s* h, bool with_k) {
  if (env_general_no_two_phase() || h->general_two_phase_failed) return false;
  const size_t n_tdof = (size_t)h->n_dof * h->dim;
  // what rules the path out is checked BEFORE anything is allocated (3-D degree >= 4 would be 1.1 MB per element)
  if (!h->adj_ptr.ptr) {
    // the gather kernel keeps one CSR row in LDS: rows longer than its image -> atomics
    const std::vector<int64_t> rp = to_host(h->rowptr, (size_t)h->n_vdofs + 1);
    int64_t longest = 0;
    for (int64_t v = 0; v < h->n_vdofs; ++v) longest = std::max(longest, rp[v + 1] - rp[v]);
    if (longest > GG_MAX_ROW || h->n_dof > 64) {
      h->general_two_phase_failed = true;
      return false;
    }
  }
  const size_t need = with_k ? (size_t)h->n_el * n_tdof * n_tdof : 0;
  if (h->scratch_k.count < need) {
    size_t free_b = 0, total_b = 0;
    MH_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t have = h->scratch_k.count * sizeof(double);
    if (need * sizeof(double) > free_b + have || need * sizeof(double) > (total_b / 2)) {
      h->general_two_phase_failed = true;
      h->scratch_k.release();          // (whatever a residual-only call left: the atomics route needs none of it)
      h->scratch_r.release();
      return false;
    }
    h->scratch_k.resize(need);
  }
  h->scratch_r.resize((size_t)h->n_el * n_tdof);
  if (!h->adj_ptr.ptr) build_adjacency(h);
  return true;
}

// the row gather of the general path: r += sums of scratch_r, and with a tangent A = A_old + grad_factor * sums of scratch_k
// (A_old: the call's base array, or A itself)
inline void launch_general_gather(mimi_hip_domain_s* h, const DomainCall& c) {
  const int64_t n_rows = h->n_vdofs;
  auto kernel = h->dim == 2 ? (c.grad ? general_gather_kernel<2, 1> : general_gather_kernel<2, 0>)
                            : (c.grad ? general_gather_kernel<3, 1> : general_gather_kernel<3, 0>);
  launch(kernel, dim3((unsigned)((n_rows + GG_WAVES - 1) / GG_WAVES)), dim3(64 * GG_WAVES), 0, h->stream, n_rows, h->n_dof, h->rowptr,
         h->adj_ptr.ptr, h->adj.ptr, h->pair_pos.ptr, h->scratch_k.ptr, h->scratch_r.ptr, c.grad_factor, c.A_old(), c.A, c.r);
}

#ifndef GEN_BIG_PP
#define GEN_BIG_PP 8
#define GEN_BIG_THREADS 512
#endif
template<int DIM>
void launch_general_dim(mimi_hip_domain_s* h, const DomainCall& c) {
  GeneralArgs a = general_args(h, c);
  const int grad = c.grad, kind = h->mat.m.kind;
  // MIMI_HIP_GENERAL_NO_WPE=1: one workgroup per element also for the small ones; MIMI_HIP_GENERAL_NO_MFMA=1: the vector-pipe
  // node-pair phase also for 64-node elements (A/B comparisons)
  const bool no_wpe = env_general_no_wpe(), no_mfma = env_general_no_mfma();
  const bool two_phase = ensure_general_two_phase(h, grad != 0);
  // the atomics add into the values in place: A <- A_base first, on the stream, then "+="
  if (!two_phase && grad && c.A_base && c.A_base != c.A)
    MH_HIP(hipMemcpyAsync(c.A, c.A_base, (size_t)h->nnz * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  a.scratch_k = (two_phase && grad) ? h->scratch_k.ptr : nullptr;
  a.scratch_r = two_phase ? h->scratch_r.ptr : nullptr;
  size_t lds = general_lds_bytes(DIM, h->n_dof, h->n_q, grad);
  if (lds > 160 * 1024) fail("element too large for LDS (%zu bytes)", lds);
  // small elements (one pass of the node-pair phase fits one wave: 2-D p <= 3, 3-D p = 1): one wave per element, four
  // elements per workgroup -- when the LDS blocks of four elements fit (a 3-D tangent assembly with 64 points per element,
  // degrees (2,1,1) / (2,2,1) at the default order, needs 51 - 54 KB per element: one workgroup per element then)
  const bool wpe = !no_wpe && grad != 2 && h->n_dof * ((h->n_dof + 2) / 3) <= 128 && h->n_q <= 64 &&
                   (lds + 15) / 16 * 16 * 4 <= 160 * 1024;
  if (wpe) {
    a.lds_per_element = (int)((lds + 15) / 16 * 16);
    lds = (size_t)a.lds_per_element * 4;
  }
  by_material_family(kind, [&](auto K) {
    // the other materials (materials_other.hpp): the tangent assembly takes P and dP/dF from the material pre-pass (one lean
    // kernel per material: w det P, w det dP/dF per point; the element kernel's family 1), the residual-only and
    // reference-FD assemblies evaluate the stress in the element kernel (family = kind)
    constexpr int FK = decltype(K)::value, REC = FK != 0 ? 1 : 0;
    if constexpr (FK != 0) {
      if (grad == 1) {
        constexpr int DD = DIM * DIM;
        h->mat_rec.resize((size_t)h->n_el * h->n_q * (DD + DD * DD));
        a.mat_rec = h->mat_rec.ptr;
        launch(general_material_kernel<DIM, FK>, dim3(h->n_el), dim3(64), (size_t)h->n_dof * DIM * sizeof(double), h->stream, a);
      }
    }
    auto go = [&](auto kernel, int threads = 256) {
      launch(kernel, dim3(wpe ? (unsigned)((h->n_el + 3) / 4) : (unsigned)h->n_el), dim3(threads), lds, h->stream, a);
    };
    if (wpe) {
      if (grad == 0) go(domain_general_kernel<DIM, 0, 3, 256, FK, 0, 1>); else go(domain_general_kernel<DIM, 1, 3, 256, REC, 0, 1>);
    } else if (grad == 1) {
      if (DIM == 3 && h->n_dof == 64 && !no_mfma) go(domain_general_kernel<3, 1, GEN_BIG_PP, GEN_BIG_THREADS, REC, 1>, GEN_BIG_THREADS);
      else if (h->n_dof * h->n_dof > 3 * 256) go(domain_general_kernel<DIM, 1, GEN_BIG_PP, GEN_BIG_THREADS, REC>, GEN_BIG_THREADS);
      else go(domain_general_kernel<DIM, 1, 3, 256, REC>);
    } else if (grad == 0) {
      go(domain_general_kernel<DIM, 0, 3, 256, FK>);
    } else {
      go(domain_general_kernel<DIM, 2, 3, 256, FK>);
    }
  });
  if (two_phase) launch_general_gather(h, c);
}

inline void launch_general(mimi_hip_domain_s* h, const DomainCall& c) {
  ensure_general_tables(h);
  if (h->dim == 2) launch_general_dim<2>(h, c); else launch_general_dim<3>(h, c);
}

// DomainPostTimeAdvance on the general tables
inline void launch_general_post(mimi_hip_domain_s* h, const DomainCall& c) {
  ensure_general_tables(h);
  const GeneralArgs a = general_args(h, c);
  const size_t lds = (size_t)h->n_dof * h->dim * sizeof(double);
  by_material_family(h->mat.m.kind, [&](auto K) {
    constexpr int REC = decltype(K)::value != 0 ? 1 : 0;
    auto kernel = h->dim == 2 ? post_time_advance_general_kernel<2, REC> : post_time_advance_general_kernel<3, REC>;
    launch(kernel, dim3(h->n_el), dim3(256), lds, h->stream, a);
  });
}

// small elements on the tensor path (kernels_tensor_small.hpp): element kernel from the 1-D tables, then the general
// path's gather (adjacency, pair positions).  mode 0 residual, 1 residual + tangent, 2 post time advance
template<int DIM, int P>
void launch_tensor_small_dp(mimi_hip_domain_s* h, int mode, const TensorArgs& a) {
  using S = SmallShape<DIM, P>;
  const size_t lds = (size_t)4 * (mode == 1 ? S::total1 : S::total0) * sizeof(double);
  by_material_family(h->mat.m.kind, [&](auto K) {
    constexpr int FK = decltype(K)::value;
    auto kernel = mode == 0 ? tensor_small_kernel<DIM, P, FK, 0> : mode == 1 ? tensor_small_kernel<DIM, P, FK, 1> : tensor_small_kernel<DIM, P, FK, 2>;
    launch(kernel, dim3((unsigned)((h->n_el + 3) / 4)), dim3(256), lds, h->stream, a, (int)h->n_el);
  });
}

// commit: the state commit of DomainPostTimeAdvance instead of an assembly.  false: the element blocks do not fit (the caller
// takes the general kernels)
inline bool launch_tensor_small(mimi_hip_domain_s* h, const DomainCall& c, bool commit = false) {
  const int mode = commit ? 2 : c.grad;
  TensorArgs a = tensor_args(h, c);
  if (!commit) {
    ensure_pair_pos(h);
    if (!ensure_general_two_phase(h, mode == 1)) return false;
    a.scratch_k = h->scratch_k.ptr;
    a.scratch_r = h->scratch_r.ptr;
  }
  by_dim_degree(h, [&](auto D, auto Pd) {
    constexpr int DIM = decltype(D)::value, P = decltype(Pd)::value;
    if constexpr (tensor_small_dp(DIM, P)) launch_tensor_small_dp<DIM, P>(h, mode, a);
    else fail("no small-element tensor kernel for dimension %d, degree %d", DIM, P);
  });
  if (!commit) launch_general_gather(h, c);
  return true;
}

// One assembly, r += R(u) and with c.grad A (+)= grad_factor K(u); c holds the CALLER's arrays, host or device.
// c.A_base (tangent assemblies only): nullptr = the plain "A += gf K"; otherwise A = A_base + gf K on the rows of the handle's
// nodes.  Both arrays on the device: the row gathers read A_base where they would read A (no extra pass); any other
// residence: A_base is copied into (the staging copy of) A first.
inline void run_domain(mimi_hip_domain_s* h, DomainCall c) {
  MH_HIP(hipSetDevice(h->device));
  if (!c.u || !c.r || (c.grad && !c.A)) fail("null vector argument");
  h->integrated = false;   // the element pieces of an earlier mimi_hip_domain_integrate are overwritten by this call
  Mirror<double> mu = Mirror<double>::in(c.u, h->n_vdofs, h->stage_u, h->stream);
  Mirror<double> mr = Mirror<double>::inout(c.r, h->n_vdofs, h->stage_r, h->stream);
  Mirror<double> mA;
  const double* base = c.A_base;
  c.A_base = nullptr;
  if (c.grad && base && base != c.A) {
    if (is_device_pointer(c.A) && is_device_pointer(base)) {
      mA = Mirror<double>::inout(c.A, h->nnz, h->stage_A, h->stream);
      c.A_base = base;
    } else if (is_device_pointer(c.A)) {
      mA = Mirror<double>::inout(c.A, h->nnz, h->stage_A, h->stream);
      MH_HIP(hipMemcpyAsync(c.A, base, (size_t)h->nnz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
      // host output: its staging copy starts from the base instead of from A's own contents
      h->stage_A.resize(h->nnz);
      MH_HIP(hipMemcpyAsync(h->stage_A.ptr, base, (size_t)h->nnz * sizeof(double), hipMemcpyDefault, h->stream));
      mA.dev = h->stage_A.ptr;
      mA.host = c.A;
      mA.count = h->nnz;
      mA.stage = &h->stage_A;
    }
  } else if (c.grad) {
    mA = Mirror<double>::inout(c.A, h->nnz, h->stage_A, h->stream);
  }
  c.u = mu.dev;
  c.r = mr.dev;
  c.A = mA.dev;
  // (a 3-D degree-2 / 3 patch whose CSR is not the structured pattern is not tensor_usable: the general kernels take it)
  if (tensor_small(h) && c.grad != 2 && launch_tensor_small(h, c)) {
    // (2-D, degree 1: element kernel from the 1-D tables + the general gather)
    h->last_family = 3;
  } else if (tensor_usable(h) && !tensor_small(h) && c.grad != 2) {
    h->last_family = launch_tensor(h, c);
  } else {
    h->last_family = 4;
    launch_general(h, c);
  }
  mr.finish(h->stream);
  if (c.grad) mA.finish(h->stream);
  const bool any_host = mu.host || mr.host || (c.grad && mA.host);
  if (any_host) check_status(h);  // synchronous for host-resident arguments
}

// DomainPostTimeAdvance: the state commit of the handle's kernel family
inline void run_post_time_advance(mimi_hip_domain_s* h, const double* u) {
  MH_HIP(hipSetDevice(h->device));
  h->integrated = false;   // (the state the stored pieces were integrated with is about to change)
  Mirror<double> mu = Mirror<double>::in(u, h->n_vdofs, h->stage_u, h->stream);
  const DomainCall c{mu.dev};
  if (tensor_small(h)) launch_tensor_small(h, c, true);
  else if (h->path == 1) launch_tensor_post(h, c);
  else launch_general_post(h, c);
  if (mu.host) check_status(h);
}

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
  auto kernel = h->dim == 2 ? expand_shape_kernel<2> : expand_shape_kernel<3>;
  launch(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, patch_dev(h, nullptr), h->shape_N.ptr);
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
    constexpr int FK = decltype(K)::value;
    auto kernel = h->dim == 2 ? field_general_kernel<2, FK> : field_general_kernel<3, FK>;
    launch(kernel, dim3((unsigned)h->n_el), dim3(256), lds, h->stream, a, fa);
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
  if (!h->adj_ptr.ptr && !h->field_adj_ptr.ptr) fill_adjacency(h, h->field_adj_ptr, h->field_adj);
  const int64_t* adj_ptr = h->adj_ptr.ptr ? h->adj_ptr.ptr : h->field_adj_ptr.ptr;
  const int32_t* adj = h->adj_ptr.ptr ? h->adj.ptr : h->field_adj.ptr;
  const int64_t total = n_nodes * (ncomp + 1);
  launch(field_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, n_nodes, h->n_dof, ncomp, adj_ptr, adj,
         (const double*)h->field_pieces.ptr, ms.dev, mw.dev);
  ms.finish(h->stream);
  if (weight) mw.finish(h->stream);
  if (mu.host || ms.host || mw.host) check_status(h);
}

// ---- linear forms (kernels_forms.hpp) ----------------------------------------------------------------------------------

// the node -> (element, local node) adjacency: the general row gather's when the handle has it, the field output's otherwise
inline void form_adjacency(mimi_hip_domain_s* h, const int64_t*& adj_ptr, const int32_t*& adj) {
  if (!h->adj_ptr.ptr && !h->field_adj_ptr.ptr) fill_adjacency(h, h->field_adj_ptr, h->field_adj);
  adj_ptr = h->adj_ptr.ptr ? h->adj_ptr.ptr : h->field_adj_ptr.ptr;
  adj = h->adj_ptr.ptr ? h->adj.ptr : h->field_adj.ptr;
}

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
  if (h->longest_row < 0) {
    const std::vector<int64_t> rp = to_host(h->rowptr, (size_t)h->n_vdofs + 1);
    int64_t longest = 0;
    for (int64_t v = 0; v < h->n_vdofs; ++v) longest = std::max(longest, rp[v + 1] - rp[v]);
    h->longest_row = longest;
  }
  if (h->longest_row > GG_MAX_ROW) fail("mass / diffusion form: a CSR row of %lld entries is longer than the row image (%d)", (long long)h->longest_row, GG_MAX_ROW);
  const int64_t* adj_ptr = nullptr;
  const int32_t* adj = nullptr;
  form_adjacency(h, adj_ptr, adj);
  const int64_t n_nodes = h->n_vdofs / h->dim;
  auto kernel = h->dim == 2 ? (kind == FORM_MASS ? form_general_kernel<2, FORM_MASS> : form_general_kernel<2, FORM_DIFFUSION>)
                            : (kind == FORM_MASS ? form_general_kernel<3, FORM_MASS> : form_general_kernel<3, FORM_DIFFUSION>);
  launch(kernel, dim3((unsigned)((n_nodes + GG_WAVES - 1) / GG_WAVES)), dim3(64 * GG_WAVES), 0, h->stream, n_nodes, h->n_dof, h->n_q, h->rowptr,
         adj_ptr, adj, (const int32_t*)h->pair_pos.ptr, (const double*)h->shape_N.ptr, (const double*)h->dN_dX.ptr, (const double*)h->wdet.ptr,
         factor, A);
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
  const int64_t* adj_ptr = nullptr;
  const int32_t* adj = nullptr;
  form_adjacency(h, adj_ptr, adj);
  h->lumped_w.resize((size_t)n_nodes);
  MH_HIP(hipMemsetAsync(h->lumped_w.ptr, 0, (size_t)n_nodes * sizeof(double), h->stream));
  launch(field_gather_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, h->stream, n_nodes, h->n_dof, 0, adj_ptr, adj,
         (const double*)h->field_pieces.ptr, (double*)nullptr, h->lumped_w.ptr);
  auto kernel = h->dim == 2 ? form_body_force_kernel<2> : form_body_force_kernel<3>;
  launch(kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, h->stream, n_nodes, (const double*)h->lumped_w.ptr, b[0], b[1],
         h->dim == 3 ? b[2] : 0.0, mr.dev);
  mr.finish(h->stream);
  if (mr.host) check_status(h);
}

// ---- tangent action (kernels_apply.hpp) ----------------------------------------------------------------------------------

// the kernel family an action runs on, with the codes of last_family: the tensor route for every tensor_usable handle
inline int apply_family_of(const mimi_hip_domain_s* h) {
  if (tensor_small(h)) return 3;
  if (tensor_usable(h)) return h->degree[0] == 3 ? 2 : 1;
  return 4;
}

// the one switch over what a linearisation leaves: the neo-Hookean action recomputes, every other material has the record
inline bool apply_recomputes(const mimi_hip_domain_s* h) { return h->mat.m.kind == MIMI_HIP_MAT_NEOHOOKEAN; }

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
  auto kernel = h->dim == 2 ? apply_general_kernel<2, MODE, FAMILY> : apply_general_kernel<3, MODE, FAMILY>;
  launch(kernel, dim3((unsigned)h->n_el), dim3(256), lds, stream, a, aa);
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
  if (!h->adj_ptr.ptr && !h->field_adj_ptr.ptr) built = true;
  const int64_t* adj_ptr = nullptr;
  const int32_t* adj = nullptr;
  form_adjacency(h, adj_ptr, adj);
  const size_t need = (size_t)h->n_el * h->n_dof * h->dim;
  if (h->scratch_r.count < need) {
    MH_HIP(hipStreamSynchronize(h->stream));   // (nothing in flight reads the pieces that are released)
    h->scratch_r.resize(need);
  }
  return built;
}

inline void apply_check(const mimi_hip_domain_s* h, double stiffness) {
  if (stiffness != 0.0 && !h->linearized)
    fail("mimi_hip_domain_apply_tangent with a stiffness coefficient before any mimi_hip_domain_linearize on this handle");
}

// y += density M x + stiffness K(u_lin) x + viscosity C x on `stream`; x, y on the device; apply_prepare has run
inline void launch_apply(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, const double* x, double* y,
                         hipStream_t stream) {
  h->integrated = false;   // the element pieces of an earlier mimi_hip_domain_integrate are overwritten
  ApplyArgs aa{};
  aa.density = density;
  aa.stiffness = stiffness;
  aa.viscosity = viscosity;
  aa.x = x;
  aa.u_lin = h->lin_u.ptr;
  aa.rec = h->lin_rec.ptr;
  aa.pieces = h->scratch_r.ptr;
  aa.N = h->shape_N.ptr;
  aa.n_pts = h->n_pts;
  aa.n_el = h->n_el;
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
  const int64_t* adj_ptr = h->adj_ptr.ptr ? h->adj_ptr.ptr : h->field_adj_ptr.ptr;
  const int32_t* adj = h->adj_ptr.ptr ? h->adj.ptr : h->field_adj.ptr;
  const int64_t total = h->n_vdofs;
  launch(apply_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, h->n_vdofs / h->dim, h->n_dof, h->dim, adj_ptr, adj,
         (const double*)h->scratch_r.ptr, y);
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
    ApplyArgs aa{};
    aa.u_lin = mu.dev;
    aa.rec = h->lin_rec.ptr;
    aa.n_pts = h->n_pts;
    aa.n_el = h->n_el;
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
