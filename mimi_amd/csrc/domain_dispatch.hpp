// Dispatch of one call of the domain integrator: what every route asks of the handle (the general tables, the node adjacency,
// the longest CSR row, the switch over dimension and degree), the general kernels and their row gather, the small-element
// tensor kernels, the choice between them and the two-phase tensor kernels (tensor_dispatch.hpp).  The field output, the
// linear forms and the matrix-free tangent action are domain_dispatch_nodal.hpp, on top of this header.
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

// calls f(integral_constant DIM)
template<class F>
void by_dim(const mimi_hip_domain_s* h, F&& f) {
  if (h->dim == 2) f(std::integral_constant<int, 2>{}); else f(std::integral_constant<int, 3>{});
}

// calls f(integral_constant DIM, integral_constant P) for a tensor_usable handle (tensor_supported: one degree, 1..3)
template<class F>
void by_dim_degree(const mimi_hip_domain_s* h, F&& f) {
  by_dim(h, [&](auto D) {
    switch (h->degree[0]) {
    case 1: f(D, std::integral_constant<int, 1>{}); break;
    case 2: f(D, std::integral_constant<int, 2>{}); break;
    default: f(D, std::integral_constant<int, 3>{}); break;
    }
  });
}

// the handle's node -> incident (element << 6 | local node) lists, built at first use: what the general row gather, the form
// kernels and node_gather_kernel walk
struct NodeAdjacency {
  const int64_t* ptr;
  const int32_t* adj;
};
inline NodeAdjacency node_adjacency(mimi_hip_domain_s* h) {
  if (h->adj_ptr.ptr) return {h->adj_ptr.ptr, h->adj.ptr};
  const size_t n = (size_t)h->n_el * h->n_dof;
  const std::vector<int32_t> dofs = to_host(h->dofs.ptr, n);
  const int64_t n_nodes = h->n_vdofs / h->dim;
  std::vector<int64_t> ptr(n_nodes + 1, 0);
  for (size_t k = 0; k < n; ++k) ++ptr[dofs[k] + 1];
  for (int64_t v = 0; v < n_nodes; ++v) ptr[v + 1] += ptr[v];
  std::vector<int32_t> adj(n);
  std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
  for (size_t k = 0; k < n; ++k) adj[fill[dofs[k]]++] = (int32_t)(((k / h->n_dof) << 6) | (k % h->n_dof));
  h->adj_ptr.assign(ptr.data(), ptr.size(), h->stream);
  h->adj.assign(adj.data(), adj.size(), h->stream);
  return {h->adj_ptr.ptr, h->adj.ptr};
}

// the longest CSR row, scanned once (the row gathers keep one row in LDS, GG_MAX_ROW entries)
inline int64_t longest_row(mimi_hip_domain_s* h) {
  if (h->longest_row < 0) {
    const std::vector<int64_t> rp = to_host(h->rowptr, (size_t)h->n_vdofs + 1);
    h->longest_row = 0;
    for (int64_t v = 0; v < h->n_vdofs; ++v) h->longest_row = std::max(h->longest_row, rp[v + 1] - rp[v]);
  }
  return h->longest_row;
}

// two-phase general path: element blocks / residual vectors densely into scratch_k / scratch_r, then
// general_gather_kernel.  Needs n_el * n_tdof^2 doubles (77 GB at 128 x 128 x 16 p = 3) and the node -> element adjacency;
// falls back to the atomics when the scratch does not fit (MIMI_HIP_GENERAL_NO_TWO_PHASE=1 at create forces that: the
// handle's flag starts from it).  What it decides depends on the CSR rows, the element size and the memory alone, never on
// what ran on the handle before
inline bool ensure_general_two_phase(mimi_hip_domain_s* h, bool with_k) {
  if (h->general_two_phase_failed) return false;
  const size_t n_tdof = (size_t)h->n_dof * h->dim;
  // what rules the path out is checked BEFORE anything is allocated.  The gather kernel keeps one CSR row in LDS: rows
  // longer than its image -> atomics.  n_dof > 64 is a guard, not a route: both creators refuse such a handle (the
  // adjacency packs the local node into 6 bits)
  if (longest_row(h) > GG_MAX_ROW || h->n_dof > 64) {
    h->general_two_phase_failed = true;
    return false;
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
  node_adjacency(h);
  return true;
}

// the row gather of the general path: r += sums of scratch_r, and with a tangent A = A_old + grad_factor * sums of scratch_k
// (A_old: the call's base array, or A itself)
inline void launch_general_gather(mimi_hip_domain_s* h, const DomainCall& c) {
  const int64_t n_rows = h->n_vdofs;
  by_dim(h, [&](auto D) {
    constexpr int DIM = decltype(D)::value;
    launch(c.grad ? general_gather_kernel<DIM, 1> : general_gather_kernel<DIM, 0>, dim3((unsigned)((n_rows + GG_WAVES - 1) / GG_WAVES)),
           dim3(64 * GG_WAVES), 0, h->stream, n_rows, h->n_dof, h->rowptr, h->adj_ptr.ptr, h->adj.ptr, h->pair_pos.ptr, h->scratch_k.ptr,
           h->scratch_r.ptr, c.grad_factor, c.A_old(), c.A, c.r);
  });
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
  h->last_general_route = two_phase ? MIMI_HIP_GENERAL_ROUTE_GATHER : MIMI_HIP_GENERAL_ROUTE_ATOMICS;
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
  by_dim(h, [&](auto D) { launch_general_dim<decltype(D)::value>(h, c); });
}

// DomainPostTimeAdvance on the general tables
inline void launch_general_post(mimi_hip_domain_s* h, const DomainCall& c) {
  ensure_general_tables(h);
  const GeneralArgs a = general_args(h, c);
  const size_t lds = (size_t)h->n_dof * h->dim * sizeof(double);
  by_material_family(h->mat.m.kind, [&](auto K) {
    constexpr int REC = decltype(K)::value != 0 ? 1 : 0;
    by_dim(h, [&](auto D) { launch(post_time_advance_general_kernel<decltype(D)::value, REC>, dim3(h->n_el), dim3(256), lds, h->stream, a); });
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
    h->last_general_route = MIMI_HIP_GENERAL_ROUTE_GATHER;
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
    h->last_family = MIMI_HIP_FAMILY_TENSOR_SMALL;
  } else if (tensor_usable(h) && !tensor_small(h) && c.grad != 2) {
    h->last_family = launch_tensor(h, c);
    h->last_general_route = MIMI_HIP_GENERAL_ROUTE_NONE;
  } else {
    h->last_family = MIMI_HIP_FAMILY_GENERAL;
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

}  // namespace mimi_hip
