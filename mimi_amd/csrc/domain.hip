// C ABI of the domain integrator (include/mimi_hip.h): handle life cycle, table upload / generation, assemblies.  Handle
// construction is domain_create.hpp, the kernel dispatch domain_dispatch.hpp and domain_dispatch_nodal.hpp.  Reference counterparts:
//   NonlinearSolid::Prepare                      integrators/nonlinear_solid.cpp:31-46
//   NonlinearSolid::AddDomainResidual            integrators/nonlinear_solid.cpp:151-160
//   NonlinearSolid::AddDomainResidualAndGrad     integrators/nonlinear_solid.cpp:162-177
//   NonlinearSolid::DomainPostTimeAdvance        integrators/nonlinear_solid.cpp:179-199
#include "apply_seam.hpp"
#include "domain_dispatch_nodal.hpp"

#include <memory>

namespace mimi_hip {

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }

// the two-step form of a tangent assembly: phase 1 of the whole handle, then phase 2 over parts of its nodes
static void require_two_phase(mimi_hip_domain_s* h) {
  const bool ok = h->dim == 3 && tensor_usable(h) && !tensor_small(h) && h->tangent_mode == MIMI_HIP_TANGENT_ANALYTIC;
  if (!ok) fail("integrate / gather: only on the two-phase tensor paths (3-D, degree 2 or 3, structured CSR, analytic tangent)");
}

// the grad of a tangent assembly's DomainCall in the handle's tangent mode
static int tangent_grad(const mimi_hip_domain_s* h) { return h->tangent_mode == MIMI_HIP_TANGENT_REFERENCE_FD ? 2 : 1; }

// ---- the operator seam of the Krylov solvers (apply_seam.hpp) ----------------------------------------------------------------
int64_t operator_size(const mimi_hip_domain_s* h) { return h->n_vdofs; }
int operator_device(const mimi_hip_domain_s* h) { return h->device; }

void operator_begin_solve(mimi_hip_domain_s* h, double density, double stiffness, hipStream_t solver_stream) {
  apply_check(h, stiffness);
  // tables, shape values and the adjacency on the handle's own stream, finished before the solver's stream reads them
  if (apply_prepare(h, density)) MH_HIP(hipStreamSynchronize(h->stream));
  if (h->lin_event && stiffness != 0.0) MH_HIP(hipStreamWaitEvent(solver_stream, h->lin_event, 0));
}

void operator_add_action(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, const double* x, double* y,
                         hipStream_t solver_stream) {
  launch_apply(h, density, stiffness, viscosity, x, y, solver_stream);
}

int operator_dim(const mimi_hip_domain_s* h) { return h->dim; }

void operator_begin_diagonal(mimi_hip_domain_s* h, double density, double stiffness, int block, hipStream_t solver_stream) {
  apply_check(h, stiffness, "mimi_hip_domain_tangent_diagonal");
  if (diagonal_prepare(h, density, block)) MH_HIP(hipStreamSynchronize(h->stream));
  if (h->lin_event && stiffness != 0.0) MH_HIP(hipStreamWaitEvent(solver_stream, h->lin_event, 0));
}

void operator_add_diagonal(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, int block, double* d,
                           hipStream_t solver_stream) {
  launch_diagonal(h, density, stiffness, viscosity, block, d, solver_stream);
}

}  // namespace mimi_hip

using namespace mimi_hip;

mimi_hip_domain_s::~mimi_hip_domain_s() {
  for (auto& ev : phase_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (lin_event) (void)hipEventDestroy(lin_event);
  if (status_dev) (void)hipFree(status_dev);
  if (status_host) (void)hipHostFree(status_host);
}

extern "C" {

const char* mimi_hip_last_error(void) { return g_last_error.c_str(); }
int mimi_hip_abi_version(void) { return MIMI_HIP_ABI_VERSION; }

int mimi_hip_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}

void mimi_hip_material_set_young_poisson(mimi_hip_material* mat, double young, double poisson) {
  // MaterialBase::SetYoungPoisson (materials.cpp:7-14)
  mat->lambda = young * poisson / ((1 + poisson) * (1 - 2 * poisson));
  mat->mu = young / (2.0 * (1.0 + poisson));
  mat->G = mat->mu;
  mat->K = young / (3.0 * (1.0 - (2.0 * poisson)));
}

int mimi_hip_domain_create(const mimi_hip_domain_tables* t, const mimi_hip_material* material, int device,
                           mimi_hip_domain_t* out) {
  return guarded([&] {
    if (!t || !material || !out) fail("null argument");
    if (t->dim != 2 && t->dim != 3) fail("Unsupported Dim: %d", t->dim);
    if (t->n_dof < 1 || t->n_dof > 64) fail("n_dof %d out of range [1,64]", t->n_dof);
    if (t->n_quad < 1 || t->n_quad > 125) fail("n_quad %d out of range [1,125]", t->n_quad);
    if (t->n_elements < 1) fail("no elements");
    auto h = std::make_unique<mimi_hip_domain_s>();
    init_common(h.get(), device, material);
    h->dim = t->dim;
    h->n_el = t->n_elements;
    h->n_dof = t->n_dof;
    h->n_q = t->n_quad;
    h->n_nodes = t->n_nodes;
    h->n_vdofs = t->n_nodes * t->dim;
    h->path = 0;
    const size_t n_tdof = (size_t)t->n_dof * t->dim;
    h->dofs.assign(t->dofs, (size_t)t->n_elements * t->n_dof, h->stream);
    h->dN_dX.assign(t->dN_dX, (size_t)t->n_elements * t->n_quad * n_tdof, h->stream);
    h->wdet.assign(t->weight_det, (size_t)t->n_elements * t->n_quad, h->stream);
    setup_csr(h.get(), t->csr_rowptr, t->csr_col, true);
    init_state(h.get());
    *out = h.release();
  });
}

int mimi_hip_domain_create_bspline(const mimi_hip_bspline_patch* p, const mimi_hip_material* material, int device,
                                   mimi_hip_domain_t* out) {
  return guarded([&] {
    if (!p || !material || !out) fail("null argument");
    if (p->dim != 2 && p->dim != 3) fail("Unsupported Dim: %d", p->dim);
    auto h = std::make_unique<mimi_hip_domain_s>();
    h->wgsym_min_wgs = env_wgsym_min_wgs();
    init_common(h.get(), device, material);
    h->dim = p->dim;
    Tables1D t1[3];
    make_patch_tables(h.get(), p, t1);
    upload_tables_1d(h.get(), t1);
    DeviceBuffer<double> ctrl;
    ctrl.assign(p->control_points, (size_t)h->n_nodes * h->dim, h->stream);
    if (p->node_ids) h->node_ids.assign(p->node_ids, (size_t)h->n_nodes, h->stream);
    const PatchDev P = patch_dev(h.get(), ctrl.ptr);
    compute_geometry(h.get(), P);
    const bool force_general = env_force_general();
    const bool tensor_ok = tensor_supported(h->dim, h->degree, h->nq1[0]);
    h->path = (tensor_ok && !force_general) ? 1 : 0;
    build_connectivity(h.get(), P, force_general || !tensor_ok || env_keep_general());
    setup_csr(h.get(), p->csr_rowptr, p->csr_col, false);
    recognise_pattern(h.get(), p, t1);
    // degree 3 has the two-phase tensor kernels only: anything else about the handle (numbering, pattern) -> general path
    if (h->path == 1 && !tensor_usable(h.get())) h->path = 0;
    // pair positions now unless this handle will run the two-phase kernels (then on demand, ensure_pair_pos)
    if (!tensor_usable(h.get()) || tensor_small(h.get())) build_pair_pos(h.get(), p->csr_col);
    init_state(h.get());
    MH_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
  });
}

int mimi_hip_domain_destroy(mimi_hip_domain_t h) { return handle_destroy(h); }

int mimi_hip_domain_set_dt(mimi_hip_domain_t h, double dt, double first_effective_dt, double second_effective_dt) {
  return guarded([&] {
    if (!h) fail("null handle");
    h->dt = dt;
    h->first_effective_dt = first_effective_dt;
    h->second_effective_dt = second_effective_dt;
  });
}

int mimi_hip_domain_set_tangent_mode(mimi_hip_domain_t h, int mode) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (mode != MIMI_HIP_TANGENT_ANALYTIC && mode != MIMI_HIP_TANGENT_REFERENCE_FD) fail("bad tangent mode %d", mode);
    h->tangent_mode = mode;
  });
}

int mimi_hip_domain_set_stream(mimi_hip_domain_t h, void* stream) { return handle_set_stream(h, stream); }

int mimi_hip_domain_integrate(mimi_hip_domain_t h, const double* u) {
  return guarded([&] {
    if (!h || !u) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    require_two_phase(h);
    if (!is_device_pointer(u)) fail("integrate / gather: device-resident arguments only");
    launch_tensor(h, DomainCall{u, nullptr, nullptr, nullptr, 0.0, 1, DomainCall::INTEGRATE_ONLY});
    h->integrated = true;
  });
}

int mimi_hip_domain_gather(mimi_hip_domain_t h, double grad_factor, double* r, double* A_values, const int32_t node_begin[3],
                           const int32_t node_end[3]) {
  return guarded([&] {
    if (!h || !r || !A_values || !node_begin || !node_end) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    require_two_phase(h);
    if (!h->integrated) fail("gather: mimi_hip_domain_integrate has not run on this handle");
    if (!is_device_pointer(r) || !is_device_pointer(A_values)) fail("integrate / gather: device-resident arguments only");
    DomainCall c{nullptr, r, A_values, nullptr, grad_factor, 1, DomainCall::GATHER_ONLY};
    for (int d = 0; d < 3; ++d) {
      const int lo = h->el_begin[d], hi = h->el_end[d] + h->degree[d];     // nodes the handle's elements touch
      if (node_begin[d] < lo || node_end[d] > hi || node_begin[d] >= node_end[d])
        fail("gather: node range [%d,%d) in direction %d is not inside the handle's nodes [%d,%d)", node_begin[d], node_end[d], d, lo, hi);
      c.gather_begin[d] = node_begin[d];
      c.gather_end[d] = node_end[d];
    }
    launch_tensor(h, c);
  });
}

int mimi_hip_domain_synchronize(mimi_hip_domain_t h) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    check_status(h);
  });
}

int mimi_hip_domain_add_residual(mimi_hip_domain_t h, const double* u, double* r) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_domain(h, DomainCall{u, r});
  });
}

int mimi_hip_domain_add_residual_and_grad(mimi_hip_domain_t h, const double* u, double grad_factor, double* r,
                                          double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_domain(h, DomainCall{u, r, A_values, nullptr, grad_factor, tangent_grad(h)});
  });
}

int mimi_hip_domain_add_residual_and_grad_from(mimi_hip_domain_t h, const double* u, double grad_factor, double* r,
                                               const double* A_base, double* A_out) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!A_base) fail("null vector argument");
    // "A_out = A_base + gf K" does not compose over element boxes the way "+=" does (a second box would overwrite the rows it
    // shares with the first, or -- on the routes that copy the base first -- the whole array): whole-patch handles only
    // (tables-created handles, el_total 1, are whole by construction)
    if (A_base != A_out)
      for (int d = 0; d < h->dim; ++d)
        if (h->el_begin[d] != 0 || h->el_end[d] != h->el_total[d])
          fail("mimi_hip_domain_add_residual_and_grad_from needs a whole-patch handle (this one holds elements [%d,%d) of %d in "
               "direction %d): assemble element boxes with mimi_hip_domain_add_residual_and_grad into a copy of the base",
               h->el_begin[d], h->el_end[d], h->el_total[d], d);
    run_domain(h, DomainCall{u, r, A_out, A_base, grad_factor, tangent_grad(h)});
  });
}

int mimi_hip_domain_post_time_advance(mimi_hip_domain_t h, const double* u) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!material_has_state(h->mat.m.kind)) return;  // has_states_ == false (nonlinear_solid.cpp:182-183)
    run_post_time_advance(h, u);
  });
}

int mimi_hip_domain_get_state(mimi_hip_domain_t h, int what, double* out, int64_t capacity) {
  return guarded([&] {
    if (!h || !out) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    if (!material_has_state(h->mat.m.kind)) fail("material has no state");
    const int dd = h->dim * h->dim;
    const bool matrix = what == MIMI_HIP_STATE_MATRIX_1 || what == MIMI_HIP_STATE_MATRIX_2;
    const int64_t need = matrix ? h->n_pts * dd : h->n_pts;
    if (capacity < need) fail("state buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
    MH_HIP(hipStreamSynchronize(h->stream));
    if (what == MIMI_HIP_STATE_EQPS) {
      MH_HIP(hipMemcpy(out, h->eqps.ptr, need * sizeof(double), hipMemcpyDeviceToHost));
    } else if (what == MIMI_HIP_STATE_TEMPERATURE) {
      MH_HIP(hipMemcpy(out, h->temperature.ptr, need * sizeof(double), hipMemcpyDeviceToHost));
    } else if (matrix) {
      if (what == MIMI_HIP_STATE_MATRIX_2 && !h->state2.ptr) fail("material has no second state matrix");
      std::vector<double> soa(need);
      MH_HIP(hipMemcpy(soa.data(), what == MIMI_HIP_STATE_MATRIX_1 ? h->plastic_strain.ptr : h->state2.ptr, need * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t pt = 0; pt < h->n_pts; ++pt)
        for (int c = 0; c < dd; ++c) out[pt * dd + c] = soa[(int64_t)c * h->n_pts + pt];
    } else {
      fail("unknown state id %d", what);
    }
  });
}

int mimi_hip_field_components(int field, int dim) { return field_components(field, dim); }

int mimi_hip_domain_point_field(mimi_hip_domain_t h, const double* u, int field, double* out, int64_t capacity) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_point_field(h, u, field, out, capacity);
  });
}

int mimi_hip_domain_nodal_field(mimi_hip_domain_t h, const double* u, int field, double* sum, double* weight) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_nodal_field(h, u, field, sum, weight);
  });
}

int mimi_hip_domain_set_shape_values(mimi_hip_domain_t h, const double* N) {
  return guarded([&] {
    if (!h || !N) fail("null argument");
    if (h->geo.ptr) fail("mimi_hip_domain_set_shape_values: flat-table handles only (a patch handle has its own 1-D tables)");
    MH_HIP(hipSetDevice(h->device));
    h->shape_N.assign(N, (size_t)h->n_el * h->n_q * h->n_dof, h->stream);
  });
}

int mimi_hip_domain_add_mass(mimi_hip_domain_t h, double density, double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_form(h, FORM_MASS, density, A_values);
  });
}

int mimi_hip_domain_add_diffusion(mimi_hip_domain_t h, double viscosity, double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_form(h, FORM_DIFFUSION, viscosity, A_values);
  });
}

int mimi_hip_domain_linearize(mimi_hip_domain_t h, const double* u) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_linearize(h, u);
  });
}

int mimi_hip_domain_apply_tangent(mimi_hip_domain_t h, double density, double stiffness, double viscosity, const double* x,
                                  double* y) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_apply_tangent(h, density, stiffness, viscosity, x, y);
  });
}

int mimi_hip_domain_tangent_diagonal(mimi_hip_domain_t h, double density, double stiffness, double viscosity, int32_t block, double* d) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_tangent_diagonal(h, density, stiffness, viscosity, block, d);
  });
}

int mimi_hip_domain_add_body_force(mimi_hip_domain_t h, const double* b, double* r) {
  return guarded([&] {
    if (!h) fail("null handle");
    run_body_force(h, b, r);
  });
}

int mimi_hip_domain_set_phase_timing(mimi_hip_domain_t h, int on) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    if (on)
      for (auto& ev : h->phase_ev)
        if (!ev) MH_HIP(hipEventCreate(&ev));
    h->phase_timing = on != 0;
  });
}

int mimi_hip_domain_phase_ms(mimi_hip_domain_t h, double* phase1_ms, double* phase2_ms) {
  return guarded([&] {
    if (!h || !phase1_ms || !phase2_ms) fail("null argument");
    if (!h->phase_timing) fail("phase timing is off (mimi_hip_domain_set_phase_timing)");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipEventSynchronize(h->phase_ev[2]));
    float a = 0.f, b = 0.f;
    MH_HIP(hipEventElapsedTime(&a, h->phase_ev[0], h->phase_ev[1]));
    MH_HIP(hipEventElapsedTime(&b, h->phase_ev[1], h->phase_ev[2]));
    *phase1_ms = a;
    *phase2_ms = b;
  });
}

int mimi_hip_domain_phase_ms_detail(mimi_hip_domain_t h, double* prepass_ms, double* integration_ms, double* gather_ms) {
  return guarded([&] {
    if (!h || !prepass_ms || !integration_ms || !gather_ms) fail("null argument");
    if (!h->phase_timing) fail("phase timing is off (mimi_hip_domain_set_phase_timing)");
    MH_HIP(hipSetDevice(h->device));
    MH_HIP(hipEventSynchronize(h->phase_ev[2]));
    float a = 0.f, b = 0.f, c = 0.f;
    if (h->phase_has_prepass) {
      MH_HIP(hipEventElapsedTime(&a, h->phase_ev[0], h->phase_ev[3]));
      MH_HIP(hipEventElapsedTime(&b, h->phase_ev[3], h->phase_ev[1]));
    } else {
      MH_HIP(hipEventElapsedTime(&b, h->phase_ev[0], h->phase_ev[1]));
    }
    MH_HIP(hipEventElapsedTime(&c, h->phase_ev[1], h->phase_ev[2]));
    *prepass_ms = a;
    *integration_ms = b;
    *gather_ms = c;
  });
}

int mimi_hip_domain_reset_state(mimi_hip_domain_t h) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    init_state(h);
  });
}

int64_t mimi_hip_domain_info(mimi_hip_domain_t h, int what) {
  if (!h) return -1;
  switch (what) {
  case MIMI_HIP_DOMAIN_INFO_N_ELEMENTS: return h->n_el;
  case MIMI_HIP_DOMAIN_INFO_N_QUAD: return h->n_q;
  case MIMI_HIP_DOMAIN_INFO_N_DOF: return h->n_dof;
  case MIMI_HIP_DOMAIN_INFO_NNZ: return h->nnz;
  case MIMI_HIP_DOMAIN_INFO_N_VDOFS: return h->n_vdofs;
  case MIMI_HIP_DOMAIN_INFO_PATH: return h->path;
  case MIMI_HIP_DOMAIN_INFO_CSR_KIND: return h->structured_csr ? 1 : (h->structured_perm ? 2 : 0);
  case MIMI_HIP_DOMAIN_INFO_LAST_FAMILY: return h->last_family;
  case MIMI_HIP_DOMAIN_INFO_HAS_GRADIENT_TABLES: return h->dN_dX.ptr ? 1 : 0;
  case MIMI_HIP_DOMAIN_INFO_APPLY_FAMILY: return h->apply_family;
  case MIMI_HIP_DOMAIN_INFO_LINEARIZATION_BYTES:
    return (h->linearized && h->lin_rec.ptr) ? h->n_pts * (int64_t)(h->dim * h->dim * h->dim * h->dim) * (int64_t)sizeof(double) : 0;
  case MIMI_HIP_DOMAIN_INFO_SEGMENT_LENGTH: return h->last_seg_len;
  case MIMI_HIP_DOMAIN_INFO_UNITS_PER_WORKGROUP: return h->last_cols_per_wg;
  case MIMI_HIP_DOMAIN_INFO_GENERAL_ROUTE: return h->last_general_route;
  default: return -1;
  }
}


int mimi_hip_bspline_sparsity(int32_t dim, const int32_t n_nodes_dir[3], const int32_t degree[3], int device,
                              int64_t* rowptr, int32_t* col, int64_t* nnz_out) {
  return bspline_sparsity(dim, n_nodes_dir, degree, nullptr, nullptr, device, rowptr, col, nnz_out);
}

int mimi_hip_bspline_sparsity_rows(int32_t dim, const int32_t n_nodes_dir[3], const int32_t degree[3],
                                   const int32_t node_begin[3], const int32_t node_end[3], int device, int64_t* rowptr,
                                   int32_t* col, int64_t* nnz_out) {
  if (!node_begin || !node_end) return guarded([&] { fail("node_begin / node_end must be given"); });
  return bspline_sparsity(dim, n_nodes_dir, degree, node_begin, node_end, device, rowptr, col, nnz_out);
}

}  // extern "C"
