// Host-side state of one domain integrator handle (= one integrators::NonlinearSolid,
// integrators/nonlinear_solid.hpp:15-50, bound to one HIP device and stream).
#pragma once

#include "bspline_host.hpp"
#include "common.hpp"

struct mimi_hip_domain_s : mimi_hip::StreamHandle {
  int dim = 0, n_el = 0, n_dof = 0, n_q = 0;
  int64_t n_nodes = 0, n_vdofs = 0, nnz = 0, n_pts = 0;
  int path = 0;  // 0 general tables, 1 tensor-product (sum factorisation)

  mimi_hip::MaterialDev mat{};
  double dt = 0.0, first_effective_dt = 0.0, second_effective_dt = 0.0;
  int tangent_mode = MIMI_HIP_TANGENT_ANALYTIC;

  // general path tables
  mimi_hip::DeviceBuffer<int32_t> dofs;      // [n_el][n_dof]
  mimi_hip::DeviceBuffer<double> dN_dX;      // [n_el][n_q][dim][n_dof]
  mimi_hip::DeviceBuffer<double> wdet;       // [n_el][n_q]
  mimi_hip::DeviceBuffer<int32_t> pair_pos;  // [n_el][n_dof][n_dof]
  mimi_hip::DeviceBuffer<int64_t> rowptr_own;
  mimi_hip::DeviceBuffer<int64_t> adj_ptr;   // node -> incident (element << 6 | local node) list, built at first use (node_adjacency):
  mimi_hip::DeviceBuffer<int32_t> adj;       // the general row gather, the form kernels, the node gather of fields and actions
  // the general path scatters with atomics instead of store + row gather: MIMI_HIP_GENERAL_NO_TWO_PHASE as read at create,
  // or what ensure_general_two_phase found (a CSR row longer than the gather's image, no room for the element blocks)
  bool general_two_phase_failed = false;
  const int64_t* rowptr = nullptr;           // device

  // tensor path tables
  int degree[3] = {0, 0, 0}, nq1[3] = {1, 1, 1}, n_ctrl[3] = {1, 1, 1};
  int el_begin[3] = {0, 0, 0}, el_end[3] = {1, 1, 1}, el_total[3] = {1, 1, 1};
  mimi_hip::DeviceBuffer<double> tab1d;      // per direction B then D: [n_spans][p+1][nq]
  mimi_hip::DeviceBuffer<int32_t> first1d;   // per direction [n_spans]
  size_t tab_off_B[3] = {0, 0, 0}, tab_off_D[3] = {0, 0, 0}, tab_off_W[3] = {0, 0, 0}, first_off[3] = {0, 0, 0};
  mimi_hip::DeviceBuffer<double> geo;        // [n_el][dim*dim+1][n_q]: dxi/dX (d,J) then w*det
  mimi_hip::DeviceBuffer<int64_t> node_ids;  // lexicographic -> global, empty = identity
  bool structured_csr = false;               // CSR positions computable arithmetically
  bool structured_perm = false;              // permuted numbering whose CSR rows are the permuted structured pattern
  mimi_hip::DeviceBuffer<unsigned char> nbr_pos;  // [n_nodes][125] rank of each window neighbour inside the row (structured_perm, p <= 2)
  mimi_hip::DeviceBuffer<uint16_t> nbr_pos16;     // [n_nodes][343] the same for degree 3
  bool first_is_identity = false;            // span e's first basis function is e (no repeated interior knots)
  mimi_hip::DeviceBuffer<double> scratch_k, scratch_r, scratch_pt, scratch_tail;  // two-phase tangent path
  mimi_hip::DeviceBuffer<double> mat_rec;    // general path, other materials' tangent assemblies: [n_el][n_q][DIM^2 + DIM^4] (kernels_general.hpp)
  mimi_hip::DeviceBuffer<double> t3_t2pack;  // degree-3 contraction: direction-2 table values per (span, lane), [n_spans][64][8] (tensor_p3.hip)

  // J2 state, SoA over points
  mimi_hip::DeviceBuffer<double> eqps, temperature, plastic_strain, state2;

  // status word raised by kernels (ScalarSolve failures, bad pattern)
  int* status_dev = nullptr;
  int* status_host = nullptr;  // pinned
  // mimi_hip_domain_set_phase_timing: events around phase 1 (integration kernels) and phase 2 (gather) of the last
  // two-phase assembly, on the launch stream
  bool phase_timing = false;
  hipEvent_t phase_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // [3]: end of the material pre-pass, when there is one
  bool phase_has_prepass = false;

  // mimi_hip_domain_integrate has stored the element pieces mimi_hip_domain_gather reads (what one call runs, and over
  // which nodes, is the call's own: DomainCall, domain_call.hpp)
  bool integrated = false;
  // kernel family of the last assembly / state commit on this handle (mimi_hip_domain_info(h, 7)): 0 none yet,
  // 1 two-phase tensor degree 2, 2 two-phase tensor degree 3, 3 small-element tensor kernel, 4 general kernels
  int last_family = MIMI_HIP_FAMILY_NONE;
  // scatter route of the last assembly (mimi_hip_domain_info(h, 13)): 0 none yet or a two-phase tensor family, 1 store +
  // general row gather, 2 atomics
  int last_general_route = MIMI_HIP_GENERAL_ROUTE_NONE;
  // symmetric-half degree-2 kernel (wgsym_geometry.hpp): MIMI_HIP_WGSYM_MIN_WGS as read at create (0: unset, the shipped
  // WGSYM_MIN_WGS), and the geometry of the handle's last launch of it (mimi_hip_domain_info(h, 11) and (h, 12); 0: none yet)
  int wgsym_min_wgs = 0;
  int last_seg_len = 0, last_cols_per_wg = 0;

  // staging for host-resident u / r / A
  mimi_hip::DeviceBuffer<double> stage_u, stage_r, stage_A;

  // field output (kernels_fields.hpp): shape values of the general route [n_el][n_q][n_dof], element pieces of the nodal
  // form [n_el][n_dof][ncomp + 1], staging for host-resident outputs
  mimi_hip::DeviceBuffer<double> shape_N, field_pieces, stage_f, stage_w;

  // linear forms (kernels_forms.hpp): the lumped weight of the body force [n_nodes]
  mimi_hip::DeviceBuffer<double> lumped_w;
  // the longest CSR row, once longest_row(h) has scanned it (the row image of the general gathers is GG_MAX_ROW entries)
  int64_t longest_row = -1;

  // tangent action (kernels_apply.hpp): what mimi_hip_domain_linearize left -- the device copy of u (neo-Hookean) or the
  // record w det dP/dF [dim^4][n_pts] (every other material) -- the event recorded behind it (a solver on another stream
  // waits on it once per solve), the kernel family of the last action (mimi_hip_domain_info(h, 9)), staging for a host x
  mimi_hip::DeviceBuffer<double> lin_u, lin_rec, stage_x;
  bool linearized = false;
  hipEvent_t lin_event = nullptr;
  int apply_family = MIMI_HIP_FAMILY_NONE;

  ~mimi_hip_domain_s();
};
