/* mimi_hip.h -- C ABI of libmimi_hip.so: MI355X (gfx950) element integration and
 * assembly for mimi's NURBS nonlinear solids.
 *
 * This is the drop-in boundary.  Each entry point replaces one virtual of the
 * reference's `mimi::integrators::NonlinearBase` (or the setup that feeds it); the
 * reference interface it stands in for is cited as path:line under
 * /root/reference/src/mimi/.  INTEGRATION.md shows the C++ subclass a mimi maintainer
 * would add to bind these.
 *
 * Conventions
 *  - plain C, no torch / HIP types in any signature.
 *  - every `const double*` / `double*` / index pointer argument may be a HOST or a
 *    DEVICE pointer; the library detects which (hipPointerGetAttributes).  Host
 *    buffers are staged through device scratch and the call is synchronous; device
 *    buffers are used in place and the call only enqueues work on the handle's
 *    stream (mimi_hip_*_set_stream / mimi_hip_*_synchronize).  ORDERING: the kernels read and write those buffers
 *    in stream order on the handle's stream only.  Work the caller has enqueued on them elsewhere (a zero fill of
 *    r / A, a copy into u) must be ordered before the call, and reads of the results behind it: give the handle the
 *    stream that work runs on (set_stream), or synchronise.  Several handles adding into one A need one stream.
 *  - u, r: fp64[n_vdofs], byVDIM ordering u[node*dim + c]   (py_nonlinear_solid.cpp:63,74)
 *  - A_values: fp64[nnz] of a CSR matrix with sorted columns whose structure
 *    (rowptr, col) was given at create time and never changes (precomputed.cpp:151-174,
 *    nonlinear_base.hpp:130).  Outputs are ACCUMULATED (+=), never overwritten.
 *  - return value: 0 on success, non-zero on error; mimi_hip_last_error() then holds
 *    the message the reference would have thrown as std::runtime_error
 *    (utils/print.hpp:47-56).  Not re-entrant per handle (like the reference:
 *    mutable work data, nonlinear_solid.hpp:42).
 *  - KERNEL-RAISED ERRORS (a return map whose ScalarSolve finds its root not bracketed or does not converge, where the
 *    reference throws from inside the evaluation) are raised on the device into a status word of the handle.  With a HOST
 *    argument the call is synchronous and reports the error itself.  With DEVICE arguments only the call has merely
 *    enqueued: it returns 0, and the error is reported by the next mimi_hip_domain_synchronize on the handle, or by the
 *    next call on it that waits (any call with a host argument) -- whichever comes first, and possibly a call that did
 *    nothing wrong itself.  A caller that keeps everything on the device therefore synchronises the handle wherever the
 *    reference's throw has to surface: after an evaluation whose result it is about to use, and after
 *    mimi_hip_domain_post_time_advance.  The error is reported ONCE: reading the word clears it, and the handle stays
 *    usable (the failed kernel ran to its end: a point whose return map failed took no plastic step).
 */
#ifndef MIMI_HIP_H
#define MIMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIMI_HIP_ABI_VERSION 12

/* ---- errors ---------------------------------------------------------------- */
const char* mimi_hip_last_error(void);
int mimi_hip_abi_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never throws) */
int mimi_hip_device_count(void);

/* ---- materials (materials/materials.hpp, materials/material_hardening.hpp) -- */
enum mimi_hip_material_kind {
  MIMI_HIP_MAT_NEOHOOKEAN = 0, /* CompressibleOgdenNeoHookean  materials.hpp:118-140, materials.cpp:96-118 */
  MIMI_HIP_MAT_J2 = 1,         /* J2 (small strain, nonlinear isotropic hardening) materials.hpp:259-403 */
  MIMI_HIP_MAT_STVK = 2,       /* StVenantKirchhoff  materials.hpp:88-111, materials.cpp:72-94 */
  MIMI_HIP_MAT_J2LINEAR = 3,   /* J2Linear (linear isotropic + kinematic hardening)  materials.hpp:142-249 */
  MIMI_HIP_MAT_J2SIMO = 4,     /* J2Simo (finite strain, be / F_old state)  materials.hpp:406-557 */
  MIMI_HIP_MAT_J2LOG = 5       /* J2Log (logarithmic strain, Fp_inv state)  materials.hpp:559-753 */
};

enum mimi_hip_hardening_kind {
  MIMI_HIP_HARD_POWERLAW = 0,      /* material_hardening.hpp:79-98  */
  MIMI_HIP_HARD_VOCE = 1,          /* :100-121 */
  MIMI_HIP_HARD_JC = 2,            /* JohnsonCookHardening :123-143 */
  MIMI_HIP_HARD_JC_RATE = 3,       /* JohnsonCookRateDependentHardening :145-187 */
  MIMI_HIP_HARD_JC_TEMP_RATE = 4,  /* JohnsonCookTemperatureAndRateDependentHardening :189-280 */
  MIMI_HIP_HARD_JC_CONST_TEMP = 5  /* JohnsonCookConstantTemperatureHardening :282-346 */
};

typedef struct mimi_hip_material {
  int32_t kind;                 /* mimi_hip_material_kind */
  int32_t hardening;            /* mimi_hip_hardening_kind (J2 only) */
  /* MaterialBase (materials.hpp:31-38); set lambda/mu/K/G with mimi_hip_material_set_young_poisson */
  double density, lambda, mu, K, G;
  /* J2 thermo members (materials.hpp:268-273) */
  double heat_fraction, specific_heat, initial_temperature, melting_temperature;
  /* hardening parameters; unused ones are ignored */
  double sigma_y, n, eps0;                  /* PowerLaw (n shared with JohnsonCook) */
  double sigma_sat, strain_constant;        /* Voce */
  double A, B, C, eps0_dot;                 /* JohnsonCook: A + B eqps^n, rate term 1 + C ln(rate/eps0_dot) */
  double reference_temperature, m;          /* thermal softening exponent m */
  /* J2Linear (materials.hpp:149-151); its yield stress sigma_y_ is the field sigma_y above */
  double lin_isotropic_hardening, lin_kinematic_hardening;
} mimi_hip_material;

/* MaterialBase::SetYoungPoisson (materials.cpp:7-14) */
void mimi_hip_material_set_young_poisson(mimi_hip_material* mat, double young, double poisson);

/* ---- tangent mode ------------------------------------------------------------ */
enum mimi_hip_tangent_mode {
  MIMI_HIP_TANGENT_ANALYTIC = 0,     /* consistent tangent dP/dF, closed form (default) */
  MIMI_HIP_TANGENT_REFERENCE_FD = 1  /* the reference's element-level forward difference,
                                        step |u_i|*1e-8 or 1e-10 (nonlinear_solid.cpp:48-76) */
};

/* ---- domain integrator: integrators::NonlinearSolid ---------------------------- */
typedef struct mimi_hip_domain_s* mimi_hip_domain_t;

/* Flat form of what PrecomputedData hands the reference integrator
 * (utils/precomputed.hpp:58-130, utils/precomputed.cpp:39-330). */
typedef struct mimi_hip_domain_tables {
  int32_t dim;           /* 2 or 3 */
  int32_t n_elements;
  int32_t n_dof;         /* ElementData::n_dof, basis functions per element, <= 64 */
  int32_t n_quad;        /* ElementQuadData::n_quad, <= 125 */
  int64_t n_nodes;       /* global scalar dofs; n_vdofs = n_nodes*dim */
  const int32_t* dofs;   /* [n_elements][n_dof]   ElementData::dofs (precomputed.cpp:83) */
  const double* dN_dX;   /* [n_elements][n_quad][dim][n_dof]  QuadData::dN_dX, (n_dof x dim)
                            column-major per point (precomputed.cpp:316-321) */
  const double* weight_det; /* [n_elements][n_quad] integration_weight*det_dX_dxi (nonlinear_solid.hpp:79) */
  const int64_t* csr_rowptr; /* [n_vdofs+1] */
  const int32_t* csr_col;    /* [nnz], sorted within each row */
} mimi_hip_domain_tables;

/* NonlinearSolid ctor + Prepare() (nonlinear_solid.hpp:45-50, nonlinear_solid.cpp:31-46)
 * from flat per-point tables: works for any mesh / numbering / rational weights. */
int mimi_hip_domain_create(const mimi_hip_domain_tables* tables, const mimi_hip_material* material,
                           int device, mimi_hip_domain_t* out);

/* Tensor-product B-spline / NURBS patch description: the library builds the
 * 1-D basis tables, per-point inverse geometry Jacobians and weights itself
 * (replaces PrepareElementData + PrecomputeElementQuadData, precomputed.cpp:39-149,264-330)
 * and integrates by sum factorisation.  Lexicographic conventions: node
 * A = A0 + n0*(A1 + n1*A2), element e = e0 + m0*(e1 + m1*e2). */
typedef struct mimi_hip_bspline_patch {
  int32_t dim;
  int32_t degree[3];
  int32_t n_knots[3];
  const double* knots[3];        /* host pointers */
  const double* control_points;  /* host, [n_nodes][dim], lexicographic */
  const int64_t* node_ids;       /* host, [n_nodes] lexicographic -> global node id, or NULL (identity) */
  int32_t quadrature_order;      /* < 0: 2*p+3 (precomputed.cpp:284-286) */
  int32_t element_begin[3];      /* half-open element box [begin,end) integrated by THIS handle  */
  int32_t element_end[3];        /* (element sharding across GPUs); all zeros = whole patch       */
  const int64_t* csr_rowptr;     /* [n_vdofs+1] host or device */
  const int32_t* csr_col;        /* [nnz]       host or device */
  const double* weights;         /* host, [n_nodes] lexicographic NURBS weights, or NULL (all 1).  They must be a tensor
                                    product w[a0,a1,a2] = w0[a0] w1[a1] w2[a2] (arcs, cylinders, annuli, extrusions and
                                    revolutions are): the rational basis is then a tensor product too and every kernel
                                    family applies.  Other weights are refused here: hand such a patch to
                                    mimi_hip_domain_create as flat tables. */
} mimi_hip_bspline_patch;

int mimi_hip_domain_create_bspline(const mimi_hip_bspline_patch* patch, const mimi_hip_material* material,
                                   int device, mimi_hip_domain_t* out);

int mimi_hip_domain_destroy(mimi_hip_domain_t h);

/* public members dt_, first_effective_dt_, second_effective_dt_ that forms::Nonlinear
 * pushes before every call (nonlinear_base.hpp:23-25, forms/nonlinear.hpp:63-65) */
int mimi_hip_domain_set_dt(mimi_hip_domain_t h, double dt, double first_effective_dt,
                           double second_effective_dt);
int mimi_hip_domain_set_tangent_mode(mimi_hip_domain_t h, int mode);
/* stream = hipStream_t as void*; NULL = the handle's own (non-blocking) stream; MIMI_HIP_STREAM_NULL = the device's
 * null stream (hipStream_t 0: what e.g. torch's default stream is) */
#define MIMI_HIP_STREAM_NULL ((void*)(intptr_t)-1)
int mimi_hip_domain_set_stream(mimi_hip_domain_t h, void* stream);
int mimi_hip_domain_synchronize(mimi_hip_domain_t h);

/* AddDomainResidual(current_u, residual): r += R(u)   (nonlinear_solid.cpp:151-160) */
int mimi_hip_domain_add_residual(mimi_hip_domain_t h, const double* u, double* r);
/* AddDomainResidualAndGrad(current_u, grad_factor, residual, grad):
 * r += R(u); A_values += grad_factor * K(u)            (nonlinear_solid.cpp:162-177) */
int mimi_hip_domain_add_residual_and_grad(mimi_hip_domain_t h, const double* u, double grad_factor,
                                          double* r, double* A_values);
/* The same assembly with the old values of the matrix taken from a second array:
 *   r += R(u); A_out = A_base + grad_factor * K(u)
 * for WHOLE-PATCH handles only (refused on an element box / slab handle: "=" does not compose over boxes the way "+="
 * does -- a slab assembles with mimi_hip_domain_add_residual_and_grad into its copy of the base).  This is operators::NonlinearSolid::ResidualAndGrad's "jacobian_ values <- mass values, then
 * AddMultGrad" (operators/nonlinear_solid.cpp:257-258) without the copy pass: with both arrays on the device the row
 * gathers read A_base where "+=" would read A_out -- no extra traffic.  A_base == A_out is the plain "+=".  Routes
 * without a row gather (the atomics fallback of the general path) and host-resident arrays copy A_base into A_out first. */
int mimi_hip_domain_add_residual_and_grad_from(mimi_hip_domain_t h, const double* u, double grad_factor,
                                               double* r, const double* A_base, double* A_out);
/* DomainPostTimeAdvance(converged_u): commit material state (nonlinear_solid.cpp:179-199) */
int mimi_hip_domain_post_time_advance(mimi_hip_domain_t h, const double* u);

/* material state access (MaterialState of materials.hpp:278-286), for tests / output: `what` is one of */
enum mimi_hip_state {
  MIMI_HIP_STATE_EQPS = 0,         /* accumulated plastic strain [n_el][n_q] */
  MIMI_HIP_STATE_TEMPERATURE = 1,  /* temperature [n_el][n_q] */
  MIMI_HIP_STATE_MATRIX_1 = 2,     /* the material's first state matrix [n_el][n_q][dim*dim] (column-major per point):
                                      plastic strain (J2, J2Linear), be_old (J2Simo), Fp_inv (J2Log) */
  MIMI_HIP_STATE_MATRIX_2 = 3      /* its second one: beta (J2Linear, materials.hpp:158), F_old (J2Simo, materials.hpp:434) */
};
int mimi_hip_domain_get_state(mimi_hip_domain_t h, int what, double* out, int64_t capacity);
int mimi_hip_domain_reset_state(mimi_hip_domain_t h);

/* ---- field output -----------------------------------------------------------------
 * Beyond the reference (its only outputs are the x_ / v_ vectors), from its own quantities.  All fields are fp64.  At a
 * quadrature point, with F = I + grad u and P the first Piola-Kirchhoff stress mimi_hip_domain_add_residual would integrate
 * at this u (committed state, the dt of mimi_hip_domain_set_dt; no state is changed):
 *   CAUCHY       dim*dim components, column-major [i + j*dim]: sigma = P F^T / det F.  For the materials that go through the
 *                reference's pk1 conversion this is their sigma, for St. Venant-Kirchhoff F S F^T / J, for J2Simo the stress
 *                the reference actually uses.
 *   VON_MISES    sqrt(3/2) * || sigma - tr(sigma)/dim I ||_F.  The deviator takes the trace over dim, as the reference's
 *                own Dev does (material_utils.hpp:33,44): for J2 this is the q of its yield function, and in 3-D the usual
 *                von Mises stress; in 2-D it is NOT the plane-strain von Mises stress of the 3-D tensor.
 *   DET_F        det(I + grad u)
 *   EQPS         the committed accumulated plastic strain, the values of mimi_hip_domain_get_state(MIMI_HIP_STATE_EQPS)
 *   TEMPERATURE  the committed temperature, the values of mimi_hip_domain_get_state(MIMI_HIP_STATE_TEMPERATURE)
 * EQPS and TEMPERATURE need no u (NULL allowed) and, like mimi_hip_domain_get_state, fail for a material without state. */
enum mimi_hip_field {
  MIMI_HIP_FIELD_CAUCHY = 0,
  MIMI_HIP_FIELD_VON_MISES = 1,
  MIMI_HIP_FIELD_DET_F = 2,
  MIMI_HIP_FIELD_EQPS = 3,
  MIMI_HIP_FIELD_TEMPERATURE = 4
};
/* components of a field in `dim` dimensions; -1: unknown field */
int mimi_hip_field_components(int field, int dim);
/* out[e][q][c] over the handle's elements, overwritten (capacity: doubles `out` holds, at least n_el * n_q * components).
 * u and out host or device; synchronous when either is on the host, stream-ordered otherwise. */
int mimi_hip_domain_point_field(mimi_hip_domain_t h, const double* u, int field, double* out, int64_t capacity);
/* Lumped L2 projection onto the nodes, in accumulate form like every other output:
 *   sum[A][c] += sum_e sum_q w_q det_q N_A(q) f_c(q),    weight[A] += sum_e sum_q w_q det_q N_A(q)      (weight may be NULL)
 * over the handle's elements, A the caller's global node id (node_ids honoured); the caller divides.  Since N_A >= 0 and the
 * shape functions sum to one, the quotient reproduces constants and stays inside the range of the point values around the
 * node; element boxes and ranks compose by adding sums and weights before the division.  No atomics: two calls on the same
 * inputs give the same bytes.  sum [n_nodes][components], weight [n_nodes]. */
int mimi_hip_domain_nodal_field(mimi_hip_domain_t h, const double* u, int field, double* sum, double* weight);
/* flat-table handles only: QuadData::N [n_elements][n_quad][n_dof] (precomputed.hpp:58-71), copied; the flat tables carry
 * no shape values, and the nodal projection needs them.  Without it mimi_hip_domain_nodal_field on such a handle reports
 * an error that says so. */
int mimi_hip_domain_set_shape_values(mimi_hip_domain_t h, const double* N);
/* ---- mass, damping and body-force forms -----------------------------------------------------------------------------
 * The element integrals of set-up, assembled into the caller's CSR / vector (py_nonlinear_solid.cpp:155-192,221-283), over
 * the handle's elements (an element-box handle adds its box only: boxes and ranks compose by addition) with the handle's
 * own rule, w det and dN/dX -- the quantities the residual integrates with.  Outputs are accumulated; of a node block only
 * the dim diagonal-component entries are written, the i != j entries are not touched.  No state and no material is read,
 * no essential dofs are involved (the caller eliminates).  Host or device arrays: synchronous for host arrays,
 * stream-ordered otherwise.  No atomics: two calls on equal inputs give equal bytes.  Mass and body force on a flat-table
 * handle need mimi_hip_domain_set_shape_values.
 *   A_values[(A,i),(B,i)] += density   * sum_e sum_q w_q det_q N_a(q) N_b(q)                 i < dim   (VectorMassIntegrator) */
int mimi_hip_domain_add_mass(mimi_hip_domain_t h, double density, double* A_values);
/* A_values[(A,i),(B,i)] += viscosity * sum_e sum_q w_q det_q dN_a/dX_J(q) dN_b/dX_J(q)     i < dim   (VectorDiffusionIntegrator) */
int mimi_hip_domain_add_diffusion(mimi_hip_domain_t h, double viscosity, double* A_values);
/* r[(A,i)] += b[i] * sum_e sum_q w_q det_q N_a(q);   b: dim doubles on the host              (VectorDomainLFIntegrator) */
int mimi_hip_domain_add_body_force(mimi_hip_domain_t h, const double* b, double* r);
/* ---- tangent action: the product with the Jacobian without the matrix.  Together the two entries stand in for
 * forms::Nonlinear::AddMultGrad followed by SparseMatrix::Mult inside the reference's GMRES: linearize() is the part of
 * AddMultGrad that depends on u, apply_tangent() the product with what it assembled.
 * linearize: the snapshot of the tangent at u -- the committed state, the dt of set_dt; changes no state.  Neo-Hookean
 * handles keep a device copy of u and nothing per point (the action recomputes F); every other material keeps the record
 * w det dP/dF, dim^4 doubles per point.  A later commit, set_dt, or the caller overwriting u does not change what
 * apply_tangent returns.  u host or device. */
int mimi_hip_domain_linearize(mimi_hip_domain_t h, const double* u);
/* y += density * M x + stiffness * K(u_lin) x + viscosity * C x over the handle's elements (boxes and ranks compose by
 * addition); M, C the forms of mimi_hip_domain_add_mass / _add_diffusion with coefficient 1, K the tangent
 * add_residual_and_grad assembles with grad_factor 1.  No essential dofs (the caller masks).  x, y host or device.
 * stiffness != 0 needs a linearize() first; stiffness == 0 needs none.  The mass term on a flat-table handle needs
 * mimi_hip_domain_set_shape_values.  No atomics: equal inputs give equal bytes.  Stands in for SparseMatrix::Mult on the
 * matrix forms::Nonlinear::AddMultGrad assembled. */
int mimi_hip_domain_apply_tangent(mimi_hip_domain_t h, double density, double stiffness, double viscosity,
                                  const double* x, double* y);
/* ---- tangent diagonal: the node-block diagonal of the operator apply_tangent applies, without the matrix.  For a control
 * point A with local index a in element e
 *   D[A][i][j] = sum_{e of A} sum_q w_q det_q [ (density N_a^2 + viscosity |grad_X N_a|^2) delta_ij
 *                                               + stiffness d_J N_a (dP_iJ / dF_jL)(q) d_L N_a ],
 * the (A,i),(A,j) entries of what add_mass, add_diffusion and add_residual_and_grad(grad_factor = stiffness) assemble.
 * d += ...: block == 0 the diagonal, n_nodes dim doubles in byVDIM order; block != 0 the node blocks, n_nodes dim dim doubles
 * [A][i][j] row-major.  The entries i == j of the blocks are the diagonal to the bit (the same instructions compute both).
 * d host or device.  stiffness != 0 needs a linearize() first, the mass term on a flat-table handle
 * mimi_hip_domain_set_shape_values, as apply_tangent.  Reads the snapshot only: a later commit, set_dt, or an overwritten u
 * changes nothing.  No essential dofs (the caller eliminates).  Element boxes compose by addition.  No atomics: equal inputs
 * give equal bytes.  What mfem::DSmoother reads off the assembled matrix (py_nonlinear_solid.cpp:329-339), without it. */
int mimi_hip_domain_tangent_diagonal(mimi_hip_domain_t h, double density, double stiffness, double viscosity, int32_t block,
                                     double* d);
/* The two-step form of mimi_hip_domain_add_residual_and_grad, for a caller that needs some rows before the others (the
 * rows a neighbour rank is waiting for: mimi_amd/parallel.py, bench.py): integrate() runs the integration kernels of the
 * whole handle -- element row pieces and element residual pieces into the handle's scratch, nothing into r / A_values --
 * and gather() adds the rows of the nodes in the box [node_begin, node_end) (global node indices per direction, inside
 * the nodes the handle's elements touch) into r / A_values.  Every node must be gathered exactly once per integrate()
 * for the sum of the calls to equal one add_residual_and_grad (bitwise: same kernels, same order of additions per row).
 * Two-phase tensor paths only (3-D, degree 2 or 3, structured CSR, analytic tangent), device-resident arguments only;
 * other handles report an error and the caller stays with the one-call form. */
int mimi_hip_domain_integrate(mimi_hip_domain_t h, const double* u);
int mimi_hip_domain_gather(mimi_hip_domain_t h, double grad_factor, double* r, double* A_values,
                           const int32_t node_begin[3], const int32_t node_end[3]);
/* measurement aid (bench.py): HIP events on the launch stream around the two phases of the last two-phase tangent
 * assembly -- phase 1 = the integration kernel(s), phase 2 = the row gather.  Off by default (three event records per
 * call when on). */
int mimi_hip_domain_set_phase_timing(mimi_hip_domain_t h, int on);
int mimi_hip_domain_phase_ms(mimi_hip_domain_t h, double* phase1_ms, double* phase2_ms);
/* the same with phase 1 split at the end of its material pre-pass (0 when the path has none): pre-pass, integration /
 * contraction kernel, row gather */
int mimi_hip_domain_phase_ms_detail(mimi_hip_domain_t h, double* prepass_ms, double* integration_ms, double* gather_ms);
/* what MIMI_HIP_DOMAIN_INFO_LAST_FAMILY and _APPLY_FAMILY report */
enum mimi_hip_kernel_family {
  MIMI_HIP_FAMILY_NONE = 0,                 /* none yet */
  MIMI_HIP_FAMILY_TENSOR_P2_TWO_PHASE = 1,  /* two-phase tensor degree 2 */
  MIMI_HIP_FAMILY_TENSOR_P3_TWO_PHASE = 2,  /* two-phase tensor degree 3 */
  MIMI_HIP_FAMILY_TENSOR_SMALL = 3,         /* small-element tensor */
  MIMI_HIP_FAMILY_GENERAL = 4
};
/* what MIMI_HIP_DOMAIN_INFO_GENERAL_ROUTE reports: how the element pieces of the last assembly reached r and A_values */
enum mimi_hip_general_route {
  MIMI_HIP_GENERAL_ROUTE_NONE = 0,     /* none yet, or a two-phase tensor family (its own row gather) */
  MIMI_HIP_GENERAL_ROUTE_GATHER = 1,   /* element pieces stored, then the general row gather: MIMI_HIP_FAMILY_GENERAL and
                                          MIMI_HIP_FAMILY_TENSOR_SMALL */
  MIMI_HIP_GENERAL_ROUTE_ATOMICS = 2   /* MIMI_HIP_FAMILY_GENERAL adding into r and A_values with atomics: a CSR row longer
                                          than the gather's row image, no room for the element blocks, or
                                          MIMI_HIP_GENERAL_NO_TWO_PHASE=1 at create */
};
/* sizes and what the handle last did: `what` of mimi_hip_domain_info.  Tests assert them; an unknown code returns -1 */
enum mimi_hip_domain_info_what {
  MIMI_HIP_DOMAIN_INFO_N_ELEMENTS = 0,
  MIMI_HIP_DOMAIN_INFO_N_QUAD = 1,
  MIMI_HIP_DOMAIN_INFO_N_DOF = 2,
  MIMI_HIP_DOMAIN_INFO_NNZ = 3,
  MIMI_HIP_DOMAIN_INFO_N_VDOFS = 4,
  MIMI_HIP_DOMAIN_INFO_PATH = 5,                  /* 0 general, 1 tensor */
  MIMI_HIP_DOMAIN_INFO_CSR_KIND = 6,              /* 0 any, 1 structured lexicographic, 2 structured permuted */
  MIMI_HIP_DOMAIN_INFO_LAST_FAMILY = 7,           /* mimi_hip_kernel_family of the last assembly on the handle */
  MIMI_HIP_DOMAIN_INFO_HAS_GRADIENT_TABLES = 8,   /* whether the handle currently holds per-point gradient tables dN_dX
                                                     (flat-table handles always; patch handles once a general kernel ran) */
  MIMI_HIP_DOMAIN_INFO_APPLY_FAMILY = 9,          /* mimi_hip_kernel_family of the last tangent action on the handle */
  MIMI_HIP_DOMAIN_INFO_LINEARIZATION_BYTES = 10,  /* bytes of linearisation record the handle holds (0 before a linearize
                                                     and on neo-Hookean handles) */
  /* the launch geometry of the handle's last assembly on the symmetric-half degree-2 kernel (neo-Hookean tangent,
   * MIMI_HIP_FAMILY_TENSOR_P2_TWO_PHASE; 0 before any): */
  MIMI_HIP_DOMAIN_INFO_SEGMENT_LENGTH = 11,       /* elements per unit -- the box's column length, or the segment length
                                                     where the columns were cut */
  MIMI_HIP_DOMAIN_INFO_UNITS_PER_WORKGROUP = 12,  /* units a workgroup walks back to back (1..4) */
  MIMI_HIP_DOMAIN_INFO_GENERAL_ROUTE = 13         /* mimi_hip_general_route of the last assembly on the handle */
};
int64_t mimi_hip_domain_info(mimi_hip_domain_t h, int what);

/* ---- structured sparsity: PrecomputedData::PrepareSparsity (precomputed.cpp:151-174) ----
 * CSR pattern of a single B-spline patch with lexicographic node numbering, built on the
 * device.  Call once with col == NULL to fill rowptr ([n_vdofs+1], device or host) and get
 * nnz, then again with col ([nnz], device or host). */
int mimi_hip_bspline_sparsity(int32_t dim, const int32_t n_nodes_dir[3], const int32_t degree[3],
                              int device, int64_t* rowptr, int32_t* col, int64_t* nnz);
/* Row slice of the same pattern, for a rank that owns a box of nodes (one slab of the patch): rowptr keeps its full
 * length [n_vdofs+1], rows of nodes outside [node_begin, node_end) get zero length, and col / the value array hold
 * only the slice (nnz = the slice's entries).  A domain handle accepts such a pattern when the box covers every node
 * its elements touch: the integration kernels only ever write rows of those nodes.  Column indices stay global. */
int mimi_hip_bspline_sparsity_rows(int32_t dim, const int32_t n_nodes_dir[3], const int32_t degree[3],
                                   const int32_t node_begin[3], const int32_t node_end[3], int device,
                                   int64_t* rowptr, int32_t* col, int64_t* nnz);

/* ---- exchange step of a sharded assembly (no reference counterpart beyond the in-process reduction of
 * integrators/nonlinear_base.hpp:90-151) ----
 * The rows `rows[0..n_rows)` (distinct, device int64) of the residual `r` and of the CSR value array travel as one
 * message: [n_rows residual entries][the rows' values, row after row]; offsets[k] (device int64) = position of row k's
 * values in the message (n_rows + the lengths of the rows before it).  A_values == NULL: residual entries only.
 * All pointers are device pointers; the kernels are enqueued on `stream` (NULL or MIMI_HIP_STREAM_NULL: the null stream)
 * of the current device and return at once. */
int mimi_hip_rows_zero(void* stream, const int64_t* rowptr, const int64_t* rows, int64_t n_rows, double* r, double* A_values);
int mimi_hip_rows_pack(void* stream, const int64_t* rowptr, const int64_t* rows, const int64_t* offsets, int64_t n_rows,
                       const double* r, const double* A_values, double* message);
int mimi_hip_rows_unpack_add(void* stream, const int64_t* rowptr, const int64_t* rows, const int64_t* offsets, int64_t n_rows,
                             const double* message, double* r, double* A_values);
/* The same message with the rows trimmed to the entries the sender's elements can have written (ABI 12): of a shared row
 * only the columns inside the sender's own node planes are not zero by construction (3 of the 5 column planes of a degree-2
 * row), so only those travel: [n_rows residual entries][A_values[positions[0..n_positions)]].  positions (device int64,
 * distinct) are places in the value array; sender and receiver list the same (row, column) pairs in the same order, each in
 * its own array (mimi_amd/parallel.py InterfaceExchange builds both from the slab bounds).  A_values == NULL: residual
 * entries only. */
int mimi_hip_entries_pack(void* stream, const int64_t* rows, int64_t n_rows, const int64_t* positions, int64_t n_positions,
                          const double* r, const double* A_values, double* message);
int mimi_hip_entries_unpack_add(void* stream, const int64_t* rows, int64_t n_rows, const int64_t* positions, int64_t n_positions,
                                const double* message, double* r, double* A_values);

/* ---- contact integrator: integrators::MortarContact ------------------------------ */
typedef struct mimi_hip_contact_s* mimi_hip_contact_t;

enum mimi_hip_rigid_body_kind {
  MIMI_HIP_BODY_SPHERE = 0, /* params: centre[3], radius */
  MIMI_HIP_BODY_PLANE = 1,  /* params: point[3], unit normal[3] pointing out of the rigid half space */
  MIMI_HIP_BODY_SPLINE = 2  /* mimi_hip_contact_tables::spline: one B-spline / NURBS curve (2-D) or surface (3-D) */
};

/* NearestDistanceToSplines with its one boundary spline (coefficients/nearest_distance.hpp:215-288): para_dim = dim - 1.
 * Orientation as in the reference (Results::ComputeNormal, :139-184): the rigid normal is (t_y, -t_x) of the curve
 * tangent in 2-D, S_u x S_v in 3-D, and must point out of the rigid body. */
typedef struct mimi_hip_spline_body {
  int32_t para_dim;
  int32_t degree[2];             /* <= 5 */
  int32_t n_knots[2];
  const double* knots[2];        /* host */
  const double* control_points;  /* host, [n_ctrl][dim], first parametric direction fastest */
  const double* weights;         /* host, [n_ctrl], or NULL */
  int32_t kdtree_resolution;     /* PlantKdTree(resolution, nthreads) (:243-255): sample points per direction for the
                                    initial guess of the search */
  int32_t max_iterations;        /* Query::max_iterations (:29); <= 0: 50 */
} mimi_hip_spline_body;

/* Flat form of the boundary-element tables MortarContact::Prepare builds
 * (mortar_contact.cpp:19-133) plus the analytic rigid body standing in for
 * NearestDistanceBase (coefficients/nearest_distance.hpp:14-213). */
typedef struct mimi_hip_contact_tables {
  int32_t dim;
  int32_t n_faces;
  int32_t n_dof;        /* per face, <= 16 */
  int32_t n_quad;       /* <= 25 */
  int64_t n_nodes;
  const int32_t* dofs;  /* [n_faces][n_dof] global node ids of the marked boundary elements */
  const double* N;      /* [n_faces][n_quad][n_dof]          QuadData::N */
  const double* dN_dxi; /* [n_faces][n_quad][dim-1][n_dof]   QuadData::dN_dxi */
  const double* weight; /* [n_faces][n_quad]                 QuadData::integration_weight */
  const double* x_ref;  /* [n_nodes][dim] reference coordinates of the control points (byVDIM) */
  int32_t body_kind;
  double body[8];
  double penalty;       /* NearestDistanceBase::coefficient_ (nearest_distance.hpp:18) */
  const int64_t* csr_rowptr;
  const int32_t* csr_col;
  const mimi_hip_spline_body* spline;  /* body_kind == MIMI_HIP_BODY_SPLINE, else NULL */
} mimi_hip_contact_tables;

int mimi_hip_contact_create(const mimi_hip_contact_tables* tables, int device, mimi_hip_contact_t* out);
int mimi_hip_contact_destroy(mimi_hip_contact_t h);
int mimi_hip_contact_set_tangent_mode(mimi_hip_contact_t h, int mode);
int mimi_hip_contact_set_stream(mimi_hip_contact_t h, void* stream);
int mimi_hip_contact_synchronize(mimi_hip_contact_t h);
/* AddBoundaryResidual (mortar_contact.cpp:297-351) */
int mimi_hip_contact_add_residual(mimi_hip_contact_t h, const double* u, double* r);
/* AddBoundaryResidualAndGrad (mortar_contact.cpp:353-421) */
int mimi_hip_contact_add_residual_and_grad(mimi_hip_contact_t h, const double* u, double grad_factor,
                                           double* r, double* A_values);
/* GapNorm (mortar_contact.cpp:423-467) */
int mimi_hip_contact_gap_norm(mimi_hip_contact_t h, const double* u, double* out);
/* last_area_, last_pressure_, last_force_[dim] of the latest Add* call
 * (mortar_contact.hpp:33-35; BoundaryPostTimeAdvance mortar_contact.cpp:469-488):
 * out[0] = area, out[1] = pressure integral, out[2..2+dim) = force */
int mimi_hip_contact_last_history(mimi_hip_contact_t h, double* out5);
/* nodal average_pressure_ (mortar_contact.hpp:59), [n_marked]; returns n_marked via *n */
int mimi_hip_contact_get_pressure(mimi_hip_contact_t h, double* out, int64_t capacity, int64_t* n);

/* The rigid body moved (examples/nl_contact.py moves the curve's control points and calls plant_kd_tree again before
 * every step) and / or the penalty changed (scene.coefficient = ...): spline != NULL re-uploads the boundary spline and its
 * sampled initial guesses (same layout rules as at create time); penalty > 0 replaces coefficient_. */
int mimi_hip_contact_update_body(mimi_hip_contact_t h, const mimi_hip_spline_body* spline, double penalty);

/* Multi-GPU (one handle per rank over the faces of its element slab): the nodal area / gap of nodes shared between
 * slabs must be summed over the ranks before the pressure is formed (mortar_contact.cpp:195-261 runs over all marked
 * faces).  gap_area = pass 1 only; marked_nodes = the sorted global node ids behind the nodal arrays (out == NULL: count
 * only); nodal = read (set 0) or write (set 1) the nodal area / gap arrays [n_marked], host or device pointers;
 * add_residual_from_nodal = pressure + pass 2 (A_values == NULL: residual only). */
int mimi_hip_contact_gap_area(mimi_hip_contact_t h, const double* u);
int mimi_hip_contact_marked_nodes(mimi_hip_contact_t h, int32_t* out, int64_t capacity, int64_t* n);
int mimi_hip_contact_nodal(mimi_hip_contact_t h, int set, double* area, double* gap);
int mimi_hip_contact_add_residual_from_nodal(mimi_hip_contact_t h, const double* u, double grad_factor, double* r,
                                             double* A_values);

/* Matrix-free action of the contact tangent: stands in for MortarContact::AddBoundaryResidualAndGrad
 * (mortar_contact.cpp:353-421) followed by SparseMatrix::Mult on what it assembled.  The tangent is the analytic one with
 * the nodal pressure frozen (mortar_contact.cpp:263-295), R(a,i) = -w p_q N_a m_i, whatever the tangent mode:
 *   (K x)(a,i) = sum_q c_q N_a dm_i,  c_q = -w p_q,  dm = dt_1 x t_2 + t_1 x dt_2 (3-D), (dt_y, -dt_x) (2-D),  dt_k = sum_b N_b,k x_b.
 * linearize = the snapshot at u: pass 1 and the pressure with the handle's current body and penalty (the nodal area / gap /
 * pressure of the handle are overwritten, the history of the last Add* call is not), then per face point c_q and the
 * surface tangents t, per face the IsPressureZero flag, in buffers of their own.  The record survives every later call on
 * the handle (Add* at another u, update_body, gap_norm); no copy of u is kept and no face tangent block is allocated.
 * apply_tangent: y += factor K(u of linearize) x over the recorded active faces, summed per node in the order of the face
 * incidences (no atomics: equal inputs give equal bytes); refused before the first linearize.  u, x, y host or device. */
int mimi_hip_contact_linearize(mimi_hip_contact_t h, const double* u);
int mimi_hip_contact_apply_tangent(mimi_hip_contact_t h, double factor, const double* x, double* y);
/* `what` of mimi_hip_contact_action_info and mimi_hip_follower_action_info (the latter knows _BYTES and _FACE_BLOCKS) */
enum mimi_hip_action_info_what {
  MIMI_HIP_ACTION_INFO_BYTES = 0,        /* bytes of the record (n_faces n_quad (1 + (dim - 1) dim) doubles + n_faces flags;
                                            0 before the first linearize; a consistent record: n_faces n_quad
                                            (2 + dim + (dim - 1) dim) doubles + 2 n_marked doubles + n_faces flags) */
  MIMI_HIP_ACTION_INFO_FACE_BLOCKS = 1,  /* whether the face tangent blocks of an assembly are allocated */
  MIMI_HIP_ACTION_INFO_CONSISTENT = 2,   /* whether the current record is a consistent one
                                            (mimi_hip_contact_set_consistent_tangent) */
  MIMI_HIP_ACTION_INFO_FRICTION = 3,     /* whether it carries friction (mimi_hip_contact_set_friction_action; _BYTES then
                                            includes n_faces n_quad (8 (dim + 1) + 1) + 8 bytes more) */
  MIMI_HIP_ACTION_INFO_AUGMENTED = 4     /* whether the current record was made in the augmented-Lagrangian mode
                                            (mimi_hip_contact_set_augmented; a consistent one then holds n_marked doubles
                                            more) */
};
/* -1: bad argument */
int64_t mimi_hip_contact_action_info(mimi_hip_contact_t h, int what);

/* The consistent contact tangent as an action (the reference has none: its Jacobian freezes the nodal pressure,
 * mortar_contact.cpp:281-294, so Newton is a fixed-point iteration in p_i = eps G_i / A_i).  on != 0: the NEXT linearize
 * records, on top of the frozen record, per face point the gap g_q and chi_q nu_q (chi_q = [g_q != 0], nu_q the body's unit
 * normal at the closest point), per marked node copies of A_i and p_i, and the penalty; apply_tangent (and a Krylov operator
 * built on the handle) then adds
 *   -sum_q w dp_q N_a m_i,  dp_q = sum_i N_i dp_i,  dp_i = (eps dG_i - p_i dA_i) / A_i,
 *   dA_i = sum_q w (n.dm) N_i,  dG_i = sum_q w ((n.dm) g_q + |m| chi_q nu_q.dx_q) N_i,  dx_q = sum_b N_b x_b
 * to the frozen action: the exact derivative of the residual with the active set frozen.  The term couples nodes up to
 * 2 p basis functions apart, outside the CSR pattern: it cannot be assembled, add_residual_and_grad is unchanged.  The
 * nodal sums run over the handle's own faces.  Takes effect at the next linearize and never touches an existing record;
 * on == 0 (the default): launches and bytes of every entry are those of a handle that never saw this call.  Refused with
 * friction (mu > 0) unless mimi_hip_contact_set_friction_action is on. */
int mimi_hip_contact_set_consistent_tangent(mimi_hip_contact_t h, int on);

/* Coulomb friction (the reference has none; model and layout: DESIGN.md "Coulomb friction").  At a face point with
 * p_N = -p_h > 0 that was in contact at the last commit: a = xi + x_q - xbar - d, s = (I - n n^T) a on the deformable
 * surface's own normal; stick (eps_t |s| <= mu p_N): t = eps_t s, xi' = s; slip: t = mu p_N s / |s|, xi' = t / eps_t;
 * r(a,i) += sum_q w |m| N_a t_i, exact tangent with the nodal pressures, the state, d and the branch frozen.  A point that
 * is new in contact carries no traction in that step.  Every Add* call writes a TRIAL state; only post_time_advance
 * commits.  mu = 0 (the default): launches and bytes of every other entry are those of a handle without friction.
 *   set_friction        mu >= 0, eps_t > 0 (with mu > 0); the first mu > 0 allocates the state (xi = 0, no point in contact).
 *                       Refused in the reference-FD tangent mode; with mu > 0 set_tangent_mode(REFERENCE_FD), linearize and
 *                       apply_tangent (and a Krylov operator built on the handle) are refused -- the last three only until
 *                       mimi_hip_contact_set_friction_action(h, 1), below.
 *   set_body_increment  d[dim]: the rigid body's displacement over the current step (NULL: zero)
 *   post_time_advance   u != NULL: an evaluation at u (pass 1, pressure, pass 2 without the gather: the history scalars are
 *                       those of u), then commit.  u == NULL: commit the trial state of the latest evaluation on the
 *                       handle's stream -- nothing is recomputed and nothing waits for the device.
 *   reset_friction      xi = 0, no point in contact, no trial state
 *   friction_history    of the latest evaluation: out[0..3) = sum da t (friction force on the body), out[3] = sum da |t|,
 *                       out[4] = sticking points, out[5] = slipping points
 *   friction_state      the committed state to the host: xi, xbar [n_faces][n_quad][dim], c [n_faces][n_quad] (each may
 *                       be NULL) */
int mimi_hip_contact_set_friction(mimi_hip_contact_t h, double mu, double eps_t);
int mimi_hip_contact_set_body_increment(mimi_hip_contact_t h, const double* d);
int mimi_hip_contact_post_time_advance(mimi_hip_contact_t h, const double* u);
int mimi_hip_contact_reset_friction(mimi_hip_contact_t h);
int mimi_hip_contact_friction_history(mimi_hip_contact_t h, double* out6);
int mimi_hip_contact_friction_state(mimi_hip_contact_t h, double* xi, double* xbar, unsigned char* c);

/* Friction on the matrix-free route (csrc/kernels_face_friction_action.hpp).  on == 0 (the default): every refusal above
 * stands, no buffer is allocated and no launch changes.  on != 0: linearize, apply_tangent, a Krylov operator built on the
 * handle and set_consistent_tangent accept a handle with mu > 0; the reference-FD tangent mode stays refused.  A linearize
 * with mu > 0 then records, on top of the frozen (and, when set, the consistent) record, per face point
 * a_q = xi + x_q - xbar - d (dim doubles), coef_q (eps_t in stick, mu p_N / |s| in slip, 0 where the point carries no
 * traction) and the branch (one byte), and mu: n_faces n_quad (8 (dim + 1) + 1) + 8 bytes.  It reads the COMMITTED state, d,
 * mu and eps_t of that moment and the nodal pressure at u; it writes neither the trial state nor the history scalars.
 * The record is a snapshot: set_friction, set_body_increment, post_time_advance, reset_friction, update_body and any
 * evaluation leave it alone, only the next linearize replaces it.  apply_tangent then adds, with tau the traction,
 *   sum_q w N_a (tau_i nD + |m| dtau_i),  nD = n.dm,  dn = (dm - n nD) / |m|,  ds = (I - n n^T) dx_q - dn (n.a) - n (dn.a),
 *   dtau = coef (ds - [slip] sh (sh.ds))     (the assembled friction tangent applied to x)
 * and, on a consistent record, -mu dp_q sh to dtau at slipping points: there tau = mu p_N sh, so the frozen-pressure tangent
 * drops a first-order term of the friction residual itself.  One face kernel takes the place of the frictionless one:
 * friction adds no launch to a product.  With mu == 0 at the linearize the record and the launches are the frictionless
 * ones. */
int mimi_hip_contact_set_friction_action(mimi_hip_contact_t h, int on);

/* Augmented-Lagrangian contact (the reference has none; law, rate and limits: DESIGN.md "Augmented-Lagrangian contact").
 * Per marked node a multiplier lambda_i <= 0 (the sign of p_i: compressive is negative).  In the mode
 *   pass 1    the point gap enters the nodal sum unclamped: g_q = true_g, 0 where the angle rule rejects the point;
 *             Gt_i = sum_q w |J| g_q N_i, gt_i = Gt_i / A_i (what mimi_hip_contact_nodal then reads as the gap)
 *   pressure  p_i = min(0, lambda_i + eps gt_i)
 * and everything that reads p_i (pass 2, the assembled frozen tangent, the frozen action, friction) is unchanged.  A
 * consistent record of the mode holds the unclamped g_q, chi_q = "the angle rule accepted the point" and G_l, and
 *   dp_l = eps (dGt_l - gt_l dA_l) / A_l on the nodes with p_l < 0, 0 on the others.
 *   set_augmented    on != 0: the mode; the first switch-on allocates lambda, every switch from off to on zeroes it.  Off
 *                    (the default): launches and bytes of every entry are those of a handle that never saw this call.
 *                    Refused in the reference-FD tangent mode, and set_tangent_mode(REFERENCE_FD) is refused in the mode.
 *   lagrange         get (set == 0) / set the multipliers at the marked nodes, in the order of
 *                    mimi_hip_contact_marked_nodes; host or device pointer; set values are projected onto lambda <= 0 on
 *                    the device.  Refused on a handle that never was in the mode.
 *   update_lagrange  the Uzawa step: pass 1 at u (the handle's nodal area / gap are overwritten, the history scalars of
 *                    the last Add* call are not), dlambda_i = p_i - lambda_i = min(-lambda_i, eps gt_i), and with
 *                    apply != 0 lambda_i <- p_i (exactly 0.0 on a released node).  out4 (host): max_i |dlambda_i| / eps (a
 *                    length: the violation of the constraint), sqrt(sum_i A_i dlambda_i^2), the number of nodes with
 *                    p_i < 0, max_i |lambda_i| after the call.  Fixed-shape reductions, no atomics: equal inputs give equal
 *                    bytes.  u host or device.
 * mimi_hip_contact_action_info(h, MIMI_HIP_ACTION_INFO_AUGMENTED) tells whether the current record was made in the mode. */
int mimi_hip_contact_set_augmented(mimi_hip_contact_t h, int on);
int mimi_hip_contact_lagrange(mimi_hip_contact_t h, int set, double* lambda);
int mimi_hip_contact_update_lagrange(mimi_hip_contact_t h, const double* u, int apply, double* out4);

/* ---- follower-pressure boundary integrator (integrators::FollowerPressure) ---------------------------------------
 * The reference stores BCMarker::Pressure(bid, value) (utils/boundary_conditions.cpp:43-50) and never applies it; here it
 * is the follower load t = -p n da on the CURRENT surface x = X + u of a set of faces of one patch:
 *   r(a,i)    += sum_q w_q p_q N_a m_i                         (m: the non-normalised outward normal, a_1 x a_2 in 3-D,
 *   A(ai, bj) += grad_factor sum_q w_q p_q N_a dm_i/dx_bj        (a_y, -a_x) in 2-D, as in the contact integrator)
 * p_q = the uniform value, or sum_a N_a p_a of values at the faces' nodes.  The tangent is exact and not symmetric.
 * Tables: the same layout rules as mimi_hip_contact_tables (face orientation such that m points out of the body); the
 * contributions are summed per CSR row in a fixed order (no atomics: bitwise reproducible). */
typedef struct mimi_hip_pressure_s* mimi_hip_pressure_t;
typedef struct mimi_hip_pressure_tables {
  int32_t dim;
  int32_t n_faces;
  int32_t n_dof;        /* per face, <= 16 */
  int32_t n_quad;       /* <= 25 */
  int64_t n_nodes;
  const int32_t* dofs;  /* [n_faces][n_dof] global node ids (QuadData of the boundary elements, as for contact) */
  const double* N;      /* [n_faces][n_quad][n_dof]          QuadData::N */
  const double* dN_dxi; /* [n_faces][n_quad][dim-1][n_dof]   QuadData::dN_dxi */
  const double* weight; /* [n_faces][n_quad]                 QuadData::integration_weight */
  const double* x_ref;  /* [n_nodes][dim] reference coordinates of the control points (byVDIM) */
  const int64_t* csr_rowptr;
  const int32_t* csr_col;
} mimi_hip_pressure_tables;

int mimi_hip_pressure_create(const mimi_hip_pressure_tables* tables, int device, mimi_hip_pressure_t* out);
int mimi_hip_pressure_destroy(mimi_hip_pressure_t h);
/* NULL = the handle's own stream; MIMI_HIP_STREAM_NULL = the device's null stream */
int mimi_hip_pressure_set_stream(mimi_hip_pressure_t h, void* stream);
int mimi_hip_pressure_synchronize(mimi_hip_pressure_t h);
/* BCMarker::pressure_[bid] (boundary_conditions.cpp:43-50): a uniform pressure, used from the next assembly on (also
 * after set_nodal); 0 at create time.  A face whose pressure is zero everywhere adds nothing to r / A_values. */
int mimi_hip_pressure_set_value(mimi_hip_pressure_t h, double p);
/* the sorted global node ids of the faces, the order of set_nodal's values (out == NULL: count only) */
int mimi_hip_pressure_face_nodes(mimi_hip_pressure_t h, int32_t* out, int64_t capacity, int64_t* n);
/* pressure values at the face nodes [n], host or device; p == NULL: back to the uniform value */
int mimi_hip_pressure_set_nodal(mimi_hip_pressure_t h, const double* p, int64_t n);
/* AddBoundaryResidual: r += R(u) (stands in for the dead-load VectorBoundaryLFIntegrator of py_nonlinear_solid.cpp:243-283,
 * which the reference applies for traction only) */
int mimi_hip_pressure_add_residual(mimi_hip_pressure_t h, const double* u, double* r);
/* AddBoundaryResidualAndGrad: r += R(u); A_values += grad_factor dR/du */
int mimi_hip_pressure_add_residual_and_grad(mimi_hip_pressure_t h, const double* u, double grad_factor, double* r,
                                            double* A_values);
/* of the latest Add* call (as mimi_hip_contact_last_history for last_area_ / last_force_, mortar_contact.hpp:33-35):
 * out[0] = current area of the faces, out[1..1+dim) = external force -sum p m w; unused entries 0 */
int mimi_hip_pressure_last_history(mimi_hip_pressure_t h, double* out4);
/* Matrix-free action of the follower-pressure tangent, the twin of mimi_hip_contact_linearize / _apply_tangent (there:
 * MortarContact::AddBoundaryResidualAndGrad, mortar_contact.cpp:353-421, followed by SparseMatrix::Mult): c_q = w p_q with
 * the uniform or nodal pressure the handle holds at linearize; the record survives set_value / set_nodal and every Add*
 * call.  action_info as mimi_hip_contact_action_info. */
int mimi_hip_follower_linearize(mimi_hip_pressure_t h, const double* u);
int mimi_hip_follower_apply_tangent(mimi_hip_pressure_t h, double factor, const double* x, double* y);
int64_t mimi_hip_follower_action_info(mimi_hip_pressure_t h, int what);

/* ---- coupling surface (partitioned fluid-structure coupling) ---------------------------------------------------------
 * What a fluid partner exchanges with the solid every coupling iteration of the reference's fixed-point loop
 * (fixed_point_solve2 / fixed_point_advance2 / advance_time2: py/py_solid.cpp:443-511, solvers/ode.cpp:81-186), on the
 * faces of a mimi_hip_pressure_tables (the same tables, rule and outward normal m as the pressure integrator; csr_rowptr /
 * csr_col are not read), for the configuration x = X + u (u == NULL: the reference configuration):
 *   points    x_q = sum_a N_a x_a,  normal n_q = m_q / |m_q|,  area weight w_q |m_q|  -- face-major, point-minor
 *   add_load  f(a,i) += sum_q w_q |m_q| N_a(xi_q) t(q,i): the consistent nodal forces of a traction t per unit area of x
 *             (Cauchy for the current configuration, nominal for the reference one); a dead load, no tangent
 * u, t, the outputs and f: host or device pointers, as for the integrators' add calls.  No atomics: the same bits every
 * run. */
typedef struct mimi_hip_surface_s* mimi_hip_surface_t;
int mimi_hip_surface_create(const mimi_hip_pressure_tables* tables, int device, mimi_hip_surface_t* out);
int mimi_hip_surface_destroy(mimi_hip_surface_t h);
/* NULL = the handle's own stream; MIMI_HIP_STREAM_NULL = the device's null stream */
int mimi_hip_surface_set_stream(mimi_hip_surface_t h, void* stream);
int mimi_hip_surface_synchronize(mimi_hip_surface_t h);
/* n_faces * n_quad (-1: null handle) */
int64_t mimi_hip_surface_n_points(mimi_hip_surface_t h);
/* x[n_points][dim], normal[n_points][dim], weight[n_points]: each output may be NULL */
int mimi_hip_surface_points(mimi_hip_surface_t h, const double* u, double* x, double* normal, double* weight);
/* t[n_points][dim]: f[n_vdofs] += the nodal forces */
int mimi_hip_surface_add_load(mimi_hip_surface_t h, const double* u, const double* t, double* f);

/* ---- periodic fold (BCMarker::PeriodicBoundary, boundary_conditions.cpp:152-159) ---------------------------------
 * The integrators assemble into the patch's unwrapped structured CSR (rowptr_u / col_u); P is the 0/1 map from the
 * folded (periodic) dofs to the unwrapped ones, given per node: node_map[n_nodes_u] -> folded node, onto [0, n_nodes_f)
 * (vdof n dim + c -> node_map[n] dim + c).  The folded pattern is that of P^T A P, columns sorted.  No atomics: the same
 * bits every run.  Host or device pointers; the work runs on the handle's stream. */
typedef struct mimi_hip_fold_s* mimi_hip_fold_t;
int mimi_hip_fold_create(int32_t dim, int64_t n_nodes_u, const int64_t* node_map, const int64_t* rowptr_u,
                         const int32_t* col_u, int device, mimi_hip_fold_t* out);
int mimi_hip_fold_destroy(mimi_hip_fold_t h);
enum mimi_hip_fold_info_what {
  MIMI_HIP_FOLD_INFO_N_NODES_F = 0,
  MIMI_HIP_FOLD_INFO_NNZ_F = 1,
  MIMI_HIP_FOLD_INFO_NNZ_U = 2,
  MIMI_HIP_FOLD_INFO_ROW_CAPACITY = 3,  /* longest folded row (rounded up to 8) */
  MIMI_HIP_FOLD_INFO_SERIAL_ROWS = 4    /* folded rows added by one lane (a source row whose window wraps onto itself) */
};
/* -1: bad argument */
int64_t mimi_hip_fold_info(mimi_hip_fold_t h, int what);
/* the folded pattern: rowptr_f[n_nodes_f dim + 1], col_f[nnz_f] (col_f NULL: rowptr only) */
int mimi_hip_fold_pattern(mimi_hip_fold_t h, int64_t* rowptr_f, int32_t* col_f);
/* NULL = the handle's own stream; MIMI_HIP_STREAM_NULL = the device's null stream */
int mimi_hip_fold_set_stream(mimi_hip_fold_t h, void* stream);
int mimi_hip_fold_synchronize(mimi_hip_fold_t h);
/* u_u = P u_f */
int mimi_hip_fold_expand(mimi_hip_fold_t h, const double* u_f, double* u_u);
/* r_f += P^T r_u (r_u == r_f == NULL: matrix only);  A_f = A_base + P^T A_u P (A_base == A_f: "+="; A_base == NULL:
 * A_f = P^T A_u P; A_u == NULL: residual only) */
int mimi_hip_fold_add(mimi_hip_fold_t h, const double* r_u, double* r_f, const double* A_u, const double* A_base,
                      double* A_f);

/* ---- the callers' steps around the assembly, device-resident ---------------------------
 * One handle per CSR pattern (rowptr / col host or device; device arrays are used in place and must outlive the
 * handle) and list of essential dofs (forms::Nonlinear's zero_dofs). */
typedef struct mimi_hip_linear_s* mimi_hip_linear_t;
int mimi_hip_linear_create(int64_t n, const int64_t* csr_rowptr, const int32_t* csr_col, const int64_t* ess_dofs,
                           int64_t n_ess, int device, mimi_hip_linear_t* out);
int mimi_hip_linear_destroy(mimi_hip_linear_t h);
/* NULL = the handle's own stream */
int mimi_hip_linear_set_stream(mimi_hip_linear_t h, void* hip_stream);
enum mimi_hip_linear_info_what {
  MIMI_HIP_LINEAR_INFO_ROWS = 0,
  MIMI_HIP_LINEAR_INFO_NNZ = 1,           /* stored entries */
  MIMI_HIP_LINEAR_INFO_ROW_GROUP = 2,     /* consecutive rows that share one column list (3 or 2: the dofs of a node in the
                                             byVDIM numbering of py_nonlinear_solid.cpp:63 -- the products read the list once
                                             per group; 1: any other pattern) */
  MIMI_HIP_LINEAR_INFO_NODE_COLUMNS = 3   /* whether that shared list is made of node triples 3 c, 3 c + 1, 3 c + 2 (1: the
                                             products read one index per node, a ninth of the index bytes) */
};
/* -1: bad argument */
int64_t mimi_hip_linear_info(mimi_hip_linear_t h, int what);
/* forms::Nonlinear::AddMult / AddMultGrad tail (forms/nonlinear.hpp:76-80,112-115): r[ess] = 0 (r may be NULL);
 * A.EliminateRowCol(ess, DIAG_ONE) on the CSR values (A_values may be NULL).  Host or device pointers. */
int mimi_hip_linear_eliminate(mimi_hip_linear_t h, double* r, double* A_values);
/* y += alpha A x on the handle's pattern (mfem::SparseMatrix::AddMult: `mass_->Mult(a, y)`, `viscosity_->AddMult(v, y)` of
 * operators::NonlinearSolid::Mult / ResidualAndGrad, operators/nonlinear_solid.cpp:172-205,240-283).  Host or device. */
int mimi_hip_linear_add_mult(mimi_hip_linear_t h, const double* A_values, const double* x, double alpha, double* y);
/* the `preconditioner` of mimi_hip_linear_gmres / _cg and the `kind` of mimi_hip_linear_apply_preconditioner */
enum mimi_hip_preconditioner {
  MIMI_HIP_PRECOND_NONE = 0,
  MIMI_HIP_PRECOND_JACOBI = 1,       /* the reference's (mfem::DSmoother) */
  MIMI_HIP_PRECOND_KRONECKER = 2,    /* the Kronecker operator below (needs set_kronecker and set_kronecker_coefficients
                                        first; an error otherwise) */
  MIMI_HIP_PRECOND_BLOCK_JACOBI = 3  /* the node-block Jacobi below (needs set_node_block first) */
};
/* The reference's iterative linear solver (py/py_nonlinear_solid.cpp:329-339: mfem::GMRESSolver + mfem::DSmoother,
 * rel 1e-8, abs 1e-12, 300 iterations; kdim <= 0 = mfem's default 50): x = 0 start, left-preconditioned restarted
 * GMRES, modified Gram-Schmidt, stops when the preconditioned residual estimate <= max(rel_tol * ||M b||, abs_tol).
 * A_values / b / x host or device. */
int mimi_hip_linear_gmres(mimi_hip_linear_t h, const double* A_values, const double* b, double* x, double rel_tol,
                          double abs_tol, int max_iter, int kdim, int preconditioner, int32_t* iterations,
                          double* final_norm, int32_t* converged);
/* The mass solve of operators::NonlinearSolid (operators/nonlinear_solid.cpp:39-50,155; .hpp:38-42: mfem::CGSolver +
 * mfem::DSmoother, rel 1e-8, abs 1e-12, 1000 iterations): x = 0 start, preconditioned conjugate gradients, stops when
 * (r, M r) <= max(rel_tol^2 (r0, M r0), abs_tol^2); final_norm = sqrt of that product. */
int mimi_hip_linear_cg(mimi_hip_linear_t h, const double* A_values, const double* b, double* x, double rel_tol,
                       double abs_tol, int max_iter, int preconditioner, int32_t* iterations, double* final_norm,
                       int32_t* converged);
/* Fast-diagonalisation (Kronecker) preconditioner for systems on ONE tensor-product patch in the byVDIM numbering, dof
 * ((i2 n1 + i1) n0 + i0) dim + c (no reference counterpart: the reference has Jacobi only).  Per component c
 *   P_c = mass (x)_d M_d + sum_d stiff[c][d] K_d (x) (M of the other axes),
 * given by the generalised eigenpairs of the 1-D matrices, K_d U_cd = M_d U_cd diag(lambda_cd), U_cd^T M_d U_cd = I:
 *   z = P^-1 r = (U_c0 (x) U_c1 (x) U_c2) D_c (U_c0 (x) U_c1 (x) U_c2)^T r,  D_c = 1 / (mass + sum_d stiff[c][d] lambda_cd[i_d]),
 * then z[ess] = r[ess] on the handle's essential dofs (what EliminateRowCol(DIAG_ONE) leaves of those rows).
 * n_dir[dim]: nodes per axis, prod n_dir * dim must be the handle's n.  U: the matrices U_cd, n_d x n_d row-major,
 * concatenated over [component][axis]; lambda: the vectors lambda_cd concatenated the same way.  A 1-D function that is
 * removed from a component (a Dirichlet face) has a zero row and column in U_cd and a NEGATIVE lambda, which makes the
 * scaling zero there.  Host or device arrays (copied). */
int mimi_hip_linear_set_kronecker(mimi_hip_linear_t h, int32_t dim, const int32_t* n_dir, const double* U,
                                  const double* lambda);
/* mass and stiff[c * dim + d] (host) of the operator above; the scaling array is rebuilt on the device */
int mimi_hip_linear_set_kronecker_coefficients(mimi_hip_linear_t h, double mass_coef, const double* stiff_coef);
/* z = M r with the preconditioner the solvers apply: kind _JACOBI (z = r / diag(A); needs A_values, or NULL with
 * set_operator_diagonal armed and an operator set), _KRONECKER (A_values may be NULL), _BLOCK_JACOBI (A_values, or
 * NULL: the blocks of the operator).  Host or device arrays; z == r is allowed. */
int mimi_hip_linear_apply_preconditioner(mimi_hip_linear_t h, int kind, const double* A_values, const double* r, double* z);
/* A domain handle in place of the matrix: with an operator set, A_values == NULL in mimi_hip_linear_gmres / _cg means
 * "the product is density M + stiffness K(u_lin) + viscosity C of `domain`" (mimi_hip_domain_apply_tangent), eliminated
 * like the matrix: y = mask(A (mask x)) + x[ess].  Stands in for SparseMatrix::Mult on the matrix
 * forms::Nonlinear::AddMultGrad assembled.  A non-null A_values takes the CSR kernels as ever.  Preconditioner ids 0, 2
 * and 3 work with the operator, id 1 (Jacobi) needs the matrix values unless mimi_hip_linear_set_operator_diagonal armed it.  The action runs on the solver's stream; a solve
 * waits once on the event behind the domain's last linearize.  The domain must be on the solver's device and have its n;
 * it must outlive the setting.  domain == NULL clears it. */
int mimi_hip_linear_set_operator(mimi_hip_linear_t h, mimi_hip_domain_t domain, double density, double stiffness, double viscosity);
enum mimi_hip_boundary_operator_kind {
  MIMI_HIP_BOUNDARY_CONTACT = 0,  /* `handle` is a mimi_hip_contact_t */
  MIMI_HIP_BOUNDARY_PRESSURE = 1  /* a mimi_hip_pressure_t */
};
/* A face tangent beside the domain operator (`handle` must be of the `kind` given).  With A_values == NULL the product becomes
 *   y = mask((density M + stiffness K + viscosity C + sum_k factor_k K_face,k) mask x) + x[ess],
 * the terms added in the order they were set (mimi_hip_contact_apply_tangent / mimi_hip_follower_apply_tangent: stands in
 * for SparseMatrix::Mult on the matrix MortarContact::AddBoundaryResidualAndGrad, mortar_contact.cpp:353-421, added to).
 * At most 8 terms; refused without a domain operator, on another device, with another n, beyond the eighth.  Every
 * mimi_hip_linear_set_operator call (domain NULL or not) drops the terms.  The actions run on the solver's stream; a solve
 * waits once on the event behind each handle's last linearize, and is refused when a handle has none.  The handles must
 * outlive the setting. */
int mimi_hip_linear_add_boundary_operator(mimi_hip_linear_t h, int kind, void* handle, double factor);
/* A periodic fold between the solver and its operator handles: the solver's n is the FOLDED size n_nodes_f dim of `fold`,
 * the domain handle and every boundary term have the UNWRAPPED size n_nodes_u dim, and with A_values == NULL the product is
 *   y_f = mask(P^T (density M + stiffness K + viscosity C + sum_k factor_k K_face,k) P (mask x_f)) + x_f[ess]:
 * the kernel in front of the actions expands the masked input into unwrapped scratch the handle owns, the actions run there
 * unchanged, and the kernel behind them adds the copies of every folded node in ascending order (the order of
 * mimi_hip_fold_add's residual, so the bits of folding the unfolded action) -- no pass more than without a fold, no atomics.
 * Refused when the fold is on another device or its folded size is not the solver's n; a solve without matrix values is
 * refused when the fold's folded size is not n or a handle has not the unwrapped size.  With a fold set,
 * mimi_hip_linear_set_operator / _add_boundary_operator expect the unwrapped size.  The fold's tables are read in place: it
 * must outlive the setting.  It survives mimi_hip_linear_set_operator (which goes on dropping the boundary terms only);
 * fold == NULL clears it.  Solves that pass matrix values, and the preconditioners, never see it. */
int mimi_hip_linear_set_operator_fold(mimi_hip_linear_t h, mimi_hip_fold_t fold);
/* y = the eliminated operator product a solve without matrix values applies, y = mask(A (mask x)) + x[ess], folded or not,
 * on the solver's stream: the product alone, for checks.  x and y (n doubles each, different vectors) host or device.
 * Refused without an operator, and where a solve would be (a handle that was never linearised, a wrong size). */
int mimi_hip_linear_operator_mult(mimi_hip_linear_t h, const double* x, double* y);
/* Node-block Jacobi, preconditioner id 3 of mimi_hip_linear_gmres / _cg / _apply_preconditioner (no reference counterpart:
 * the reference has the scalar Jacobi only): z_A = B_A^-1 r_A with B_A the dim x dim block (A,i),(A,j) of node A, which carries
 * the coupling between the components of a control point.  set_node_block says that the handle's n is n_nodes dim in byVDIM
 * order (dim 1 to 3); refused when n % dim != 0.  Id 3 needs it.  With matrix values the blocks are read out of the CSR
 * (positions searched once per pattern; an (A,i),(A,j) entry the pattern lacks counts as zero); with A_values == NULL they come
 * from mimi_hip_domain_tangent_diagonal(block = 1) of the operator's domain with the coefficients of set_operator (the domain's
 * dim must be the block's).  Either way the blocks are eliminated like the matrix (row and column of an essential dof zero,
 * its diagonal 1), inverted per node in closed form on the device once per solve, and applied behind the product.  A block
 * whose determinant is zero or not finite fails the solve; the error names the node. */
int mimi_hip_linear_set_node_block(mimi_hip_linear_t h, int32_t dim);
/* Arms preconditioner id 1 (Jacobi) for solves WITHOUT matrix values: 1 / diag then comes from
 * mimi_hip_domain_tangent_diagonal(block = 0) of the operator's domain with the coefficients of set_operator, essential dofs 1,
 * built once per solve on the solver's stream behind the event wait of the product, and applied inside the kernel behind the
 * actions.  A free dof whose diagonal entry is zero or not finite fails the solve; the error names the dof.  What
 * mfem::DSmoother reads off the assembled matrix (py_nonlinear_solid.cpp:329-339), without it.  Off by default:
 * id 1 with A_values == NULL is then refused ("needs the matrix values").  Solves that pass values never see the setting.
 * With an operator fold the unwrapped diagonal (or, id 3, the unwrapped blocks) is summed over the copies of each folded node
 * in the fold's ascending order: the diagonal of P^T A P whenever no element holds both copies of a node, i.e. when the
 * periodic axis has at least two knot spans; with a single span the cross blocks between the copies are left out.
 * Boundary terms (mimi_hip_linear_add_boundary_operator) contribute nothing to the diagonal or the blocks: for frozen contact
 * and follower pressure the scalar diagonal is identically zero (d m_i / d x_a,i = (e_i x t)_i = 0 in 3-D; m = (t_y, -t_x) in
 * 2-D), so id 1 is exactly the assembled route's Jacobi there; their skew node blocks, the friction action and the
 * consistent-tangent terms are not carried.  Solves converge to the same solution; the preconditioner is weaker. */
int mimi_hip_linear_set_operator_diagonal(mimi_hip_linear_t h, int32_t on);

/* ---- explicit central-difference step with a lumped mass -----------------------------------------------------------
 * Stands in for the reference's CentralDifference = Newmark(beta = 0, gamma = 1/2) step (solvers/ode.hpp:257,
 * ode.cpp:229-250), which solves with the consistent mass; here the mass is the vector m and a step is
 *   predict, the caller's force evaluation at the new x (and the damping force at the new v), correct.
 * Masks, one byte per dof (NULL: none set): fixed (v = 0, x kept) and prescribed (v = prescribed_velocity, a = 0; wins
 * where both are set).  The create arguments may be host or device arrays (copied).  Every vector of the other entries
 * must be device-resident: a host pointer is refused (ode.cpp:229-250 works on the solver's own vectors; a staged copy
 * per step would defeat the step).  Nothing but mimi_hip_explicit_energies and _synchronize waits for the device. */
typedef struct mimi_hip_explicit_s* mimi_hip_explicit_t;
int mimi_hip_explicit_create(int64_t n, const unsigned char* fixed, const unsigned char* prescribed,
                             const double* prescribed_velocity, int device, mimi_hip_explicit_t* out);
int mimi_hip_explicit_destroy(mimi_hip_explicit_t h);
/* NULL = the handle's own stream; MIMI_HIP_STREAM_NULL = the device's null stream.  The launches of one handle must not
 * overlap: the sums of start / correct share the handle's partial-sum buffers and ticket, so a caller that moves the handle
 * to another stream orders that stream behind the work already enqueued (one stream per handle is the intended use). */
int mimi_hip_explicit_set_stream(mimi_hip_explicit_t h, void* stream);
/* waits for the handle's stream and reads its status word: an error when set_mass saw a non-positive mass on a free or
 * prescribed dof */
int mimi_hip_explicit_synchronize(mimi_hip_explicit_t h);
enum mimi_hip_explicit_info_what {
  MIMI_HIP_EXPLICIT_INFO_N = 0,
  MIMI_HIP_EXPLICIT_INFO_R_PREV = 1,   /* the address of the internal force vector of the previous step (the handle keeps
                                          the caller's buffer by pointer: no copy) */
  MIMI_HIP_EXPLICIT_INFO_D_PREV = 2,   /* the same of the damping force vector */
  MIMI_HIP_EXPLICIT_INFO_STEPS = 3,    /* corrects since start */
  /* the shape of the ledger's sums, valid with h == NULL: */
  MIMI_HIP_EXPLICIT_INFO_SUM_BLOCK = 4,       /* threads of a workgroup */
  MIMI_HIP_EXPLICIT_INFO_SUM_GRID_CAP = 5,    /* most workgroups of a launch */
  MIMI_HIP_EXPLICIT_INFO_SUM_FINAL_RUN = 6,   /* partials a thread of the last workgroup adds */
  MIMI_HIP_EXPLICIT_INFO_SUM_TREE_DEPTH = 7,  /* levels of the two trees */
  MIMI_HIP_EXPLICIT_INFO_GRID = 8      /* workgroups of a launch on this handle */
};
/* -1: bad argument */
int64_t mimi_hip_explicit_info(mimi_hip_explicit_t h, int what);
/* the lumped mass (the M of ode.cpp:229-250 as a vector), copied; positive on every free and every prescribed dof (the
 * latter's enters KE), checked on the device; a fixed dof's is not read */
int mimi_hip_explicit_set_mass(mimi_hip_explicit_t h, const double* m);
/* a_0 = ((f - r) - d) / m on free dofs, 0 elsewhere (the initial acceleration of ode.cpp:229-250); the masks are applied
 * to v; r and d become the previous force vectors; the works are zeroed.  f and d may be NULL (no load / no damping). */
int mimi_hip_explicit_start(mimi_hip_explicit_t h, double* v, const double* f, const double* r, const double* d);
/* v <- v + dt/2 a, x <- x + dt v with the masks applied (the predictor of ode.cpp:229-250 at beta = 0, gamma = 1/2) */
int mimi_hip_explicit_predict(mimi_hip_explicit_t h, double dt, double* x, double* v);
/* a <- ((f - r) - d) / m on free dofs, v <- v + dt/2 a (the corrector of ode.cpp:229-250 with the mass solve replaced by
 * the division), and the energy ledger in the same pass (mimi_amd/csrc/explicit.hip).  r: the raw internal force at the
 * new x, d: the damping force at the predictor velocity (NULL iff it was NULL at start).  r and d are read again by the
 * next correct, which must be given other buffers: the caller alternates two and leaves the last one untouched. */
int mimi_hip_explicit_correct(mimi_hip_explicit_t h, double dt, const double* f, const double* r, const double* d, double* v);
/* a (device, n doubles) <- the current acceleration (the d2x/dt2 ode.cpp:229-250 keeps between steps) */
int mimi_hip_explicit_acceleration(mimi_hip_explicit_t h, double* a);
/* out6 (host) = KE, W_int, W_ext, W_damp, Q = dt^2/8 sum m a^2, E* = KE - Q + W_int + W_damp - W_ext: the ledger beside
 * the step of ode.cpp:229-250 (the reference keeps none).  dt: the step size Q is formed with.  Waits for the stream. */
int mimi_hip_explicit_energies(mimi_hip_explicit_t h, double dt, double* out6);

#ifdef __cplusplus
}
#endif
#endif /* MIMI_HIP_H */
