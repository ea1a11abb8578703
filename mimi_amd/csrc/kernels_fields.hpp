// Field output (include/mimi_hip.h, "field output"): Cauchy stress, von Mises stress, det F and the committed scalar state at
// the quadrature points, and their lumped L2 projection onto the nodes
//   sum[A][c] += sum_e sum_q w_q det_q N_A(q) f_c(q),   weight[A] += sum_e sum_q w_q det_q N_A(q).
// The reference stores none of this (its outputs are x_ / v_ vectors); the quantities are its own: P of
// NonlinearSolid::QuadLoop (integrators/nonlinear_solid.hpp:65-87) through the same device functions as the assemblies
// (materials.hpp, materials_other.hpp), sigma = P F^T / det F, and the deviator of material_utils.hpp:33,44, which takes
// the trace over dim -- in 3-D the usual von Mises stress, in 2-D the q of the reference's own yield function.
//
// Two element kernels, one workgroup per element and one lane per point in both:
//   field_tensor_kernel   every tensor_usable patch handle.  H = sum_a u_a dN_a/dxi by sum factorisation from the 1-D tables
//                         (one parametric direction at a time, through LDS), F = I + H dxi/dX from the 10 (5 in 2-D) doubles
//                         of geometry per point the handle holds; for the nodal form w det f_c and w det are contracted back
//                         with the B tables, one direction at a time, to the element's (p + 1)^dim nodes.  No per-point
//                         basis table is read or built.
//   field_general_kernel  flat-table handles and patch handles on the general path: F from dN_dX, the nodal form with the
//                         shape values N[e][q][a] (the caller's, or expanded from the 1-D tables next to dN_dX).
// Point form: out[e][q][c], stored through LDS so that a workgroup writes its element's values as one contiguous run.
// Nodal form, no atomics: the element kernel stores pieces[e][a][ncomp + 1] (the last one is the weight), and
// node_gather_kernel sums them per node over the handle's node -> (element, local node) adjacency, in the adjacency's
// order -- every (node, component) is written by exactly one thread, so two calls give the same bytes.  The same gather
// serves the body force (the weight alone) and the tangent action (kernels_apply.hpp: DIM components, no weight).
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_general.hpp"
#include "kernels_setup.hpp"
#include "sum_factor.hpp"

namespace mimi_hip {

struct FieldArgs {
  int field;         // mimi_hip_field
  int ncomp;         // its components
  int nodal;         // 0: out = point values [e][q][ncomp]; 1: out = element pieces [e][a][ncomp + 1]
  int need_F;        // the field depends on u (fields 0..2)
  double* out;
  const double* N;   // general kernel, nodal form: [n_el][n_q][n_dof]
};

inline int field_components(int field, int dim) {
  if (field == MIMI_HIP_FIELD_CAUCHY) return dim * dim;
  return (field >= MIMI_HIP_FIELD_VON_MISES && field <= MIMI_HIP_FIELD_TEMPERATURE) ? 1 : -1;
}

// FAMILY of the field kernels: by_material_family's (0: J2 here, 2..5 the other materials), and neo-Hookean on its own -- behind
// one switch with J2 it would carry J2's 174 registers (2 waves per SIMD) through a kernel that is bound by its reads
constexpr int FIELD_NEOHOOKEAN = -1;

// the field at one quadrature point, f[0 .. ncomp); the state is read, never written
template<int DIM, int FAMILY>
MH_DEV int field_at_point(const MaterialDev& mat, double dt, const StateView& st, int64_t pt, int field, const double* F, double* f) {
  constexpr int DD = DIM * DIM;
  if (field == MIMI_HIP_FIELD_EQPS) {
    f[0] = st.eqps[pt];
    return 0;
  }
  if (field == MIMI_HIP_FIELD_TEMPERATURE) {
    f[0] = st.temperature[pt];
    return 0;
  }
  const double J = det_of<DIM>(F);
  if (field == MIMI_HIP_FIELD_DET_F) {
    f[0] = J;
    return 0;
  }
  int status = 0;
  double Pk[DD];
  if constexpr (FAMILY == FIELD_NEOHOOKEAN) {
    PointResult<DIM> w;
    neo_hookean_stress<DIM>(mat.m, F, w);     // (what evaluate_pk1 runs for this kind, without J2's registers)
#pragma unroll
    for (int k = 0; k < DD; ++k) Pk[k] = w.P[k];
  } else if constexpr (FAMILY != 0) {
    status = evaluate_other<DIM, FAMILY>(mat, dt, st, pt, F, Pk, nullptr, 1.0);
  } else {
    PointResult<DIM> w;
    status = evaluate_pk1<DIM>(mat, dt, st, pt, F, w);
#pragma unroll
    for (int k = 0; k < DD; ++k) Pk[k] = w.P[k];
  }
  // sigma = P F^T / det F
  double sig[DD];
  const double over_J = 1.0 / J;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      double s = 0.0;
#pragma unroll
      for (int K = 0; K < DIM; ++K) s += MH_M(Pk, i, K) * MH_M(F, j, K);
      MH_M(sig, i, j) = s * over_J;
    }
  if (field == MIMI_HIP_FIELD_CAUCHY) {
#pragma unroll
    for (int k = 0; k < DD; ++k) f[k] = sig[k];
    return status;
  }
  // von Mises: sqrt(3/2) || sigma - tr(sigma) / DIM I ||_F
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) tr += MH_M(sig, i, i);
  tr /= (double)DIM;
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      const double d = MH_M(sig, i, j) - (i == j ? tr : 0.0);
      n2 += d * d;
    }
  f[0] = sqrt(1.5) * sqrt(n2);
  return status;
}

// what a lane leaves in LDS for its point: the point form [q][ncomp] (the order of `out`), the nodal form [c][NPT] with
// w det f_c and, at c = ncomp, w det
template<int DD>
MH_DEV void field_stage_point(const FieldArgs& fa, const double* f, double wd, int q, int npt, double* vals) {
  if (fa.nodal) {
#pragma unroll
    for (int c = 0; c < DD; ++c)
      if (c < fa.ncomp) vals[c * npt + q] = wd * f[c];
    vals[fa.ncomp * npt + q] = wd;
  } else {
#pragma unroll
    for (int c = 0; c < DD; ++c)
      if (c < fa.ncomp) vals[q * fa.ncomp + c] = f[c];
  }
}

template<int DIM, int P>
struct FieldShape : ElementShape<DIM, P> {
  using E = ElementShape<DIM, P>;
  static constexpr int NB = E::NB, NQ = E::NQ, NBZ = E::NBZ, ND = E::ND, NPT = E::NPT;
  static constexpr int THREADS = NPT <= 64 ? 64 : 128;
  __host__ __device__ static constexpr int cmax(int a, int b) { return a > b ? a : b; }
  // LDS carve, in doubles, for a field of nc = ncomp + 1 staged values per point (dynamic: a scalar field leaves room for
  // five waves per SIMD where the Cauchy stress's carve allows three).  X and Y hold the forward stages, then (dead by then)
  // the backward ones
  static constexpr int off_ue = 0;                                   // [DIM][ND]
  static constexpr int off_tab = off_ue + DIM * ND;                  // [3 dir][B, D][NB][NQ]
  static constexpr int off_x = off_tab + 3 * 2 * NB * NQ;            // T1 [DIM][2][NB NBZ][NQ]      | G2 [nc][NB NBZ][NQ]
  __host__ __device__ static constexpr int off_y(int nc) { return off_x + cmax(DIM * 2, nc) * NB * NBZ * NQ; }   // T2 [DIM][3][NBZ][NQ NQ] | G1 [nc][NBZ][NQ NQ]
  __host__ __device__ static constexpr int off_vals(int nc) { return off_y(nc) + cmax(DIM * 3, nc) * NBZ * NQ * NQ; }
  __host__ __device__ static constexpr int total(int nc) { return off_vals(nc) + nc * NPT; }
};

template<int DIM, int P, int FAMILY>
__global__ __launch_bounds__((FieldShape<DIM, P>::THREADS)) void field_tensor_kernel(TensorArgs p, FieldArgs fa) {
  using S = FieldShape<DIM, P>;
  constexpr int NB = S::NB, NQ = S::NQ, NBZ = S::NBZ, NQZ = S::NQZ, ND = S::ND, NPT = S::NPT, DD = S::DD, NT = S::THREADS;
  constexpr int NB12 = NB * NBZ, NQ01 = NQ * NQ, TS = NB * NQ;
  extern __shared__ __align__(16) double smem_field_tensor[];
  double* lds = smem_field_tensor;
  double* ue = lds + S::off_ue;
  double* tab = lds + S::off_tab;
  double* X = lds + S::off_x;
  double* Y = lds + S::off_y(fa.ncomp + 1);
  double* vals = lds + S::off_vals(fa.ncomp + 1);
  const int tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  int el[3];
  element_in_box<DIM>(p, e, el);
  load_element_tables<DIM, P, NT>(p, el, tid, tab);
  if (fa.need_F) {
    for (int a = tid; a < ND; a += NT) gather_element_u<DIM, ND>(p, e, a, ue);
  }
  __syncthreads();
  // T1 into X, T2 into Y (sum_factor.hpp)
  if (fa.need_F) forward_stages<DIM, P, DIM, NT>(tab, ue, X, Y, tid, [] { __syncthreads(); });

  // ---- quadrature-point stage: lane = point -----------------------------------------------------------------------------
  int status = 0;
  if (tid < NPT) {
    const int q01 = tid % NQ01, q2 = tid / NQ01;
    const PointGeometry<DIM, NPT> geo(p, e, tid);
    const double wd = geo.wdet();
    double F[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) F[k] = 0.0;
    if (fa.need_F) {
      double H[DD];
      parametric_gradient<DIM, P>(tab, Y, 0, q01, q2, H);
      double Ji[DD];
      geo.Ji(Ji);
      deformation_gradient<DIM>(H, Ji, F);
    }
    double f[DD];
    status = field_at_point<DIM, FAMILY>(p.mat, p.dt, p.state, e * NPT + tid, fa.field, F, f);
    field_stage_point<DD>(fa, f, wd, tid, NPT, vals);
  }
  if (status) atomicOr(p.status, status);
  __syncthreads();

  if (!fa.nodal) {
    const int n = NPT * fa.ncomp;
    double* out = fa.out + e * (int64_t)n;
    for (int t = tid; t < n; t += NT) out[t] = vals[t];
    return;
  }
  // ---- back to the nodes, one direction at a time -----------------------------------------------------------------------
  const int NC = fa.ncomp + 1;
  // G1[c][a2][q01] = sum_q2 B2[a2][q2] vals[c][q01 + NQ^2 q2]
  for (int t = tid; t < NC * NBZ * NQ01; t += NT) {
    const int q01 = t % NQ01, a2 = (t / NQ01) % NBZ, c = t / (NQ01 * NBZ);
    const double* tb = tab + 4 * TS + a2 * NQ;
    double s = 0.0;
#pragma unroll
    for (int q2 = 0; q2 < NQZ; ++q2) s += tb[q2] * vals[c * NPT + q01 + NQ01 * q2];
    Y[t] = s;
  }
  __syncthreads();
  // G2[c][a1 + NB a2][q0] = sum_q1 B1[a1][q1] G1[c][a2][q0 + NQ q1]
  for (int t = tid; t < NC * NB12 * NQ; t += NT) {
    const int q0 = t % NQ, a12 = (t / NQ) % NB12, a1 = a12 % NB, a2 = a12 / NB, c = t / (NQ * NB12);
    const double* tb = tab + 2 * TS + a1 * NQ;
    const double* g1 = Y + (c * NBZ + a2) * NQ01 + q0;
    double s = 0.0;
#pragma unroll
    for (int q1 = 0; q1 < NQ; ++q1) s += tb[q1] * g1[NQ * q1];
    X[t] = s;
  }
  __syncthreads();
  // pieces[e][a0 + NB a12][c] = sum_q0 B0[a0][q0] G2[c][a12][q0]
  double* out = fa.out + e * (int64_t)(ND * NC);
  for (int t = tid; t < ND * NC; t += NT) {
    const int c = t % NC, a = t / NC, a0 = a % NB, a12 = a / NB;
    const double* tb = tab + a0 * NQ;
    const double* g2 = X + (c * NB12 + a12) * NQ;
    double s = 0.0;
#pragma unroll
    for (int q0 = 0; q0 < NQ; ++q0) s += tb[q0] * g2[q0];
    out[t] = s;
  }
}

// dynamic LDS: u_e [DIM][n_dof], then the staged point values [(DIM^2 + 1) n_q]
template<int DIM, int FAMILY>
__global__ __launch_bounds__(256) void field_general_kernel(GeneralArgs p, FieldArgs fa) {
  constexpr int DD = DIM * DIM;
  extern __shared__ __align__(16) unsigned char smem_field[];
  const int64_t e = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_dof = p.n_dof, n_q = p.n_q, n_tdof = n_dof * DIM;
  double* u_e = reinterpret_cast<double*>(smem_field);
  double* vals = u_e + n_tdof;
  if (fa.need_F) gather_element_vector<DIM>(p.dofs, e, n_dof, p.u, u_e, tid, blockDim.x);
  __syncthreads();
  int status = 0;
  for (int q = tid; q < n_q; q += blockDim.x) {
    const int64_t pt = e * n_q + q;
    double F[DD], f[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) F[k] = 0.0;
    if (fa.need_F) compute_F_general<DIM>(n_dof, p.dN_dX + pt * n_tdof, u_e, F);
    status |= field_at_point<DIM, FAMILY>(p.mat, p.dt, p.state, pt, fa.field, F, f);
    field_stage_point<DD>(fa, f, p.wdet[pt], q, n_q, vals);
  }
  if (status) atomicOr(p.status, status);
  __syncthreads();
  if (!fa.nodal) {
    const int n = n_q * fa.ncomp;
    double* out = fa.out + e * (int64_t)n;
    for (int t = tid; t < n; t += blockDim.x) out[t] = vals[t];
    return;
  }
  const int NC = fa.ncomp + 1;
  const double* Ne = fa.N + e * (int64_t)n_q * n_dof;
  double* out = fa.out + e * (int64_t)(n_dof * NC);
  for (int t = tid; t < n_dof * NC; t += blockDim.x) {
    const int c = t % NC, a = t / NC;
    double s = 0.0;
    for (int q = 0; q < n_q; ++q) s += Ne[(int64_t)q * n_dof + a] * vals[c * n_q + q];
    out[t] = s;
  }
}

// one thread per (node, column < stride) of the element pieces [e][a][stride]: the pieces of the elements around the node,
// in the adjacency's order ((element << 6) | local node).  Column c < ncomp adds into sum[node][c]; column ncomp (there
// is one when stride == ncomp + 1) into weight[node], when a weight is given
__global__ __launch_bounds__(256) void node_gather_kernel(int64_t n_nodes, int n_dof, int stride, int ncomp, const int64_t* __restrict__ adj_ptr,
                                                          const int32_t* __restrict__ adj, const double* __restrict__ pieces,
                                                          double* __restrict__ sum, double* __restrict__ weight) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_nodes * stride) return;
  const int64_t node = idx / stride;
  const int c = (int)(idx % stride);
  if (c == ncomp && !weight) return;
  const int64_t a_beg = adj_ptr[node], a_end = adj_ptr[node + 1];
  if (a_beg == a_end) return;   // no element of this handle touches the node (element boxes)
  double s = 0.0;
  for (int64_t t = a_beg; t < a_end; ++t) {
    const int32_t ea = adj[t];
    s += pieces[((int64_t)(ea >> 6) * n_dof + (ea & 63)) * stride + c];
  }
  if (c < ncomp) sum[node * ncomp + c] += s;
  else weight[node] += s;
}

// N[e][q][a] of a patch handle from its 1-D tables (QuadData::N, precomputed.hpp:58-71): the general route's nodal form
template<int DIM>
__global__ void expand_shape_kernel(PatchDev P, double* __restrict__ N) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)P.n_el * P.n_q * P.n_dof) return;
  const int a = idx % P.n_dof;
  const int q = (idx / P.n_dof) % P.n_q;
  const int e = idx / ((int64_t)P.n_dof * P.n_q);
  int el[3] = {0, 0, 0}, qi[3] = {0, 0, 0}, al[3] = {0, 0, 0};
  int bn[3] = {P.box_n[0], P.box_n[1], DIM == 3 ? P.box_n[2] : 1};
  int nq[3] = {P.nq[0], P.nq[1], DIM == 3 ? P.nq[2] : 1};
  int np[3] = {P.p[0] + 1, P.p[1] + 1, DIM == 3 ? P.p[2] + 1 : 1};
  split3(e, bn, el);
  split3(q, nq, qi);
  split3(a, np, al);
  double v = 1.0;
  for (int d = 0; d < DIM; ++d) v *= P.B[d][((size_t)(P.box_begin[d] + el[d]) * (P.p[d] + 1) + al[d]) * P.nq[d] + qi[d]];
  N[idx] = v;
}

}  // namespace mimi_hip
