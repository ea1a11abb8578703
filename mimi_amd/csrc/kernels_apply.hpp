// Matrix-free tangent action (include/mimi_hip.h, "tangent action"):
//   y += density M x + stiffness K(u_lin) x + viscosity C x
// over the handle's elements, without a CSR matrix.  M and C are the forms of kernels_forms.hpp with coefficient 1, K the
// tangent the assemblies add with grad_factor 1.  The reference has no counterpart as one routine: inside its GMRES the
// product is SparseMatrix::Mult on the matrix forms::Nonlinear::AddMultGrad assembled; this is that product without the matrix.
//
// What a linearisation leaves (mimi_hip_domain_linearize), by material:
//   neo-Hookean       a device copy of u and nothing per point.  The action recomputes F at the point and takes the
//                     directional derivative in closed form, with G = grad x:
//                       dP[G] = mu G - c1 F^-T G^T F^-T + c2 tr(F^-1 G) F^-T,   c1 = lambda J (J - 1) - mu, c2 = lambda J (2 J - 1)
//                     (tangent_of's neo-Hookean branch contracted with G on paper: three DIM x DIM products instead of the
//                     DIM^4 entries of the tangent routine, which would have to be formed before they are contracted).
//   every other one   the record w det dP/dF, DIM^4 doubles per point, from the routines the assemblies call
//                     (evaluate_pk1 + tangent_row_of for J2, other_tangent_begin / _dir for the rest), stored
//                     rec[entry][point]: lane = point, so a wave reads and writes whole runs of 64 doubles per entry.
//
// One kernel text per route, three MODEs of it:
//   APPLY_NEOHOOKEAN  forward stages on x and u_lin, closed-form dP[G] at the point
//   APPLY_RECORD      forward stages on x, dP[G] = record : G
//   APPLY_LINEARIZE   forward stages on u, the material's tangent at the point into the record; no backward stages
// apply_tensor_kernel   every tensor_usable handle: grad_xi by sum factorisation from the 1-D tables, one parametric direction
//                       per stage through LDS (as field_tensor_kernel), the point values contracted back with the D and B
//                       tables to the element's nodes.  At most 64 points per element: one wave per element, four elements
//                       per 256-thread workgroup; 125 points: two waves per element.  No per-point basis table is read.
// apply_general_kernel  flat tables and mixed degrees: the same from dN_dX, wdet and the shape values.
// Both store element pieces [e][a][DIM]; node_gather_kernel (kernels_fields.hpp) sums them per node over the handle's
// node -> (element, local node) adjacency in the adjacency's order: every (node, component) is written by exactly one
// thread, no atomics, equal inputs give equal bytes.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_fields.hpp"

namespace mimi_hip {

constexpr int APPLY_NEOHOOKEAN = 0, APPLY_RECORD = 1, APPLY_LINEARIZE = 2;

struct ApplyArgs {
  double density, stiffness, viscosity;
  const double* x;       // the vector the action is applied to
  const double* u_lin;   // APPLY_NEOHOOKEAN: the displacement of the linearisation; APPLY_LINEARIZE: the u to linearise at
  double* rec;           // [DIM^4][n_pts]: read by APPLY_RECORD, written by APPLY_LINEARIZE
  double* pieces;        // [n_el][n_dof][DIM]
  const double* N;       // general route, density != 0: shape values [n_el][n_q][n_dof]
  int64_t n_pts;
  int n_el;
};

// G = H dxi/dX (H[i DIM + m] = dx_i / dxi_m; G column-major as F)
template<int DIM>
MH_DEV void physical_gradient(const double* H, const double* Ji, double* G) {
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int J = 0; J < DIM; ++J) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < DIM; ++m) s += H[i * DIM + m] * Ji[m * DIM + J];
      G[i + J * DIM] = s;
    }
}

// dP[G] of the neo-Hookean law at F (both column-major)
template<int DIM>
MH_DEV void neo_hookean_direction(const mimi_hip_material& m, const double* F, const double* G, double* dP) {
  constexpr int DD = DIM * DIM;
  double Fi[DD], T[DD];
  const double J = det_of<DIM>(F);
  inverse_of<DIM>(F, J, Fi);
  const double c1 = m.lambda * J * (J - 1.) - m.mu;
  const double c2 = m.lambda * (2. * J - 1.) * J;
  double tr = 0.0;
  // T = F^-1 G
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) s += MH_M(Fi, a, k) * MH_M(G, k, b);
      MH_M(T, a, b) = s;
      if (a == b) tr += s;
    }
  // dP_iJ = mu G_iJ - c1 (T F^-1)_Ji + c2 tr F^-1_Ji
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int Jx = 0; Jx < DIM; ++Jx) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) s += MH_M(T, Jx, k) * MH_M(Fi, k, i);
      MH_M(dP, i, Jx) = m.mu * MH_M(G, i, Jx) - c1 * s + c2 * tr * MH_M(Fi, Jx, i);
    }
}

// w det dP[G] from the record of point pt
template<int DIM>
MH_DEV void record_direction(const double* __restrict__ rec, int64_t n_pts, int64_t pt, const double* G, double* dP) {
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int Jx = 0; Jx < DIM; ++Jx) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < DIM; ++j)
#pragma unroll
        for (int L = 0; L < DIM; ++L) s += rec[(int64_t)(((i * DIM + Jx) * DIM + j) * DIM + L) * n_pts + pt] * MH_M(G, j, L);
      MH_M(dP, i, Jx) = s;
    }
}

// the record of point pt: w det dP_iJ / dF_jL at entry ((i DIM + J) DIM + j) DIM + L (the layout of tangent_of).
// FAMILY: by_material_family's (0: J2, closed form; 2..5: the other materials, one direction (j, L) at a time)
template<int DIM, int FAMILY>
MH_DEV int record_at_point(const MaterialDev& mat, double dt, const StateView& st, int64_t pt, const double* F, double wd,
                           double* __restrict__ rec, int64_t n_pts) {
  constexpr int DD = DIM * DIM, D3 = DD * DIM;
  int status = 0;
  if constexpr (FAMILY == 0) {
    PointResult<DIM> w;
    status = evaluate_pk1<DIM>(mat, dt, st, pt, F, w);
    double Ar[D3];
    tangent_row_of<DIM, 0>(mat.m, w, Ar);
#pragma unroll
    for (int k = 0; k < D3; ++k) rec[(int64_t)k * n_pts + pt] = wd * Ar[k];
    tangent_row_of<DIM, 1>(mat.m, w, Ar);
#pragma unroll
    for (int k = 0; k < D3; ++k) rec[(int64_t)(D3 + k) * n_pts + pt] = wd * Ar[k];
    if constexpr (DIM == 3) {
      tangent_row_of<DIM, 2>(mat.m, w, Ar);
#pragma unroll
      for (int k = 0; k < D3; ++k) rec[(int64_t)(2 * D3 + k) * n_pts + pt] = wd * Ar[k];
    }
  } else {
    double P[DD];
    OtherTangent<DIM> ot;
    status = other_tangent_begin<DIM, FAMILY>(mat, dt, st, pt, F, P, ot);
#pragma unroll 1
    for (int j = 0; j < DIM; ++j)
#pragma unroll 1
      for (int L = 0; L < DIM; ++L) {
        double dP[DD], Fl[DD];
        // (F through an empty asm per direction, as general_material_kernel: nothing of the dual-number routine is hoisted
        // out of the loop and kept live across the directions)
#pragma unroll
        for (int k = 0; k < DD; ++k) {
          Fl[k] = F[k];
          asm volatile("" : "+v"(Fl[k]));
        }
        other_tangent_dir<DIM, FAMILY>(mat, dt, Fl, ot, j, L, dP);
#pragma unroll
        for (int i = 0; i < DIM; ++i)
#pragma unroll
          for (int Jx = 0; Jx < DIM; ++Jx) rec[(int64_t)(((i * DIM + Jx) * DIM + j) * DIM + L) * n_pts + pt] = wd * MH_M(dP, i, Jx);
      }
  }
  return status;
}

// what a point hands to the backward stages: w det (stiffness dP[G] + viscosity G) and w det density x, DIM (DIM + 1) values
template<int DIM, int MODE>
MH_DEV void action_at_point(const ApplyArgs& aa, const mimi_hip_material& m, int64_t pt, double wd, const double* F, const double* G,
                            const double* xv, double* Hp /* [i + J DIM] */, double* mv) {
  constexpr int DD = DIM * DIM;
#pragma unroll
  for (int k = 0; k < DD; ++k) Hp[k] = wd * aa.viscosity * G[k];
  if (aa.stiffness != 0.0) {
    double dP[DD];
    if constexpr (MODE == APPLY_NEOHOOKEAN) {
      neo_hookean_direction<DIM>(m, F, G, dP);
#pragma unroll
      for (int k = 0; k < DD; ++k) Hp[k] += wd * aa.stiffness * dP[k];
    } else {
      record_direction<DIM>(aa.rec, aa.n_pts, pt, G, dP);
#pragma unroll
      for (int k = 0; k < DD; ++k) Hp[k] += aa.stiffness * dP[k];
    }
  }
#pragma unroll
  for (int i = 0; i < DIM; ++i) mv[i] = wd * aa.density * xv[i];
}

template<int DIM, int P, int MODE>
struct ApplyShape : ElementShape<DIM, P> {
  using E = ElementShape<DIM, P>;
  static constexpr int NB = E::NB, NQ = E::NQ, NBZ = E::NBZ, ND = E::ND, NPT = E::NPT;
  static constexpr int LANES = NPT <= 64 ? 64 : 128;     // threads of one element
  static constexpr int EPW = NPT <= 64 ? 4 : 1;          // elements of one workgroup
  static constexpr int THREADS = LANES * EPW;
  static constexpr int NCF = MODE == APPLY_NEOHOOKEAN ? 2 * DIM : DIM;   // vector components through the forward stages
  static constexpr int NV = DIM * 4;                     // staged point values: per component three gradient slots and one value
  __host__ __device__ static constexpr int cmax(int a, int b) { return a > b ? a : b; }
  // LDS carve of one element, in doubles: the tables, then two regions that the forward and the backward stages use in turn
  //   A: the element's vectors [NCF][ND] and T1 [NCF][2][NB NBZ][NQ]  | G1 [DIM][4][NBZ][NQ NQ]
  //   B: T2 [NCF][3][NBZ][NQ NQ]  | the point values [NV][NPT] (written once every lane has read its T2)  | G2 [DIM][2][NB NBZ][NQ]
  // (degree 2, neo-Hookean: 1530 doubles = 12 KB per wave, twelve waves per CU; three separate areas took 18 KB: eight)
  static constexpr int off_tab = 0;                                       // [3 dir][B, D][NB][NQ]
  static constexpr int off_ue = off_tab + 3 * 2 * NB * NQ;
  static constexpr int off_x = off_ue + NCF * ND;
  static constexpr int off_g1 = off_ue;
  static constexpr int size_a = cmax(NCF * ND + NCF * 2 * NB * NBZ * NQ, DIM * 4 * NBZ * NQ * NQ);
  static constexpr int off_y = off_ue + size_a;
  static constexpr int off_vals = off_y, off_g2 = off_y;
  static constexpr int size_b = cmax(cmax(NCF * 3 * NBZ * NQ * NQ, MODE == APPLY_LINEARIZE ? 0 : NV * NPT), DIM * 2 * NB * NBZ * NQ);
  static constexpr int total = off_y + size_b;
};

// FAMILY: APPLY_LINEARIZE only (the material whose tangent is recorded); the actions do not evaluate a material routine
template<int DIM, int P, int MODE, int FAMILY>
__global__ __launch_bounds__((ApplyShape<DIM, P, MODE>::THREADS)) void apply_tensor_kernel(TensorArgs p, ApplyArgs aa) {
  using S = ApplyShape<DIM, P, MODE>;
  constexpr int NB = S::NB, NQ = S::NQ, NBZ = S::NBZ, NQZ = S::NQZ, ND = S::ND, NPT = S::NPT, DD = S::DD, NT = S::LANES;
  constexpr int NB12 = NB * NBZ, NQ01 = NQ * NQ, TS = NB * NQ, NCF = S::NCF;
  extern __shared__ __align__(16) double smem_apply_tensor[];
  const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
  double* lds = smem_apply_tensor + sub * S::total;
  double* ue = lds + S::off_ue;
  double* tab = lds + S::off_tab;
  double* X = lds + S::off_x;
  double* Y = lds + S::off_y;
  // one wave per element (EPW == 4): the waves of a workgroup share nothing, every barrier is a wave barrier and a wave past
  // the last element leaves; two waves per element (EPW == 1): workgroup barriers, and every workgroup has its element
  const int64_t e = (int64_t)blockIdx.x * S::EPW + sub;
  if (e >= aa.n_el) return;
  constexpr bool active = true;
  auto sync = [] {
    if constexpr (S::EPW == 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
  };
  int el[3];
  element_in_box<DIM>(p, e, el);
  load_element_tables<DIM, P, NT>(p, el, tid, tab);
  for (int a = tid; a < ND; a += NT) {
    const int64_t node = p.dofs[e * ND + a];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      if constexpr (MODE == APPLY_LINEARIZE) {
        ue[c * ND + a] = aa.u_lin[node * DIM + c];
      } else {
        ue[c * ND + a] = aa.x[node * DIM + c];
        if constexpr (MODE == APPLY_NEOHOOKEAN) ue[(DIM + c) * ND + a] = aa.stiffness != 0.0 ? aa.u_lin[node * DIM + c] : 0.0;
      }
    }
  }
  sync();
  // T1 into X, T2 into Y (sum_factor.hpp)
  forward_stages<DIM, P, NCF, NT>(tab, ue, X, Y, tid, sync);

  // ---- quadrature-point stage: lane = point -------------------------------------------------------------------------------
  int status = 0;
  double staged[S::NV];   // what the lane's point hands to the backward stages
  if (tid < NPT) {
    const int q01 = tid % NQ01, q2 = tid / NQ01;
    const PointGeometry<DIM, NPT> geo(p, e, tid);
    const double wd = geo.wdet();
    double Ji[DD];
    geo.Ji(Ji);
    // H of component set 0: x, or u when linearising; set 1: u_lin beside x
    double H[DD];
    parametric_gradient<DIM, P>(tab, Y, 0, q01, q2, H);
    if constexpr (MODE == APPLY_LINEARIZE) {
      double F[DD];
      deformation_gradient<DIM>(H, Ji, F);
      if (active) status = record_at_point<DIM, FAMILY>(p.mat, p.dt, p.state, e * NPT + tid, F, wd, aa.rec, aa.n_pts);
    } else {
      double G[DD], F[DD] = {}, xv[DIM];
      physical_gradient<DIM>(H, Ji, G);
      point_value<DIM, P>(tab, Y, q01, q2, xv);
      if constexpr (MODE == APPLY_NEOHOOKEAN) {
        parametric_gradient<DIM, P>(tab, Y, 1, q01, q2, H);
        deformation_gradient<DIM>(H, Ji, F);
      }
      double Hp[DD], mv[DIM];
      action_at_point<DIM, MODE>(aa, p.mat.m, e * NPT + tid, wd, F, G, xv, Hp, mv);
      // staged[i][m] = sum_J Hp_iJ dxi_m / dX_J (m < DIM), 0 for the direction a 2-D patch lacks, the mass value at m = 3
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          double s = 0.0;
          if (m < DIM) {
#pragma unroll
            for (int Jx = 0; Jx < DIM; ++Jx) s += MH_M(Hp, i, Jx) * Ji[(m < DIM ? m : 0) * DIM + Jx];
          }
          staged[i * 4 + m] = s;
        }
        staged[i * 4 + 3] = mv[i];
      }
    }
  }
  if constexpr (MODE == APPLY_LINEARIZE) {
    if (status) atomicOr(p.status, status);
    return;
  } else {
    // vals[i][m][q] over T2, once every lane of the element has read its part of it
    sync();
    double* vals = lds + S::off_vals;
    double* G1 = lds + S::off_g1;
    double* G2 = lds + S::off_g2;
    if (tid < NPT) {
#pragma unroll
      for (int v = 0; v < S::NV; ++v) vals[v * NPT + tid] = staged[v];
    }
    sync();
    // ---- back to the nodes, one direction at a time ---------------------------------------------------------------------
    // G1[i][k][a2][q01] = sum_q2 (k == 2 ? D2 : B2)[a2][q2] vals[i][k][q01 + NQ^2 q2]
    for (int t = tid; t < DIM * 4 * NBZ * NQ01; t += NT) {
      const int q01 = t % NQ01, a2 = (t / NQ01) % NBZ, ik = t / (NQ01 * NBZ), k = ik % 4;
      const double* tb = tab + (4 + (k == 2 ? 1 : 0)) * TS + a2 * NQ;
      double s = 0.0;
#pragma unroll
      for (int q2 = 0; q2 < NQZ; ++q2) s += tb[q2] * vals[ik * NPT + q01 + NQ01 * q2];
      G1[t] = s;
    }
    sync();
    // G2[i][0][a12][q0] = sum_q1 B1[a1][q1] G1[i][0][a2][q0 + NQ q1]                              (D0 still to come)
    // G2[i][1][a12][q0] = sum_q1 D1[a1][q1] G1[i][1][..] + B1[a1][q1] (G1[i][2][..] + G1[i][3][..])   (B0 still to come)
    for (int t = tid; t < DIM * 2 * NB12 * NQ; t += NT) {
      const int q0 = t % NQ, a12 = (t / NQ) % NB12, a1 = a12 % NB, a2 = a12 / NB, s01 = (t / (NQ * NB12)) % 2, i = t / (NQ * NB12 * 2);
      const double* tbB = tab + 2 * TS + a1 * NQ;
      const double* tbD = tab + 3 * TS + a1 * NQ;
      const double* g1 = G1 + ((i * 4) * NBZ + a2) * NQ01 + q0;
      constexpr int KS = NBZ * NQ01;   // stride between the kinds of G1
      double s = 0.0;
      if (s01 == 0) {
#pragma unroll
        for (int q1 = 0; q1 < NQ; ++q1) s += tbB[q1] * g1[NQ * q1];
      } else {
#pragma unroll
        for (int q1 = 0; q1 < NQ; ++q1) s += tbD[q1] * g1[KS + NQ * q1] + tbB[q1] * (g1[2 * KS + NQ * q1] + g1[3 * KS + NQ * q1]);
      }
      G2[t] = s;
    }
    sync();
    // pieces[e][a0 + NB a12][i] = sum_q0 D0[a0][q0] G2[i][0][a12][q0] + B0[a0][q0] G2[i][1][a12][q0]
    if (active) {
      double* out = aa.pieces + e * (int64_t)(ND * DIM);
      for (int t = tid; t < ND * DIM; t += NT) {
        const int i = t % DIM, a = t / DIM, a0 = a % NB, a12 = a / NB;
        const double* tbB = tab + a0 * NQ;
        const double* tbD = tab + TS + a0 * NQ;
        const double* g2 = G2 + ((i * 2) * NB12 + a12) * NQ;
        double s = 0.0;
#pragma unroll
        for (int q0 = 0; q0 < NQ; ++q0) s += tbD[q0] * g2[q0] + tbB[q0] * g2[NB12 * NQ + q0];
        out[t] = s;
      }
    }
  }
}

// dx_i / dX_J = sum_a v_ai dN_a / dX_J from the flat tables (column-major, no identity added)
template<int DIM>
MH_DEV void gradient_general(int n_dof, const double* __restrict__ g /* [DIM][n_dof] */, const double* v_e /* LDS [DIM][n_dof] */, double* G) {
#pragma unroll
  for (int k = 0; k < DIM * DIM; ++k) G[k] = 0.0;
  for (int a = 0; a < n_dof; ++a) {
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int J = 0; J < DIM; ++J) MH_M(G, i, J) += v_e[i * n_dof + a] * g[J * n_dof + a];
  }
}

// dynamic LDS: x_e [DIM][n_dof], u_e [DIM][n_dof], then the staged point values [n_q][DIM (DIM + 1)]
template<int DIM, int MODE, int FAMILY>
__global__ __launch_bounds__(256) void apply_general_kernel(GeneralArgs p, ApplyArgs aa) {
  constexpr int DD = DIM * DIM, NV = DIM * (DIM + 1);
  extern __shared__ __align__(16) unsigned char smem_apply_general[];
  const int64_t e = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_dof = p.n_dof, n_q = p.n_q, n_tdof = n_dof * DIM;
  double* x_e = reinterpret_cast<double*>(smem_apply_general);
  double* u_e = x_e + n_tdof;
  double* vals = u_e + n_tdof;
  const bool need_u = MODE == APPLY_LINEARIZE || (MODE == APPLY_NEOHOOKEAN && aa.stiffness != 0.0);
  if constexpr (MODE != APPLY_LINEARIZE) gather_element_vector<DIM>(p.dofs, e, n_dof, aa.x, x_e, tid, blockDim.x);
  gather_element_vector<DIM>(p.dofs, e, n_dof, need_u ? aa.u_lin : nullptr, u_e, tid, blockDim.x);
  __syncthreads();
  int status = 0;
  for (int q = tid; q < n_q; q += blockDim.x) {
    const int64_t pt = e * n_q + q;
    const double* g = p.dN_dX + pt * n_tdof;
    const double wd = p.wdet[pt];
    double F[DD] = {};
    if constexpr (MODE != APPLY_RECORD) compute_F_general<DIM>(n_dof, g, u_e, F);
    if constexpr (MODE == APPLY_LINEARIZE) {
      status |= record_at_point<DIM, FAMILY>(p.mat, p.dt, p.state, pt, F, wd, aa.rec, aa.n_pts);
    } else {
      double G[DD], xv[DIM], Hp[DD], mv[DIM];
      gradient_general<DIM>(n_dof, g, x_e, G);
#pragma unroll
      for (int i = 0; i < DIM; ++i) xv[i] = 0.0;
      if (aa.density != 0.0) {
        const double* Nq = aa.N + pt * n_dof;
        for (int a = 0; a < n_dof; ++a) {
#pragma unroll
          for (int i = 0; i < DIM; ++i) xv[i] += Nq[a] * x_e[i * n_dof + a];
        }
      }
      action_at_point<DIM, MODE>(aa, p.mat.m, pt, wd, F, G, xv, Hp, mv);
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
#pragma unroll
        for (int J = 0; J < DIM; ++J) vals[q * NV + i * (DIM + 1) + J] = MH_M(Hp, i, J);
        vals[q * NV + i * (DIM + 1) + DIM] = mv[i];
      }
    }
  }
  if constexpr (MODE == APPLY_LINEARIZE) {
    if (status) atomicOr(p.status, status);
    return;
  } else {
    __syncthreads();
    // pieces[e][a][i] = sum_q sum_J dN_a/dX_J Hp_iJ + N_a mv_i
    double* out = aa.pieces + e * (int64_t)n_tdof;
    const double* gE = p.dN_dX + e * (int64_t)n_q * n_tdof;
    const double* Ne = aa.density != 0.0 ? aa.N + e * (int64_t)n_q * n_dof : nullptr;
    for (int t = tid; t < n_tdof; t += blockDim.x) {
      const int i = t % DIM, a = t / DIM;
      double s = 0.0;
      for (int q = 0; q < n_q; ++q) {
        const double* g = gE + (int64_t)q * n_tdof;
        const double* v = vals + q * NV + i * (DIM + 1);
#pragma unroll
        for (int J = 0; J < DIM; ++J) s += g[J * n_dof + a] * v[J];
        if (Ne) s += Ne[(int64_t)q * n_dof + a] * v[DIM];
      }
      out[t] = s;
    }
  }
}

}  // namespace mimi_hip
