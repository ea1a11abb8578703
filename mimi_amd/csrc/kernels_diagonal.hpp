// Node-block diagonal of the matrix-free tangent (include/mimi_hip.h, "tangent diagonal"): for a control point A with local
// index a in element e
//   D[A][i][j] = sum_{e of A} sum_q w_q det_q [ (density N_a^2 + viscosity |grad_X N_a|^2) delta_ij
//                                               + stiffness d_J N_a (dP_iJ / dF_jL)(q) d_L N_a ]
// -- the (A, i), (A, j) entries of what AddMass, AddDiffusion and AddDomainResidualAndGrad(grad_factor = stiffness) assemble,
// without the matrix: the diagonal of the operator kernels_apply.hpp applies.  block: all DIM^2 entries [A][i][j]; otherwise
// the DIM entries i == j alone (the work for i != j is skipped; the entries i == j run through the same instructions in both
// modes, so the diagonal of the blocks and the diagonal-only mode agree to the bit).
//
// Tangent source, as the action (kernels_apply.hpp):
//   neo-Hookean       F recomputed from the device copy of u that the linearisation left; the block in closed form, from
//                     neo_hookean_direction with G = e_j (x) grad_X N_a and c2 - c1 = lambda J^2 + mu:
//                       w det [ mu |grad_X N_a|^2 delta_ij + (lambda J^2 + mu) (grad_x N_a)_i (grad_x N_a)_j ],  grad_x = F^-T grad_X
//   every other one   the record rec[entry][point] = w det dP_iJ / dF_jL of the linearisation.
//
// diagonal_tensor_kernel   every tensor_usable handle.  With d_m = dN_a / dxi_m every term is a quadratic form
//                          sum_mn d_m S^ij_mn(q) d_n: S is the point's coefficient pulled back with dxi/dX and summed over
//                          (m, n) and (n, m).  N_a = B0 B1 B2 and d_m replaces B by D on axis m, so the products d_m d_n (and
//                          N_a^2 of the mass term) factorise per axis into D D, B D or B B of the element's 1-D table block:
//                          three product tables per axis in LDS, seven kinds of point coefficient (four in 2-D)
//                            kind          00  11  01  mass  22  02  12
//                            axis 0 table  DD  BB  BD  BB    BB  BD  BB
//                            axis 1 table  BB  DD  BD  BB    BB  BB  BD
//                            axis 2 table  BB  BB  BB  BB    DD  BD  BD
//                          contracted back one direction at a time, in the reverse order of forward_stages: axis 2 per kind,
//                          axis 1 into the three sums that share their axis-0 table, axis 0 to the node.  One component (i, j)
//                          at a time through the same LDS.  The workgroup shape of the action: one wave per element up to 64
//                          points, four elements per 256-thread workgroup; two waves per element at 125 points.  No per-point
//                          basis table is read.
// diagonal_general_kernel  flat tables and mixed degrees: the direct sum from dN_dX, w det and the shape values.
// Both store element pieces [e][a][ncomp]; node_gather_kernel (kernels_fields.hpp) sums them per node in the adjacency's
// order: no atomics, equal inputs give equal bytes, element boxes compose by addition.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_apply.hpp"

namespace mimi_hip {

struct DiagonalArgs {
  double density, stiffness, viscosity;
  const double* u_lin;   // APPLY_NEOHOOKEAN: the displacement of the linearisation
  const double* rec;     // APPLY_RECORD: [DIM^4][n_pts]
  double* pieces;        // [n_el][n_dof][ncomp]
  const double* N;       // general route, density != 0: shape values [n_el][n_q][n_dof]
  int64_t n_pts;
  int n_el;
  int block;             // ncomp = block ? DIM^2 : DIM
};

// the 1-D table kind (0: D D, 1: B D, 2: B B) of coefficient kind k on `axis`, from the table of the header comment
MH_DEV constexpr int diagonal_table_of(int axis, int k) {
  constexpr int code[3] = {
      0 | 2 << 2 | 1 << 4 | 2 << 6 | 2 << 8 | 1 << 10 | 2 << 12,
      2 | 0 << 2 | 1 << 4 | 2 << 6 | 2 << 8 | 2 << 10 | 1 << 12,
      2 | 2 << 2 | 2 << 4 | 2 << 6 | 0 << 8 | 1 << 10 | 1 << 12,
  };
  return (code[axis] >> (2 * k)) & 3;
}

template<int DIM, int P, int MODE>
struct DiagonalShape : ElementShape<DIM, P> {
  using E = ElementShape<DIM, P>;
  static constexpr int NB = E::NB, NQ = E::NQ, NBZ = E::NBZ, ND = E::ND, NPT = E::NPT;
  static constexpr int LANES = NPT <= 64 ? 64 : 128;     // threads of one element
  static constexpr int EPW = NPT <= 64 ? 4 : 1;          // elements of one workgroup
  static constexpr int THREADS = LANES * EPW;
  static constexpr int NK = DIM == 3 ? 7 : 4;            // kinds of point coefficient
  __host__ __device__ static constexpr int cmax(int a, int b) { return a > b ? a : b; }
  // LDS carve of one element, in doubles: the tables, the product tables, then one region that the forward stages
  // (neo-Hookean: F of u_lin) and the backward stages use in turn
  static constexpr int off_tab = 0;                                       // [3 dir][B, D][NB][NQ]
  static constexpr int off_prod = off_tab + 3 * 2 * NB * NQ;              // [3 dir][DD, BD, BB][NB][NQ]
  static constexpr int off_work = off_prod + 3 * 3 * NB * NQ;
  static constexpr int off_ue = off_work;                                 // [DIM][ND]
  static constexpr int off_x = off_ue + DIM * ND;                         // T1 [DIM][2][NB NBZ][NQ]
  static constexpr int off_y = off_x + DIM * 2 * NB * NBZ * NQ;           // T2 [DIM][3][NBZ][NQ NQ]
  static constexpr int size_fwd = MODE == APPLY_NEOHOOKEAN ? DIM * ND + DIM * 2 * NB * NBZ * NQ + DIM * 3 * NBZ * NQ * NQ : 0;
  static constexpr int off_vals = off_work;                               // [NK][NPT]
  static constexpr int off_g1 = off_vals + NK * NPT;                      // [NK][NBZ][NQ NQ]
  static constexpr int off_g2 = off_g1 + NK * NBZ * NQ * NQ;              // [3][NB NBZ][NQ]
  static constexpr int size_bwd = NK * NPT + NK * NBZ * NQ * NQ + 3 * NB * NBZ * NQ;
  static constexpr int total = off_work + cmax(size_fwd, size_bwd);
};

template<int DIM, int P, int MODE>
__global__ __launch_bounds__((DiagonalShape<DIM, P, MODE>::THREADS)) void diagonal_tensor_kernel(TensorArgs p, DiagonalArgs da) {
  using S = DiagonalShape<DIM, P, MODE>;
  constexpr int NB = S::NB, NQ = S::NQ, NBZ = S::NBZ, NQZ = S::NQZ, ND = S::ND, NPT = S::NPT, DD = S::DD, NT = S::LANES, NK = S::NK;
  constexpr int NB12 = NB * NBZ, NQ01 = NQ * NQ, TS = NB * NQ;
  extern __shared__ __align__(16) double smem_diagonal_tensor[];
  const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
  double* lds = smem_diagonal_tensor + sub * S::total;
  double* tab = lds + S::off_tab;
  double* prod = lds + S::off_prod;
  // (the barriers and the early exit of apply_tensor_kernel)
  const int64_t e = (int64_t)blockIdx.x * S::EPW + sub;
  if (e >= da.n_el) return;
  auto sync = [] {
    if constexpr (S::EPW == 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
  };
  int el[3];
  element_in_box<DIM>(p, e, el);
  load_element_tables<DIM, P, NT>(p, el, tid, tab);
  const bool stiff = da.stiffness != 0.0;
  if constexpr (MODE == APPLY_NEOHOOKEAN) {
    if (stiff) {
      double* ue = lds + S::off_ue;
      for (int a = tid; a < ND; a += NT) {
        const int64_t node = p.dofs[e * ND + a];
#pragma unroll
        for (int c = 0; c < DIM; ++c) ue[c * ND + a] = da.u_lin[node * DIM + c];
      }
    }
  }
  sync();
  // prod[dir][0][a][q] = D D, [1] = B D, [2] = B B
  for (int t = tid; t < 3 * 3 * TS; t += NT) {
    const int k = t % TS, kind = (t / TS) % 3, dir = t / (3 * TS);
    const double b = tab[(2 * dir) * TS + k], d = tab[(2 * dir + 1) * TS + k];
    prod[t] = kind == 0 ? d * d : kind == 1 ? b * d : b * b;
  }
  if constexpr (MODE == APPLY_NEOHOOKEAN) {
    if (stiff) forward_stages<DIM, P, DIM, NT>(tab, lds + S::off_ue, lds + S::off_x, lds + S::off_y, tid, sync);
  }

  // ---- quadrature-point stage: lane = point; what the lane keeps for the components --------------------------------------
  double wd = 0.0, c21 = 0.0;
  double Ji[DD] = {}, W[DD] = {}, K[DD] = {};   // W[m + i DIM] = sum_J dxi_m/dX_J F^-1_Ji;  K[m + n DIM] = sum_J dxi_m/dX_J dxi_n/dX_J
  const int64_t pt = e * NPT + tid;
  if (tid < NPT) {
    const PointGeometry<DIM, NPT> geo(p, e, tid);
    wd = geo.wdet();
    geo.Ji(Ji);
#pragma unroll
    for (int m = 0; m < DIM; ++m)
#pragma unroll
      for (int n = 0; n < DIM; ++n) {
        double s = 0.0;
#pragma unroll
        for (int J = 0; J < DIM; ++J) s += Ji[m * DIM + J] * Ji[n * DIM + J];
        K[m + n * DIM] = s;
      }
    if constexpr (MODE == APPLY_NEOHOOKEAN) {
      if (stiff) {
        const int q01 = tid % NQ01, q2 = tid / NQ01;
        double H[DD], F[DD], Fi[DD];
        parametric_gradient<DIM, P>(tab, lds + S::off_y, 0, q01, q2, H);
        deformation_gradient<DIM>(H, Ji, F);
        const double J = det_of<DIM>(F);
        inverse_of<DIM>(F, J, Fi);
        c21 = p.mat.m.lambda * J * J + p.mat.m.mu;
#pragma unroll
        for (int m = 0; m < DIM; ++m)
#pragma unroll
          for (int i = 0; i < DIM; ++i) {
            double s = 0.0;
#pragma unroll
            for (int Jx = 0; Jx < DIM; ++Jx) s += Ji[m * DIM + Jx] * MH_M(Fi, Jx, i);
            W[m + i * DIM] = s;
          }
      }
    }
  }
  sync();   // (every lane has read its T2: the backward region may be written)

  double* vals = lds + S::off_vals;
  double* G1 = lds + S::off_g1;
  double* G2 = lds + S::off_g2;
  const int ncomp = da.block ? DD : DIM;
  double* out = da.pieces + e * (int64_t)ND * ncomp;
#pragma unroll 1
  for (int c = 0; c < ncomp; ++c) {
    const int i = da.block ? c / DIM : c, j = da.block ? c % DIM : c;
    if (tid < NPT) {
      // Sm[m + n DIM] = sum_JL dxi_m/dX_J Q_JL dxi_n/dX_L,  Q_JL = w det (stiffness dP_iJ/dF_jL + (i == j) viscosity delta_JL)
      double Sm[DD];
      const double iso = i == j ? wd * da.viscosity : 0.0;
#pragma unroll
      for (int k = 0; k < DD; ++k) Sm[k] = iso * K[k];
      if (stiff) {
        if constexpr (MODE == APPLY_NEOHOOKEAN) {
          // (columns i and j of W by selection: no register array is indexed by a run-time value)
          double wi[DIM], wj[DIM];
#pragma unroll
          for (int m = 0; m < DIM; ++m) {
            wi[m] = i == 0 ? W[m] : i == 1 ? W[m + DIM] : W[m + (DIM - 1) * DIM];
            wj[m] = j == 0 ? W[m] : j == 1 ? W[m + DIM] : W[m + (DIM - 1) * DIM];
          }
          const double f = wd * da.stiffness;
          const double fmu = i == j ? f * p.mat.m.mu : 0.0;
#pragma unroll
          for (int m = 0; m < DIM; ++m)
#pragma unroll
            for (int n = 0; n < DIM; ++n) Sm[m + n * DIM] += fmu * K[m + n * DIM] + f * c21 * wi[m] * wj[n];
        } else {
          const double* r = da.rec + (int64_t)((i * DIM) * DIM + j) * DIM * da.n_pts + pt;   // entry ((i DIM + J) DIM + j) DIM + L
          double T[DD];   // T[m + L DIM] = sum_J dxi_m/dX_J Q_JL
#pragma unroll
          for (int k = 0; k < DD; ++k) T[k] = 0.0;
#pragma unroll
          for (int Jx = 0; Jx < DIM; ++Jx)
#pragma unroll
            for (int L = 0; L < DIM; ++L) {
              const double q = da.stiffness * r[(int64_t)(Jx * DD + L) * da.n_pts];
#pragma unroll
              for (int m = 0; m < DIM; ++m) T[m + L * DIM] += Ji[m * DIM + Jx] * q;
            }
#pragma unroll
          for (int m = 0; m < DIM; ++m)
#pragma unroll
            for (int n = 0; n < DIM; ++n) {
              double s = 0.0;
#pragma unroll
              for (int L = 0; L < DIM; ++L) s += T[m + L * DIM] * Ji[n * DIM + L];
              Sm[m + n * DIM] += s;
            }
        }
      }
      vals[0 * NPT + tid] = Sm[0];
      vals[1 * NPT + tid] = Sm[1 + DIM];
      vals[2 * NPT + tid] = Sm[1] + Sm[DIM];
      vals[3 * NPT + tid] = i == j ? wd * da.density : 0.0;
      if constexpr (DIM == 3) {
        vals[4 * NPT + tid] = Sm[2 + 2 * DIM];
        vals[5 * NPT + tid] = Sm[2] + Sm[2 * DIM];
        vals[6 * NPT + tid] = Sm[1 + 2 * DIM] + Sm[2 + DIM];
      }
    }
    sync();
    // G1[k][a2][q01] = sum_q2 (axis-2 table of kind k)[a2][q2] vals[k][q01 + NQ^2 q2]
    for (int t = tid; t < NK * NBZ * NQ01; t += NT) {
      const int q01 = t % NQ01, a2 = (t / NQ01) % NBZ, k = t / (NQ01 * NBZ);
      const double* tb = prod + ((2 * 3 + diagonal_table_of(2, k)) * NB + a2) * NQ;
      double s = 0.0;
#pragma unroll
      for (int q2 = 0; q2 < NQZ; ++q2) s += tb[q2] * vals[k * NPT + q01 + NQ01 * q2];
      G1[t] = s;
    }
    sync();
    // G2[t0][a12][q0] = sum over the kinds k whose axis-0 table is t0, sum_q1 (axis-1 table of k)[a1][q1] G1[k][a2][q0 + NQ q1]
    for (int t = tid; t < 3 * NB12 * NQ; t += NT) {
      const int q0 = t % NQ, a12 = (t / NQ) % NB12, a1 = a12 % NB, a2 = a12 / NB, t0 = t / (NQ * NB12);
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (diagonal_table_of(0, k) != t0) continue;
        const double* tb = prod + ((1 * 3 + diagonal_table_of(1, k)) * NB + a1) * NQ;
        const double* g1 = G1 + (k * NBZ + a2) * NQ01 + q0;
#pragma unroll
        for (int q1 = 0; q1 < NQ; ++q1) s += tb[q1] * g1[NQ * q1];
      }
      G2[t] = s;
    }
    sync();
    // pieces[e][a0 + NB a12][c] = sum_t0 sum_q0 (axis-0 table t0)[a0][q0] G2[t0][a12][q0]
    for (int t = tid; t < ND; t += NT) {
      const int a0 = t % NB, a12 = t / NB;
      double s = 0.0;
#pragma unroll
      for (int t0 = 0; t0 < 3; ++t0) {
        const double* tb = prod + (t0 * NB + a0) * NQ;
        const double* g2 = G2 + (t0 * NB12 + a12) * NQ;
#pragma unroll
        for (int q0 = 0; q0 < NQ; ++q0) s += tb[q0] * g2[q0];
      }
      out[(int64_t)t * ncomp + c] = s;
    }
    // (the next component's point values are written behind this barrier's predecessors: vals was last read before the
    // second barrier above, G1 before the third; G2 is next written two barriers from here)
  }
}

// dynamic LDS: u_e [DIM][n_dof], then (neo-Hookean) per point F^-1 (column-major) and lambda J^2 + mu
template<int DIM, int MODE>
__global__ __launch_bounds__(256) void diagonal_general_kernel(GeneralArgs p, DiagonalArgs da) {
  constexpr int DD = DIM * DIM, NP = DD + 1;
  extern __shared__ __align__(16) unsigned char smem_diagonal_general[];
  const int64_t e = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_dof = p.n_dof, n_q = p.n_q, n_tdof = n_dof * DIM;
  double* u_e = reinterpret_cast<double*>(smem_diagonal_general);
  double* pts = u_e + n_tdof;
  const bool stiff = da.stiffness != 0.0;
  if constexpr (MODE == APPLY_NEOHOOKEAN) {
    if (stiff) {
      gather_element_vector<DIM>(p.dofs, e, n_dof, da.u_lin, u_e, tid, blockDim.x);
      __syncthreads();
      for (int q = tid; q < n_q; q += blockDim.x) {
        double F[DD], Fi[DD];
        compute_F_general<DIM>(n_dof, p.dN_dX + (e * n_q + q) * n_tdof, u_e, F);
        const double J = det_of<DIM>(F);
        inverse_of<DIM>(F, J, Fi);
#pragma unroll
        for (int k = 0; k < DD; ++k) pts[q * NP + k] = Fi[k];
        pts[q * NP + DD] = p.mat.m.lambda * J * J + p.mat.m.mu;
      }
      __syncthreads();
    }
  }
  const int ncomp = da.block ? DD : DIM;
  double* out = da.pieces + e * (int64_t)n_dof * ncomp;
  const double* gE = p.dN_dX + e * (int64_t)n_q * n_tdof;
  const double* Ne = da.density != 0.0 ? da.N + e * (int64_t)n_q * n_dof : nullptr;
  for (int t = tid; t < n_dof * ncomp; t += blockDim.x) {
    const int c = t % ncomp, a = t / ncomp;
    const int i = da.block ? c / DIM : c, j = da.block ? c % DIM : c;
    double s = 0.0;
    for (int q = 0; q < n_q; ++q) {
      const int64_t pt = e * n_q + q;
      const double wd = p.wdet[pt];
      double g[DIM], g2 = 0.0;
#pragma unroll
      for (int Jx = 0; Jx < DIM; ++Jx) {
        g[Jx] = gE[(int64_t)q * n_tdof + Jx * n_dof + a];
        g2 += g[Jx] * g[Jx];
      }
      double v = 0.0;
      if (i == j) {
        v = wd * da.viscosity * g2;
        if (Ne) {
          const double Na = Ne[(int64_t)q * n_dof + a];
          v += wd * da.density * Na * Na;
        }
      }
      if (stiff) {
        if constexpr (MODE == APPLY_NEOHOOKEAN) {
          const double* Fi = pts + q * NP;
          double hi = 0.0, hj = 0.0;
#pragma unroll
          for (int Jx = 0; Jx < DIM; ++Jx) {
            hi += Fi[Jx + i * DIM] * g[Jx];
            hj += Fi[Jx + j * DIM] * g[Jx];
          }
          v += wd * da.stiffness * ((i == j ? p.mat.m.mu * g2 : 0.0) + Fi[DD] * hi * hj);
        } else {
          const double* r = da.rec + (int64_t)((i * DIM) * DIM + j) * DIM * da.n_pts + pt;
          double w = 0.0;
#pragma unroll
          for (int Jx = 0; Jx < DIM; ++Jx)
#pragma unroll
            for (int L = 0; L < DIM; ++L) w += g[Jx] * r[(int64_t)(Jx * DD + L) * da.n_pts] * g[L];
          v += da.stiffness * w;
        }
      }
      s += v;
    }
    out[t] = s;
  }
}

}  // namespace mimi_hip
