// Phase 1 of the two-phase tangent assembly as a ROLE-SPECIALISED workgroup (p = 2, 3-D).
//
// Why: a single wave doing everything for an (element column, row i) -- the first phase-1 kernel of this path --
// needs the whole register file of a SIMD (constitutive stage + contraction tiles + prefetch live together) and
// 31 KB of LDS, so it runs alone per SIMD and every LDS / matrix-pipe / memory latency is exposed (measured:
// ~46 k cycles per (element, i) for ~20 k cycles of issued work).  Here the work of one element column is
// split over four waves of one workgroup so that each wave fits in half a register file and two workgroups
// (8 waves) share a CU:
//
//   wave 0  "X"   quadrature-point stage: the point's material ONCE per point (the single-wave kernel
//                 repeated this for every row i) -- here read from the record of the material pre-pass,
//                 in kernels_tensor_wgsym.hpp from F --, then per row i the residual piece (sum
//                 factorisation) and the pulled-back tangent row
//                 Ahat_i[m][j][n] -> LDS (lane = quadrature point, private slots).
//   wave 1+i "Y_i" contraction of row i:  S1 (matrix pipe, q2) -> S2 (vector pipe, q1, wave-uniform
//                 coefficients) -> S3 (matrix pipe, q0), with the tile TRANSPOSED with respect to
//                 the single-wave kernel: rows = (a2,b2) pair index, so that the entries shared with
//                 the next element of the column, (a2,b2) -> (a2-1,b2-1) = pair index - 4, are the
//                 NEXT ACCUMULATOR REGISTER OF THE SAME LANE.  The carry along the column therefore
//                 lives in registers (27 doubles per lane) instead of a 17.5 KB LDS tile with
//                 read-modify-write; LDS is only used to transpose the finished entries for
//                 coalesced stores (write once, read once).
//
// Per element X evaluates the points of the NEXT element and then writes its three Ahat rows; Y_i contracts the
// column components j = 0, 1, 2 of row i.  Only Ahat is shared, with a single LDS buffer:
//     Y: [tables, j = 0, j = 1: free running]  [read the j = 2 operands] barrier [j = 2, flush] barrier
//     X: [point stage of the next element: free running]               barrier [its rows]       barrier
// (what runs free reads data written before the previous barrier and writes nothing another wave reads before
// the next one; the store-transposition buffer of a contraction wave is private).  Every wave executes 2 n + 1
// barriers.  Scratch layout, phase 2 and the bitwise reproducibility of the result: kernels_tensor_2phase.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "materials_other.hpp"

#include "kernels_tensor_2phase.hpp"
#include "p2_tile_map.hpp"

namespace mimi_hip {

// The shape all degree-2 3-D kernels share: degree, basis functions and quadrature points per direction, their products
struct P2Shape {
  static constexpr int P = 2, NB = 3, NQ = 4, NB2 = 9, ND = 27, NQ3 = 64, NROW = 81;
};

// LDS doubles of stage R (p2_stage_r) at `rows` rows per pass: PH [rows][3 m][64], V [rows][3 m][3 a2][16], W [rows][3 m][9 a1a2][4]
constexpr int p2_stage_r_size(int rows) {
  using S = P2Shape;
  return rows * 3 * (S::NQ3 + S::NB * S::NQ * S::NQ + S::NB2 * S::NQ);
}

struct WgsLds : P2Shape {
  static constexpr int off_tab = 0;                      // [2 parity][3 dir][2][3][4]  X -> Y
  static constexpr int off_r = off_tab + 2 * 6 * NB * NQ;  // stage-R scratch, one row    X private
  static constexpr int off_ah = off_r + p2_stage_r_size(1);  // [3 i][27 (m,j,n)][64]        X -> Y_i
  static constexpr int n_final = 9 * NROW + 18 * ND;     // 1215 entries stored by a non-last element
  static constexpr int n_carry = 18 * 2 * ND;            // 972 more by the last element of a column
  static constexpr int st_size = n_final + 1;
  static constexpr int off_st = off_ah + 3 * ND * NQ3;   // [3 i][1216] store transposition     Y_i private
  static constexpr int total = off_st + 3 * st_size;
};

#define WGS_PIN(x) asm volatile("" : "+v"(x))

MH_DEV void wgs_barrier() {
  // LDS hand-off only: outstanding global loads / stores need not drain here
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// v_permlane32_swap(a, b) -> ([a.lo, b.lo], [a.hi, b.hi]) (halves of 32 lanes; checked on gfx950,
// scratch/pl/pl_test.hip).  One pair of swaps gives both rotations the carry needs:
//   c_hi_in_lo : lanes 0..31 hold c of lanes 32..63      o_lo_in_hi : lanes 32..63 hold o of lanes 0..31
MH_DEV void swap32_f64(double c, double o, double& c_hi_in_lo, double& o_lo_in_hi) {
  const unsigned long long uc = __double_as_longlong(c), uo = __double_as_longlong(o);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)uc, (unsigned)uo, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(uc >> 32), (unsigned)(uo >> 32), false, false);
  o_lo_in_hi = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
  c_hi_in_lo = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
}

// ------------------------------------------------------------------------------------------------
// J2: material pre-pass.  The return mapping (scalar Newton with dual-number Johnson-Cook hardening:
// pow / log in fp64) costs tens of thousands of cycles per point; inside the workgroup it would run in
// the single point wave and bound the whole kernel.  Here every wave of the chip takes one element
// (lane = quadrature point) and leaves the PointResult in scratch_pt[element][field][point].
// ------------------------------------------------------------------------------------------------
// record of a point: Finv 9, detF, sigma (symmetric: 6), trial deviator (symmetric: 6), beta, gamma of the algorithmic
// tangent (materials.hpp tangent_row_of) -- P = J sigma F^-T is recomputed by the reader
constexpr int WGS_PT_FIELDS = 24;

MH_DEV void wgs_point_store(double* rec, int lane, const mimi_hip_material& m, const PointResult<3>& w) {
  constexpr int NQ3 = P2Shape::NQ3;
  constexpr int sym_i[6] = {0, 1, 2, 1, 2, 2}, sym_j[6] = {0, 0, 0, 1, 1, 2};
#pragma unroll
  for (int k = 0; k < 9; ++k) rec[k * NQ3 + lane] = w.Finv[k];
  rec[9 * NQ3 + lane] = w.detF;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    rec[(10 + k) * NQ3 + lane] = w.sigma[sym_i[k] + 3 * sym_j[k]];
    rec[(16 + k) * NQ3 + lane] = w.s_trial[sym_i[k] + 3 * sym_j[k]];
  }
  double beta, gamma;
  j2_beta_gamma<3>(m, w, beta, gamma);
  rec[22 * NQ3 + lane] = beta;
  rec[23 * NQ3 + lane] = gamma;
}

// w gets Finv, detF, sigma, s_trial and (recomputed as the material does, pk1_from_cauchy) P
MH_DEV void wgs_point_load(const double* rec, int lane, PointResult<3>& w, double& beta, double& gamma) {
  constexpr int NQ3 = P2Shape::NQ3;
  constexpr int sym_i[6] = {0, 1, 2, 1, 2, 2}, sym_j[6] = {0, 0, 0, 1, 1, 2};
#pragma unroll
  for (int k = 0; k < 9; ++k) w.Finv[k] = rec[k * NQ3 + lane];
  w.detF = rec[9 * NQ3 + lane];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double sg = rec[(10 + k) * NQ3 + lane], st = rec[(16 + k) * NQ3 + lane];
    w.sigma[sym_i[k] + 3 * sym_j[k]] = sg;
    w.sigma[sym_j[k] + 3 * sym_i[k]] = sg;
    w.s_trial[sym_i[k] + 3 * sym_j[k]] = st;
    w.s_trial[sym_j[k] + 3 * sym_i[k]] = st;
  }
  beta = rec[22 * NQ3 + lane];
  gamma = rec[23 * NQ3 + lane];
  pk1_from_cauchy<3>(w);
}

// The other materials (materials_other.hpp): no closed form of the pulled-back tangent -- the pre-pass leaves the
// tangent itself, pulled back to the reference element and weighted, in the record:
//   field i*27 + (m*3 + j)*3 + n : Ahat_i[m][j][n] = wd sum_JL Jinv[m][J] dP_iJ/dF_jL Jinv[n][L]
//   field 81 + i*3 + m           : Phat_i[m]       = wd sum_J  P_iJ Jinv[m][J]
// (46 KB per element; wave X of the nine-block kernel then only copies its row into LDS).
constexpr int WGS_REC_FIELDS = 90;
constexpr int WGS_KIND_RECORD = 100;   // compile-time "material kind" of the kernels that read such records

// FAMILY 0: J2 (24-field record, closed forms in wave X); 2..5: that one of the other materials (90-field record) as a
// compile-time constant (all four in one kernel spilled 168 .. 298 registers, one at a time none).
// COMMIT 1: DomainPostTimeAdvance (nonlinear_solid.cpp:179-199) -- F at the points as for an assembly, then the material's
// state commit and nothing else (round 4: the separate commit kernel's unrolled 27-node sum took 432 registers, one wave per
// SIMD: 4.8 ms for the 16.8 M points of the north-star mesh with J2)
template<int FAMILY, int COMMIT = 0>
__global__ __launch_bounds__(256) void tensor_point_kernel(TensorArgs p, int n_el) {
  constexpr int P = P2Shape::P, NB = P2Shape::NB, NQ = P2Shape::NQ, ND = P2Shape::ND, NQ3 = P2Shape::NQ3;
  constexpr int FK = family_kind<FAMILY>();
  __shared__ double ue_all[4][3 * ND];
  __shared__ double tab_all[4][6 * NB * NQ];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + wave;
  if (e >= n_el) return;
  double* ue = ue_all[wave];
  double* tab = tab_all[wave];
  // (own text of the element side of patch_index.hpp: through its helpers the instruction stream changes)
  int el[3];
  el[0] = e % p.box_n[0];
  el[1] = (e / p.box_n[0]) % p.box_n[1];
  el[2] = e / ((int64_t)p.box_n[0] * p.box_n[1]);
  const int32_t* dofs = p.dofs + e * ND;
  for (int a = lane; a < ND; a += 64) {
    const int64_t node = dofs[a];
    for (int c = 0; c < 3; ++c) ue[c * ND + a] = p.u[node * 3 + c];
  }
  for (int t = lane; t < 6 * NB * NQ; t += 64) {
    const int dir = t / (2 * NB * NQ), rem = t % (2 * NB * NQ), isD = rem / (NB * NQ), k = rem % (NB * NQ);
    const int span = p.box_begin[dir] + el[dir];
    tab[t] = ((isD ? p.tabD[dir] : p.tabB[dir]) + (int64_t)span * NB * NQ)[k];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int q0 = lane % NQ, q1 = (lane / NQ) % NQ, q2 = lane / (NQ * NQ);
  double H[9];
  for (int k = 0; k < 9; ++k) H[k] = 0.0;
#pragma unroll 1
  for (int a2 = 0; a2 < NB; ++a2)
#pragma unroll 1
    for (int a1 = 0; a1 < NB; ++a1)
      for (int a0 = 0; a0 < NB; ++a0) {
        const int a = a0 + NB * (a1 + NB * a2);
        const double b0 = tab_ptr<P>(tab, 0, 0)[a0 * NQ + q0], d0 = tab_ptr<P>(tab, 0, 1)[a0 * NQ + q0];
        const double b1 = tab_ptr<P>(tab, 1, 0)[a1 * NQ + q1], d1 = tab_ptr<P>(tab, 1, 1)[a1 * NQ + q1];
        const double b2 = tab_ptr<P>(tab, 2, 0)[a2 * NQ + q2], d2 = tab_ptr<P>(tab, 2, 1)[a2 * NQ + q2];
        // same association as the point wave: d0 * (b1 * b2), b0 * (d1 * b2), b0 * (b1 * d2)
        const double dn0 = d0 * (b1 * b2), dn1 = b0 * (d1 * b2), dn2 = b0 * (b1 * d2);
        for (int i = 0; i < 3; ++i) {
          const double uu = ue[i * ND + a];
          H[i * 3 + 0] += uu * dn0;
          H[i * 3 + 1] += uu * dn1;
          H[i * 3 + 2] += uu * dn2;
        }
      }
  const double* g = p.geo + e * 10 * NQ3 + lane;
  double F[9];
  for (int i = 0; i < 3; ++i)
    for (int J = 0; J < 3; ++J) {
      double sf = (i == J) ? 1.0 : 0.0;
      for (int m = 0; m < 3; ++m) sf += H[i * 3 + m] * g[(int64_t)(m * 3 + J) * NQ3];
      F[i + J * 3] = sf;
    }
  if constexpr (COMMIT) {
    int st;
    if constexpr (FAMILY != 0) st = accumulate_other<3, FK>(p.mat, p.dt, p.state, e * NQ3 + lane, F);
    else st = accumulate_state<3>(p.mat, p.dt, p.state, e * NQ3 + lane, F);
    if (st) atomicOr(p.status, st);
    return;
  }
  if constexpr (FAMILY != 0) {
    // the tangent one direction (j, L) at a time, pulled back and accumulated over L as it arrives (27 accumulators per j
    // instead of all 81 entries of dP/dF: see tp3_point_kernel, tensor_p3.hip)
    double Pk[9];
    OtherTangent<3> ot;
    const int status = other_tangent_begin<3, FK>(p.mat, p.dt, p.state, e * NQ3 + lane, F, Pk, ot);
    double* rec = p.scratch_pt + e * (int64_t)(WGS_REC_FIELDS * NQ3) + lane;
    const double wd = g[(int64_t)9 * NQ3];
    double Ji[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ji[k] = g[(int64_t)k * NQ3];
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
      double acc[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll 1
      for (int L = 0; L < 3; ++L) {
        double dP[9];
        other_tangent_dir<3, FK>(p.mat, p.dt, F, ot, j, L, dP);
        double jl[3];     // Jinv[n][L]
#pragma unroll
        for (int n = 0; n < 3; ++n) jl[n] = L == 0 ? Ji[n * 3] : (L == 1 ? Ji[n * 3 + 1] : Ji[n * 3 + 2]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int m = 0; m < 3; ++m) {
            double b = 0.0;
#pragma unroll
            for (int J = 0; J < 3; ++J) b += Ji[m * 3 + J] * dP[i + J * 3];
#pragma unroll
            for (int n = 0; n < 3; ++n) acc[(i * 3 + m) * 3 + n] += b * jl[n];
          }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
          for (int n = 0; n < 3; ++n) rec[(int64_t)(i * 27 + (m * 3 + j) * 3 + n) * NQ3] = wd * acc[(i * 3 + m) * 3 + n];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double t = 0.0;
#pragma unroll
        for (int J = 0; J < 3; ++J) t += Pk[i + J * 3] * Ji[m * 3 + J];
        rec[(int64_t)(81 + i * 3 + m) * NQ3] = wd * t;
      }
    if (status) atomicOr(p.status, status);
  } else {
    PointResult<3> w;
    const int status = evaluate_pk1<3>(p.mat, p.dt, p.state, e * NQ3 + lane, F, w);
    wgs_point_store(p.scratch_pt + e * (int64_t)(WGS_PT_FIELDS * NQ3), lane, p.mat.m, w);
    if (status) atomicOr(p.status, status);
  }
}

// ------------------------------------------------------------------------------------------------
// wave X
// ------------------------------------------------------------------------------------------------
// What wave X keeps per quadrature point between its three steps.  KIND is the material kind as a
// compile-time constant: the fields the other material needs are then dead, and so is its code.
template<int KIND>
struct WgsPoint;

// Neo-Hookean, closed form of the pulled-back tangent: with G = Jinv F^-1 (G[m][i] = sum_J Jinv[m][J] Finv[J][i])
// and M = Jinv Jinv^T, from dP_iJ/dF_jL = mu d_ij d_JL - c1 Finv_Li Finv_Jj + c2 Finv_Lj Finv_Ji
// (materials.hpp tangent_of):
//   Ahat_i[m][j][n] = wd (mu d_ij M[m][n] - c1 G[n][i] G[m][j] + c2 G[n][j] G[m][i])
template<>
struct WgsPoint<MIMI_HIP_MAT_NEOHOOKEAN> {
  double G[9], M[6], Phat[9];  // Phat[i*3 + m]
  double mu_w, c1_w, c2_w;     // coefficients times wd
};

// J2 (small-strain return mapping inside finite kinematics, materials.hpp tangent_row_of): with G = Jinv F^-1,
// N = G Jinv^T, Q[n][j] = sum_L s_jL Jinv[n][L], S_i[m] = sum_k sigma_ik G[m][k], Ts_i[m] = sum_k s_ik G[m][k]
// (s = trial deviator), the pulled-back tangent row is
//   Ahat_i[m][j][n] = wd J ( G[n][j] S_i[m] - G[m][j] S_i[n] + (K - beta 2G/3) G[m][i] Jinv[n][j]
//                            + beta G (d_ij N[m][n] + G[m][j] Jinv[n][i]) - 2G gamma Ts_i[m] Q[n][j] )
template<>
struct WgsPoint<MIMI_HIP_MAT_J2> {
  double G[9], Ji[9], N[9], Q[9], sig[9], st[9], Phat[9];
  double wdJ, Kc, hb, gg;   // wd J, K - beta 2G/3, beta G, 2G gamma
};

template<>
struct WgsPoint<WGS_KIND_RECORD> {
  const double* rec;   // this lane's column of the element's record
};

// fills WgsPoint<J2> from the PointResult of the material pre-pass
MH_DEV void wgs_j2_point(const mimi_hip_material& m, const PointResult<3>& w, double beta, double gamma, const double* Ji,
                         double wd, WgsPoint<MIMI_HIP_MAT_J2>& s) {
  const double G2 = 2.0 * m.G;
  s.wdJ = wd * w.detF;
  s.Kc = m.K - beta * G2 / 3.0;
  s.hb = 0.5 * beta * G2;
  s.gg = G2 * gamma;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    s.Ji[k] = Ji[k];
    s.sig[k] = w.sigma[k];
    s.st[k] = w.s_trial[k];
  }
#pragma unroll
  for (int mm = 0; mm < 3; ++mm)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double g = 0.0;
#pragma unroll
      for (int Jx = 0; Jx < 3; ++Jx) g += Ji[mm * 3 + Jx] * w.Finv[Jx + c * 3];
      s.G[mm * 3 + c] = g;
    }
#pragma unroll
  for (int mm = 0; mm < 3; ++mm)
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v += s.G[mm * 3 + k] * Ji[n * 3 + k];
      s.N[mm * 3 + n] = v;
    }
#pragma unroll
  for (int n = 0; n < 3; ++n)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
#pragma unroll
      for (int Lx = 0; Lx < 3; ++Lx) v += w.s_trial[j + Lx * 3] * Ji[n * 3 + Lx];
      s.Q[n * 3 + j] = v;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int mm = 0; mm < 3; ++mm) {
      double sp = 0.0;
#pragma unroll
      for (int Jx = 0; Jx < 3; ++Jx) sp += w.P[i + Jx * 3] * Ji[mm * 3 + Jx];
      s.Phat[i * 3 + mm] = wd * sp;
    }
}

// fills WgsPoint<neo-Hookean> from F at the point (no pre-pass: the law is a dozen instructions)
MH_DEV void wgs_neohookean_point(const mimi_hip_material& mat, const double* F, const double* Ji, double wd,
                                 WgsPoint<MIMI_HIP_MAT_NEOHOOKEAN>& s) {
  PointResult<3> w;
  neo_hookean_stress<3>(mat, F, w);
  const double J = w.detF;
  s.mu_w = wd * mat.mu;
  s.c1_w = wd * (mat.lambda * J * (J - 1.) - mat.mu);
  s.c2_w = wd * (mat.lambda * (2. * J - 1.) * J);
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double g = 0.0;
#pragma unroll
      for (int Jx = 0; Jx < 3; ++Jx) g += Ji[m * 3 + Jx] * w.Finv[Jx + i * 3];
      s.G[m * 3 + i] = g;
    }
  {
    int c = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int n = m; n < 3; ++n) {
        double v = 0.0;
#pragma unroll
        for (int Jx = 0; Jx < 3; ++Jx) v += Ji[m * 3 + Jx] * Ji[n * 3 + Jx];
        s.M[c++] = v;
      }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      double sp = 0.0;
#pragma unroll
      for (int Jx = 0; Jx < 3; ++Jx) sp += w.P[i + Jx * 3] * Ji[m * 3 + Jx];
      s.Phat[i * 3 + m] = wd * sp;
    }
}

// ------------------------------------------------------------------------------------------------
// stage R: residual rows of one element by sum factorisation, three passes through LDS
// ------------------------------------------------------------------------------------------------
// Rows I0 .. I0 + ROWS - 1 of an element.  In: the caller has stored Phat, RS[(I * 3 + m) * 64 + point] (lane = point); tab =
// the element's tables.  Out: er[a * 3 + I0 + I], er = the element's part of scratch_r ([element][a][i]: tensor_p2_kernel
// reads a node's three rows from one sector).  The rows of a call share the LDS passes.
// Lane -> output maps of the three passes (as in the degree-3 pre-pass): a lane owns ONE pair of the indices that are neither
// summed nor a tensor component, reads its table values once and walks (I, m) with compile-time offsets -- 48 / 36 / 54 (one row:
// 27) of the 64 lanes busy, a third of the instructions of loops over the flat output index (20 - 30 integer instructions of
// index arithmetic per four multiply-adds).  Every sum runs in index order as a chain of fused multiply-adds from 0.0.
template<int ROWS>
MH_DEV void p2_stage_r(const double* tab, double* RS, int lane, double* er, int I0) {
  using S = P2Shape;
  constexpr int P = S::P, NB = S::NB, NQ = S::NQ, NB2 = S::NB2, ND = S::ND, NQ3 = S::NQ3;
  double* PH = RS;                              // [ROWS I][3 m][64]
  double* V = PH + ROWS * 3 * NQ3;              // [ROWS I][3 m][3 a2][16]
  double* W = V + ROWS * 3 * NB * NQ * NQ;      // [ROWS I][3 m][9 a1a2][4]
  __builtin_amdgcn_wave_barrier();
  // V[I m][a2][q0 q1] = sum_q2 T2^m[a2][q2] PH[I m][q0 q1 q2]
  if (lane < NB * NQ * NQ) {
    const int q01 = lane & 15, a2 = lane >> 4;
    double T[2][NQ];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q2 = 0; q2 < NQ; ++q2) T[v][q2] = tab_ptr<P>(tab, 2, v)[a2 * NQ + q2];
#pragma unroll
    for (int im = 0; im < ROWS * 3; ++im) {
      double sv = 0.0;
#pragma unroll
      for (int q2 = 0; q2 < NQ; ++q2) sv = __builtin_fma(T[im % 3 == 2 ? 1 : 0][q2], PH[im * NQ3 + q01 + NQ * NQ * q2], sv);
      V[im * (NB * NQ * NQ) + lane] = sv;   // (im * NB + a2) * 16 + q01
    }
  }
  __builtin_amdgcn_wave_barrier();
  // W[I m][a1 a2][q0] = sum_q1 T1^m[a1][q1] V[I m][a2][q0 q1]
  if (lane < NB2 * NQ) {
    const int q0 = lane & 3, a12 = lane >> 2, a1 = a12 % NB, a2 = a12 / NB;
    double T[2][NQ];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q1 = 0; q1 < NQ; ++q1) T[v][q1] = tab_ptr<P>(tab, 1, v)[a1 * NQ + q1];
#pragma unroll
    for (int im = 0; im < ROWS * 3; ++im) {
      double sw = 0.0;
#pragma unroll
      for (int q1 = 0; q1 < NQ; ++q1) sw = __builtin_fma(T[im % 3 == 1 ? 1 : 0][q1], V[(im * NB + a2) * NQ * NQ + q0 + NQ * q1], sw);
      W[im * (NB2 * NQ) + lane] = sw;   // (im * NB2 + a12) * 4 + q0
    }
  }
  __builtin_amdgcn_wave_barrier();
  // er[a][I] = sum_m sum_q0 T0^m[a0][q0] W[I m][a1 a2][q0]: lanes 0..26 take the even rows, lanes 27..53 the odd ones
  if (lane < (ROWS > 1 ? 2 : 1) * ND) {
    const int a = lane < ND ? lane : lane - ND, a0 = a % NB, a12 = a / NB;
    double T[2][NQ];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q0 = 0; q0 < NQ; ++q0) T[v][q0] = tab_ptr<P>(tab, 0, v)[a0 * NQ + q0];
    const int n_rows = lane < ND ? (ROWS + 1) / 2 : ROWS / 2;
    for (int k = 0; k < n_rows; ++k) {
      const int I = lane < ND ? 2 * k : 2 * k + 1;
      double sr = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int q0 = 0; q0 < NQ; ++q0) sr = __builtin_fma(T[m == 0 ? 1 : 0][q0], W[((I * 3 + m) * NB2 + a12) * NQ + q0], sr);
      er[a * 3 + I0 + I] = sr;
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// row I of one element: Ahat_I -> LDS (lane = quadrature point), residual piece -> scratch_r
template<int KIND, int I>
MH_DEV void wgs_x_row(const TensorArgs& p, double* lds, int lane, int64_t e, int par, const WgsPoint<KIND>& s) {
  using L = WgsLds;
  constexpr int NB = L::NB, NQ = L::NQ, ND = L::ND, NQ3 = L::NQ3;
  static_assert(KIND == MIMI_HIP_MAT_J2 || KIND == WGS_KIND_RECORD, "nine-block kernel: the material comes from the pre-pass");
  const double* tab = lds + L::off_tab + par * 6 * NB * NQ;
  double* AH = lds + L::off_ah + I * ND * NQ3;
  double* RS = lds + L::off_r;
  double Phat[3];
  if constexpr (KIND == WGS_KIND_RECORD) {
#pragma unroll
    for (int m = 0; m < 3; ++m) Phat[m] = s.rec[(int64_t)(81 + I * 3 + m) * NQ3];
    double v[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) v[k] = s.rec[(int64_t)(I * ND + k) * NQ3];
#pragma unroll
    for (int k = 0; k < ND; ++k) AH[k * NQ3 + lane] = v[k];
  } else {
#pragma unroll
    for (int m = 0; m < 3; ++m) Phat[m] = s.Phat[I * 3 + m];
    double S[3], Ts[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a += s.sig[I + k * 3] * s.G[m * 3 + k];
        b += s.st[I + k * 3] * s.G[m * 3 + k];
      }
      S[m] = a;
      Ts[m] = b;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          double v = s.G[n * 3 + j] * S[m] - s.G[m * 3 + j] * S[n];
          v += s.Kc * s.G[m * 3 + I] * s.Ji[n * 3 + j];
          v += s.hb * ((I == j ? s.N[m * 3 + n] : 0.0) + s.G[m * 3 + j] * s.Ji[n * 3 + I]);
          v -= s.gg * Ts[m] * s.Q[n * 3 + j];
          AH[((m * 3 + j) * 3 + n) * NQ3 + lane] = s.wdJ * v;
        }
  }
  // residual row I (one row per pass: the LDS of two workgroups per CU has room for one row's buffers)
#pragma unroll
  for (int m = 0; m < 3; ++m) RS[m * NQ3 + lane] = Phat[m];
  p2_stage_r<1>(tab, RS, lane, p.scratch_r + e * ND * 3, I);
}

// ------------------------------------------------------------------------------------------------
// the column walk of a workgroup, and what the point wave requests along it (also used by kernels_tensor_wgsym.hpp)
// ------------------------------------------------------------------------------------------------
// A workgroup walks some units back to back, a unit = one segment of p.seg_len elements of an element column (unit index =
// column * segments-per-column + segment; the nine-block kernel: one unit, a whole column).  The walk keeps the element, its
// spans and its layer and moves one element at a time: the unit's column by division when a unit begins, then one layer further
// per step (asked for by division at every use -- g / seg_len, % segments, column % n0, column / n0 -- they were ~12 run-time
// integer divisions, 300 - 400 scalar instructions per element, in the point wave and ~80 in a contraction wave).
struct ColumnWalk {
  int first, nseg;     // the workgroup's first unit; segments per column
  int g, pos, unit;    // sequence index = unit * seg_len + pos; position inside the unit; unit inside the workgroup
  int cx, cy, ez;      // the element inside the box: the spans of its column, its layer
  int64_t e;           // the element
  MH_DEV ColumnWalk(const TensorArgs& p, int first_unit) : first(first_unit), nseg(p.box_n[2] / p.seg_len), g(0) { begin_unit(p, 0); }
  MH_DEV void begin_unit(const TensorArgs& p, int u) {
    const int un = first + u, col = un / nseg;
    unit = u;
    pos = 0;
    cx = col % p.box_n[0];
    cy = col / p.box_n[0];
    ez = (un % nseg) * p.seg_len;
    e = cx + (int64_t)p.box_n[0] * (cy + (int64_t)p.box_n[1] * ez);
  }
  MH_DEV void advance(const TensorArgs& p) {
    ++g;
    if (++pos == p.seg_len) {
      begin_unit(p, unit + 1);
    } else {
      ++ez;
      e += (int64_t)p.box_n[0] * p.box_n[1];
    }
  }
};

// Tables (72 values, [3 dir][B, D][3][4] as they lie in LDS: two per lane) and geometry (10 per lane) of an element, requested
// at the END of the previous element's last step: they are in flight across the two barriers, not across the row
// computations, which need the registers.
struct WgsOperands {
  static constexpr int NT = 6 * P2Shape::NB * P2Shape::NQ, TROUNDS = 2;
  double tab[TROUNDS], geo[10];
  MH_DEV static const double* table_src(const TensorArgs& p, const ColumnWalk& c, int t) {
    constexpr int NBQ = P2Shape::NB * P2Shape::NQ;
    const int dir = t / (2 * NBQ);
    const int rem = t % (2 * NBQ);
    const int isD = rem / NBQ;
    const int k = rem % NBQ;
    const int span = (dir == 0 ? p.box_begin[0] + c.cx : dir == 1 ? p.box_begin[1] + c.cy : p.box_begin[2] + c.ez);
    return (isD ? (dir == 0 ? p.tabD[0] : dir == 1 ? p.tabD[1] : p.tabD[2])
                : (dir == 0 ? p.tabB[0] : dir == 1 ? p.tabB[1] : p.tabB[2])) + (int64_t)span * NBQ + k;
  }
  MH_DEV void request(const TensorArgs& p, const ColumnWalk& c, int lane) {
#pragma unroll
    for (int rd = 0; rd < TROUNDS; ++rd) {
      const int t = rd * 64 + lane;
      tab[rd] = *table_src(p, c, t < NT ? t : 0);
    }
    const double* g = p.geo + c.e * 10 * P2Shape::NQ3 + lane;
#pragma unroll
    for (int k = 0; k < 10; ++k) geo[k] = g[(int64_t)k * P2Shape::NQ3];
  }
  MH_DEV void tables_to_lds(double* dst, int lane) const {
#pragma unroll
    for (int rd = 0; rd < TROUNDS; ++rd) {
      const int t = rd * 64 + lane;
      if (t < NT) dst[t] = tab[rd];
    }
  }
};

// wave X of the nine-block kernel: per element the point's record of the material pre-pass, then the three rows
template<int KIND>
MH_DEV void wgs_x_loop(const TensorArgs& p, double* lds, int unit) {
  using L = WgsLds;
  const int lane = threadIdx.x & 63;
  const int n_seq = p.seg_len;
  ColumnWalk cq(p, unit);   // the element whose operands are requested next
  ColumnWalk cs = cq;       // the element of the next quadrature-point stage
  ColumnWalk cr = cq;       // the element whose rows are written next
  WgsOperands op;
  auto request = [&]() {
    op.request(p, cq, lane);
    if (cq.g + 1 < n_seq) cq.advance(p);
  };
  WgsPoint<KIND> s;
  // quadrature-point stage of the element at cs from the requested operands (tables -> LDS parity g & 1)
  auto point_stage = [&]() {
    op.tables_to_lds(lds + L::off_tab + (cs.g & 1) * WgsOperands::NT, lane);
    if constexpr (KIND == WGS_KIND_RECORD) {
      s.rec = p.scratch_pt + cs.e * (int64_t)(WGS_REC_FIELDS * L::NQ3) + lane;
    } else {
      // J2: the material was evaluated by tensor_point_kernel
      PointResult<3> w;
      double beta, gamma;
      wgs_point_load(p.scratch_pt + cs.e * (int64_t)(WGS_PT_FIELDS * L::NQ3), lane, w, beta, gamma);
      wgs_j2_point(p.mat.m, w, beta, gamma, op.geo, op.geo[9], s);
    }
    __builtin_amdgcn_wave_barrier();
    if (cs.g + 1 < n_seq) cs.advance(p);
  };
  auto rows = [&]() {
    wgs_x_row<KIND, 0>(p, lds, lane, cr.e, cr.g & 1, s);
    wgs_x_row<KIND, 1>(p, lds, lane, cr.e, cr.g & 1, s);
    wgs_x_row<KIND, 2>(p, lds, lane, cr.e, cr.g & 1, s);
  };
  // prologue: point stage and rows of element 0
  request();
  point_stage();
  if (1 < n_seq) request();
  rows();
  wgs_barrier();
  for (int it = 0; it < n_seq; ++it) {
    // free running: point stage of element it + 1 (its own point data, the table buffer of the OTHER parity)
    if (it + 1 < n_seq) {
      point_stage();
      if (it + 2 < n_seq) request();
    }
    // lock step: rows of element it + 1, once every contraction wave holds its last operands of element it
    wgs_barrier();
    if (it + 1 < n_seq) {
      cr.advance(p);
      rows();
    }
    wgs_barrier();
  }
}

// ------------------------------------------------------------------------------------------------
// contraction waves: shared pieces (also used by kernels_tensor_wgsym.hpp)
// ------------------------------------------------------------------------------------------------
struct WgsLane {
  int lane, grp;
  bool col_ok;
  // 1.0 where the carried value (as held / rotated by 32 lanes) belongs into the first / second result register of this
  // lane group, else 0.0: the carry is added by ONE fused multiply-add instead of a select and an add
  double take_c0, take_c1;
  // compact store-transposition slots (kernels_tensor_wgs.hpp): as computed ...
  int base0, stride0, base1, basec;
  // ... and with the roles of a and b exchanged
  int baseT0, strideT0, baseT1, basecT;
};

// for_dump: the lanes / registers without an entry get zero offsets and strides (what they index is the dump region of
// wgs_contract_block, never a staging buffer)
MH_DEV WgsLane wgs_lane_constants(bool for_dump = false) {
  constexpr int NB = P2Shape::NB, ND = P2Shape::ND, NROW = P2Shape::NROW;
  WgsLane c;
  c.lane = threadIdx.x & 63;
  const int col = c.lane & 15;
  c.grp = c.lane >> 4;
  c.col_ok = col < 9;
  c.take_c0 = c.grp != 2 ? 1.0 : 0.0;
  c.take_c1 = c.grp == 0 ? 1.0 : 0.0;
  const int a0 = c.col_ok ? col / NB : 0, b0 = c.col_ok ? col % NB : 0;
  const int grp = c.grp;
  // rows of register 0: (a2,b2) = (0,0) (0,1) (0,2) (1,0) for grp 0..3; register 1, grp 2: (2,0)
  c.base0 = grp < 3 ? a0 * NROW + grp * ND + b0 * 3 : 9 * NROW + a0 * ND + b0 * 3;
  c.stride0 = grp < 3 ? 3 * NROW : 3 * ND;   // per a1
  c.base1 = 9 * NROW + (a0 + 9) * ND + b0 * 3;  // per a1: 3 * ND
  // carried rows in the element block (P2Block: row a - 9 at 162 (a - 9), this piece's 54 values inside at 54 I -- the
  // caller's pointer --, then (b2 - 1) 27 + b1 9 + b0 3 + j)
  c.basec = a0 * 162 + b0 * 3 + (grp == 0 ? 0 : grp == 1 ? ND : grp == 3 ? 9 * 162 : 9 * 162 + ND);  // per a1: 486
  // transposed: node a' = b, node b' = a.  a2' = b2 == 0 (grp 0, 3; row 6): s = (b0 + 3 b1) 81 + a2 27 + a1 9 + a0 3 + i
  //             a2' = b2 >= 1 (grp 1, 2):      s = 729 + (b0 + 3 b1 + 9 (b2 - 1)) 27 + a1 9 + a0 3 + i
  c.baseT0 = grp == 0 ? b0 * NROW + a0 * 3
           : grp == 3 ? b0 * NROW + ND + a0 * 3
           : grp == 1 ? 9 * NROW + b0 * ND + a0 * 3
                      : 9 * NROW + (b0 + 9) * ND + a0 * 3;
  c.strideT0 = (grp == 0 || grp == 3) ? 3 * NROW : 3 * ND;   // per b1; per a1: 9
  c.baseT1 = b0 * NROW + 2 * ND + a0 * 3;                      // row 6 (2,0) -> (0,2): per b1 3 * NROW; per a1 9
  // carried rows: grp 0 row 4 (1,1) -> (1,1); grp 1 row 5 (1,2) -> (2,1); grp 3 row 7 (2,1) -> (1,2); grp 2 row 8 (2,2)
  //   s' = (a' - 9) 162 + (b2' - 1) 27 + b1' 9 + b0' 3 + i,  a' = b0 + 3 b1 + 9 b2,  b2' = a2
  c.basecT = b0 * 162 + a0 * 3 + (grp == 0 ? 0 : grp == 1 ? 9 * 162 : grp == 3 ? ND : 9 * 162 + ND);   // per b1: 486; per a1: 9
  if (for_dump) {
    if (!c.col_ok) c.base0 = c.stride0 = c.baseT0 = c.strideT0 = 0;
    if (!c.col_ok || grp != 2) c.base1 = c.baseT1 = 0;
  }
  return c;
}

// Lane constants of the RIDER of a packed b1 (p2_tile_map.hpp): its results lie in accumulator registers 2 and 3 of tile 0
//   register 2: grp 1, 2, 3 = pairs (0,0) (0,1) (0,2)  (grp 0 is row 8 of the host)      register 3: grp 0 = (1,0), grp 3 = (2,0)
// and are stored from there (the lanes without an entry: zero constants, dump region); register 3 of grp 1, 2 = pairs (1,1), (1,2)
// is carried; register 3 of tile 1, grp 0, 1 = pairs (2,1), (2,2) is carried into register 3 of tile 0.
struct WgsPackLane {
  bool ok2, ok3;
  bool take2, wide2;              // the carried value belongs into register 2 (grp 1, 2); transposed rows of 81 (grp 1), not 27
  int base2, baseT2;              // + a1 243 + b1 9 + j | + b1 (wide2 ? 243 : 81) + a1 9 + i
  int base3, baseT3;              // + a1 81 + b1 9 + j  | + b1 243 + a1 9 + i
};

MH_DEV WgsPackLane wgs_pack_lane_constants(const WgsLane& lc) {
  constexpr int ND = P2Shape::ND, NROW = P2Shape::NROW, NB = P2Shape::NB;
  WgsPackLane c;
  const int col = lc.lane & 15, grp = lc.grp;
  const int a0 = lc.col_ok ? col / NB : 0, b0 = lc.col_ok ? col % NB : 0;
  c.ok2 = lc.col_ok && grp >= 1;
  c.ok3 = lc.col_ok && (grp == 0 || grp == 3);
  c.take2 = grp == 1 || grp == 2;
  c.wide2 = grp == 1;
  // register 2: a2 = 0, b2 = grp - 1.  Transposed (a' = b): b2 = 0 -> a2' = 0; b2 >= 1 -> the rows of 27
  c.base2 = c.ok2 ? a0 * NROW + (grp - 1) * ND + b0 * 3 : 0;
  c.baseT2 = !c.ok2 ? 0 : grp == 1 ? b0 * NROW + a0 * 3 : 9 * NROW + (b0 + 9 * (grp - 2)) * ND + a0 * 3;
  // register 3: a2 = 1 (grp 0) or 2 (grp 3), b2 = 0
  c.base3 = c.ok3 ? 9 * NROW + (a0 + (grp == 3 ? 9 : 0)) * ND + b0 * 3 : 0;
  c.baseT3 = c.ok3 ? b0 * NROW + (grp == 3 ? 2 : 1) * ND + a0 * 3 : 0;
  return c;
}

// dst with its rows N..15 (of the lane quads in BANKS: bit q = rows 4 q .. 4 q + 3) replaced by rows 0..15 - N of src
// (matrix operand layout: row = lane & 15, one DPP row; v_mov_b32 row_shr:N without bound_ctrl leaves the rows below N alone)
template<int N, int BANKS>
MH_DEV double wgs_rows_up(double dst, double src) {
  const unsigned long long ud = __double_as_longlong(dst), us = __double_as_longlong(src);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)ud, (int)(unsigned)us, 0x110 + N, 0xf, BANKS, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(ud >> 32), (int)(unsigned)(us >> 32), 0x110 + N, 0xf, BANKS, false);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// One (i, j) block of one element in a contraction wave: S1, then S2 / S3 pipelined over b1, the
// carry in registers, finished entries into the store-transposition buffer(s).
// st_n / jn: buffer of piece i and the column component j; st_t / jt: buffer of piece j and i.
// MODE 0: plain block.  MODE 1 (off-diagonal block, i > j): every entry is also stored transposed.
// MODE 2 (diagonal block, i == j): the block is symmetric itself, K[(a1 ..), (b1 ..)] = K[(b1 ..), (a1 ..)]^T, so
// only the six chains with a1 >= b1 are contracted and those with a1 > b1 are also stored transposed
// (st_t == st_n, jt == jn).
// DUMP (round 4, symmetric-half kernel): the staging stores carry no execution mask -- the lanes that hold no
// entry (7 of every 16 columns; for the second register every lane group but 2) store to a 512-double dump region instead
// (their lane constants are zero, wgs_lane_constants(true)).  Thirty mask regions per element and contraction wave
// (s_and_saveexec / s_cbranch_execz / s_or: ~90 scalar instructions and as many scheduling boundaries) are gone.
// PACK = packing level (symmetric-half kernel, with DUMP; p2_b1_packed): the three chains of a packed b1 (p2_tile_map.hpp) go through S3 in two tiles instead
// of three.  S1 and S2 are untouched; the rider's S3 operand rows are moved into idle rows of the hosts' operands (sixteen
// v_mov_b32 row_shr per b1 for four matrix instructions less), every result row is the same sum as in a tile of its own, and
// the rider's results are stored and carried from where they lie (pl; its slot of C holds its pairs (1,1), (1,2); CP, an LDS
// array [b1][64 lanes] of this wave alone, its pairs (2,1), (2,2): written once and read once per element by the same lane --
// two LDS instructions instead of two registers of the 256) -- no permlane swap for the rider.
template<int MODE, bool DUMP = false, int PACK = 0>
MH_DEV void wgs_contract_block(const WgsLane& lc, const double (&ah)[9], const double (&aS0)[4], const double (&aS2)[4],
                               const double (&uB1)[3][4], const double (&uD1)[3][4], double (&C)[9],
                               double* st_n, int jn, double* st_t, int jt, double* dump = nullptr,
                               const WgsPackLane* pl = nullptr, double* CP = nullptr) {
  constexpr int NB = P2Shape::NB, NQ = P2Shape::NQ, ND = P2Shape::ND, NROW = P2Shape::NROW;
  static_assert(!PACK || (DUMP && MODE != 0), "packed tiles: symmetric-half kernel only");
  static_assert(P2_RIDER == 1 && p2_tile_slot(0, 8).tile == 0 && p2_tile_slot(2, 8).tile == 1, "hosts a1 = 0, 2");
  const mh_d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  const int grp = lc.grp;
  double* const dn0 = lc.col_ok ? st_n : dump;
  double* const dn1 = (lc.col_ok && grp == 2) ? st_n : dump;
  double* const dt0 = lc.col_ok ? st_t : dump;
  double* const dt1 = (lc.col_ok && grp == 2) ? st_t : dump;
  mh_d4 D1[9];
#pragma unroll
  for (int mn = 0; mn < 9; ++mn) {
    const int m = mn / 3, n = mn % 3;
    const int v2 = (m == 2 ? 1 : 0) + (n == 2 ? 2 : 0);
    // (diagonal block: Ahat_(i m)(i n) is symmetric in (m, n) and (0, 1), (1, 0) share the table variant: one product)
    if (MODE == 2 && mn == 3) D1[3] = D1[1];
    else D1[mn] = __builtin_amdgcn_mfma_f64_16x16x4f64(ah[mn], aS2[v2], zero4, 0, 0, 0);
  }
  mh_d4 Kt[NB];
  auto carry_and_stage = [&](int b1) {
    const bool packed = p2_b1_packed(MODE, b1, PACK);
    if (packed) {
      // the rider: registers 2, 3 of tile 0 (Kt[0]), register 3 of tile 1 (Kt[2])
      constexpr int a1 = P2_RIDER;
      double* const d2n = pl->ok2 ? st_n : dump;
      double* const d3n = pl->ok3 ? st_n : dump;
      double* const d2t = pl->ok2 ? st_t : dump;
      double* const d3t = pl->ok3 ? st_t : dump;
      // (register 3 takes the whole of CP: rows 14, 15 of tile 1 are sums of zero operand rows)
      const double out3 = __builtin_fma(CP[b1 * 64 + lc.lane], 1.0, Kt[0][3]);
      const double out2 = __builtin_fma(pl->take2 ? C[a1 * NB + b1] : 0.0, 1.0, Kt[0][2]);
      d2n[pl->base2 + a1 * (3 * NROW) + b1 * 9 + jn] = out2;
      d3n[pl->base3 + a1 * (3 * ND) + b1 * 9 + jn] = out3;
      if (MODE == 1 || (MODE == 2 && a1 > b1)) {
        d2t[pl->baseT2 + (pl->wide2 ? b1 * (3 * NROW) : b1 * (3 * ND)) + a1 * 9 + jt] = out2;
        d3t[pl->baseT3 + b1 * (3 * NROW) + a1 * 9 + jt] = out3;
      }
      C[a1 * NB + b1] = out3;
      CP[b1 * 64 + lc.lane] = Kt[2][3];
    }
#pragma unroll
    for (int a1 = 0; a1 < NB; ++a1) {
      if (MODE == 2 && a1 < b1) continue;
      if (packed && a1 == P2_RIDER) continue;
      const int a1b1 = a1 * NB + b1;
      const double cin = C[a1b1];
      double c_rot, o2_rot;
      swap32_f64(cin, Kt[a1][2], c_rot, o2_rot);
      // (the nine-block kernel, MODE 0, has no registers for the two lane masks: it keeps the select + add form)
      const double out0 = MODE == 0 ? Kt[a1][0] + (grp != 2 ? cin : 0.0) : __builtin_fma(cin, lc.take_c0, Kt[a1][0]);
      const double out1 = MODE == 0 ? Kt[a1][1] + (grp == 0 ? c_rot : 0.0) : __builtin_fma(c_rot, lc.take_c1, Kt[a1][1]);
      if constexpr (DUMP) {
        dn0[lc.base0 + a1 * lc.stride0 + b1 * 9 + jn] = out0;
        dn1[lc.base1 + a1 * (3 * ND) + b1 * 9 + jn] = out1;
        if (MODE == 1 || (MODE == 2 && a1 > b1)) {
          dt0[lc.baseT0 + b1 * lc.strideT0 + a1 * 9 + jt] = out0;
          dt1[lc.baseT1 + b1 * (3 * NROW) + a1 * 9 + jt] = out1;
        }
      } else {
        if (lc.col_ok) st_n[lc.base0 + a1 * lc.stride0 + b1 * 9 + jn] = out0;
        if (lc.col_ok && grp == 2) st_n[lc.base1 + a1 * (3 * ND) + b1 * 9 + jn] = out1;
        if (MODE == 1 || (MODE == 2 && a1 > b1)) {
          if (lc.col_ok) st_t[lc.baseT0 + b1 * lc.strideT0 + a1 * 9 + jt] = out0;
          if (lc.col_ok && grp == 2) st_t[lc.baseT1 + b1 * (3 * NROW) + a1 * 9 + jt] = out1;
        }
      }
      C[a1b1] = grp == 2 ? o2_rot : out1;
    }
  };
#pragma unroll
  for (int b1 = 0; b1 < NB; ++b1) {
    // S2.  The nine (m, n) terms are merged by the table variant of their a-side BEFORE the a-side multiplication
    // (g = 3: (0,0); g = 1: (0,1) (0,2); g = 2: (1,0) | (2,0); g = 0: (1,1) (1,2) | (2,1) (2,2)): 9 + 6 x (pairs) instead
    // of 9 + 9 x (pairs) instructions per (b1, q1), every accumulation ONE fused multiply-add (round 3: on this chip
    // every vector instruction costs its ~5 cycles of the SIMD whatever else is in flight, scratch/issue_bench.hip).
    double Ec[4][NB];
#pragma unroll
    for (int q1 = 0; q1 < NQ; ++q1) {
      const double cbB = uB1[b1][q1], cbD = uD1[b1][q1];
      const double W3 = cbB * D1[0][q1];
      const double W1 = __builtin_fma(cbD, D1[1][q1], cbB * D1[2][q1]);
      const double W2a = cbB * D1[3][q1], W2b = cbB * D1[6][q1];
      const double W0a = __builtin_fma(cbD, D1[4][q1], cbB * D1[5][q1]);
      const double W0b = __builtin_fma(cbD, D1[7][q1], cbB * D1[8][q1]);
#pragma unroll
      for (int a1 = 0; a1 < NB; ++a1) {
        if (MODE == 2 && a1 < b1) continue;
        const double caB = uB1[a1][q1], caD = uD1[a1][q1];
        if (q1 == 0) {   // (no accumulator starts from 0.0: x + 0.0 is an instruction)
          Ec[3][a1] = caB * W3;
          Ec[1][a1] = caB * W1;
          Ec[2][a1] = __builtin_fma(caD, W2a, caB * W2b);
          Ec[0][a1] = __builtin_fma(caD, W0a, caB * W0b);
        } else {
          Ec[3][a1] = __builtin_fma(caB, W3, Ec[3][a1]);
          Ec[1][a1] = __builtin_fma(caB, W1, Ec[1][a1]);
          Ec[2][a1] = __builtin_fma(caD, W2a, __builtin_fma(caB, W2b, Ec[2][a1]));
          Ec[0][a1] = __builtin_fma(caD, W0a, __builtin_fma(caB, W0b, Ec[0][a1]));
        }
      }
    }
    if (b1 > 0) carry_and_stage(b1 - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int a1 = 0; a1 < NB; ++a1)
        if (!(MODE == 2 && a1 < b1)) WGS_PIN(Ec[g][a1]);
    const bool packed = p2_b1_packed(MODE, b1, PACK);
    if (packed) {
      static_assert(p2_tile_slot(P2_RIDER, 0).row == P2_RIDER_SHIFT_LOW && p2_tile_slot(P2_RIDER, 8).row == 8 + P2_RIDER_SHIFT_HIGH);
      // rows 9..15 of host 0 <- the rider's pairs 0..6; rows 12..15 of host 2 <- the rider's pairs 7, 8 (and its rows 9, 10: zero)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Ec[g][0] = wgs_rows_up<P2_RIDER_SHIFT_LOW, 0xf>(Ec[g][0], Ec[g][P2_RIDER]);
        Ec[g][2] = wgs_rows_up<P2_RIDER_SHIFT_HIGH, 0x8>(Ec[g][2], Ec[g][P2_RIDER]);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        WGS_PIN(Ec[g][0]);
        WGS_PIN(Ec[g][2]);
      }
    }
#pragma unroll
    for (int a1 = 0; a1 < NB; ++a1)
      if (!(MODE == 2 && a1 < b1) && !(packed && a1 == P2_RIDER)) Kt[a1] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ec[0][a1], aS0[0], zero4, 0, 0, 0);
#pragma unroll
    for (int g = 1; g < 4; ++g)
#pragma unroll
      for (int a1 = 0; a1 < NB; ++a1)
        if (!(MODE == 2 && a1 < b1) && !(packed && a1 == P2_RIDER)) Kt[a1] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ec[g][a1], aS0[g], Kt[a1], 0, 0, 0);
  }
  carry_and_stage(NB - 1);
}

// carried rows of the last element of a column -> the third part of the element block (st_n / st_t: P2Block::carry_of(E, i))
// PACK: the rider of a packed b1 holds its pairs (1,1), (1,2) in grp 1, 2 of its slot of C and its pairs (2,1), (2,2) in grp 0, 1
// of CP[b1][lane] (LDS, wgs_contract_block)
template<int MODE, int PACK = 0>
MH_DEV void wgs_stage_carry(const WgsLane& lc, const double (&C)[9], double* st_n, int jn, double* st_t, int jt,
                            const double* CP = nullptr) {
  constexpr int NB = P2Shape::NB, ND = P2Shape::ND;
#pragma unroll
  for (int a1b1 = 0; a1b1 < 9; ++a1b1) {
    const int a1 = a1b1 / NB, b1 = a1b1 % NB;
    if (MODE == 2 && a1 < b1) continue;
    if (p2_b1_packed(MODE, b1, PACK) && a1 == P2_RIDER) {
      // as basec / basecT of wgs_lane_constants: (a2 - 1) 9 x 162 + (b2 - 1) 27, transposed (b2 - 1) 9 x 162 + (a2 - 1) 27
      const int col = lc.lane & 15, grp = lc.grp;
      const int a0 = lc.col_ok ? col / NB : 0, b0 = lc.col_ok ? col % NB : 0;
      const int n0 = a0 * 162 + b0 * 3 + a1 * 486 + b1 * 9 + jn, t0 = b0 * 162 + a0 * 3 + b1 * 486 + a1 * 9 + jt;
      const bool tr = MODE == 1 || (MODE == 2 && a1 > b1);
      if (lc.col_ok && (grp == 1 || grp == 2)) {          // (1,1), (1,2)
        st_n[n0 + (grp == 2 ? ND : 0)] = C[a1b1];
        if (tr) st_t[t0 + (grp == 2 ? 9 * 162 : 0)] = C[a1b1];
      }
      if (lc.col_ok && grp < 2) {                         // (2,1), (2,2)
        const double cp = CP[b1 * 64 + lc.lane];
        st_n[n0 + 9 * 162 + (grp == 1 ? ND : 0)] = cp;
        if (tr) st_t[t0 + ND + (grp == 1 ? 9 * 162 : 0)] = cp;
      }
      continue;
    }
    if (lc.col_ok) st_n[lc.basec + a1 * 486 + b1 * 9 + jn] = C[a1b1];
    if ((MODE == 1 || (MODE == 2 && a1 > b1)) && lc.col_ok) st_t[lc.basecT + b1 * 486 + a1 * 9 + jt] = C[a1b1];
  }
}

// (the pieces stored with the non-temporal hint: step 7.18 -> 7.09 ms on one box, but WRITE_SIZE of this kernel 8.2 -> 9.9 GB
// -- the runs of 81 / 27 doubles are not whole lines and the hint takes them past the write combining of L2 --: not kept,
// profiles/r04_northstar_nt_pieces.txt)
#define WGS_PIECE_STORE(ptr, v) (*(ptr) = (v))
// buffer (compact: nine rows of 81, eighteen rows of 27) -> this piece's runs in the element block E (P2Block)
MH_DEV void wgs_flush_final(int lane, const double* ST, double* E, int I) {
  constexpr int NROW = P2Shape::NROW, ND = P2Shape::ND;
  {
    // rows a2 = 0: E[a 243 + I 81 + k], k < 81: the first 64 values of a row per instruction, then the 17 others of
    // three rows together (lanes 0..16, 17..33, 34..50)
    const int g3 = lane / 17, k3 = lane - 17 * g3;
    const bool ok3 = lane < 51;
    const int src3 = ok3 ? g3 * NROW + 64 + k3 : 0, dst3 = g3 * 3 * NROW + 64 + k3;
    double v0[9], v1[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) v0[a] = ST[a * NROW + lane];
#pragma unroll
    for (int q = 0; q < 3; ++q) v1[q] = ST[q * 3 * NROW + src3];
    double* d = E + I * NROW;
#pragma unroll
    for (int a = 0; a < 9; ++a) WGS_PIECE_STORE(&d[(unsigned)(a * 3 * NROW + lane)], v0[a]);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (ok3) WGS_PIECE_STORE(&d[(unsigned)(q * 9 * NROW + dst3)], v1[q]);
  }
  {
    // rows a2 >= 1, b2 = 0: E[2187 + (a - 9) 81 + I 27 + k], k < 27: two rows per instruction (lanes 0..26, 32..58)
    const int half = lane >> 5, k = lane & 31;
    const bool ok = k < ND;
    double w[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) w[r] = ST[9 * NROW + (2 * r + half) * ND + (ok ? k : 0)];
    double* d = E + P2Block::off_b20 + I * ND + half * NROW + k;
#pragma unroll
    for (int r = 0; r < 9; ++r)
      if (ok) WGS_PIECE_STORE(&d[(unsigned)(2 * r * NROW)], w[r]);
  }
}

// The tables of a contraction wave as wgs_contract_block takes them, from the element's tables in LDS: aS0, aS2 = pair tables of
// directions 0 and 2 (variants B.B, D.B, B.D, D.D; matrix operand: pair index (a, b) on lane bits 3:0, contraction index on bits
// 5:4), uB1, uD1 = wave-uniform direction-1 tables.
// The tables of directions 0 and 1 belong to the element COLUMN: a caller that keeps the arrays from one element to the next
// asks for them (24 LDS reads, 48 v_readfirstlane, the pair products of direction 0) with column_too at the first element of
// a unit only -- every vector instruction of a contraction wave is on the kernel's critical path;
// direction 2 changes with every element
MH_DEV void wgs_load_tables(const double* tab, int lane, bool column_too, double (&aS0)[4], double (&aS2)[4],
                            double (&uB1)[P2Shape::NB][P2Shape::NQ], double (&uD1)[P2Shape::NB][P2Shape::NQ]) {
  constexpr int P = P2Shape::P, NB = P2Shape::NB, NQ = P2Shape::NQ;
  const int mrow = lane & 15, mk = lane >> 4;
  const bool mrow_ok = mrow < P2Shape::NB2;
  const int mra = mrow_ok ? mrow / NB : 0, mrb = mrow_ok ? mrow % NB : 0;
  auto pair_products = [&](int dir, double (&aS)[4]) {
    const double Ba = tab_ptr<P>(tab, dir, 0)[mra * NQ + mk], Da = tab_ptr<P>(tab, dir, 1)[mra * NQ + mk];
    const double Bb = tab_ptr<P>(tab, dir, 0)[mrb * NQ + mk], Db = tab_ptr<P>(tab, dir, 1)[mrb * NQ + mk];
    aS[0] = mrow_ok ? Ba * Bb : 0.0;
    aS[1] = mrow_ok ? Da * Bb : 0.0;
    aS[2] = mrow_ok ? Ba * Db : 0.0;
    aS[3] = mrow_ok ? Da * Db : 0.0;
  };
  if (column_too) {
    pair_products(0, aS0);
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
      for (int q1 = 0; q1 < NQ; ++q1) {
        const unsigned long long vb = __double_as_longlong(tab_ptr<P>(tab, 1, 0)[a * NQ + q1]);
        const unsigned long long vd = __double_as_longlong(tab_ptr<P>(tab, 1, 1)[a * NQ + q1]);
        const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)vb), bhi = __builtin_amdgcn_readfirstlane((unsigned)(vb >> 32));
        const unsigned dlo = __builtin_amdgcn_readfirstlane((unsigned)vd), dhi = __builtin_amdgcn_readfirstlane((unsigned)(vd >> 32));
        uB1[a][q1] = __longlong_as_double(((unsigned long long)bhi << 32) | blo);
        uD1[a][q1] = __longlong_as_double(((unsigned long long)dhi << 32) | dlo);
      }
  }
  pair_products(2, aS2);
}

// ------------------------------------------------------------------------------------------------
// wave Y_I of the nine-block kernel: row I, one column component j per step
// ------------------------------------------------------------------------------------------------
template<int I>
MH_DEV void wgs_y_loop(const TensorArgs& p, double* lds, int unit) {
  using L = WgsLds;
  constexpr int NB = L::NB, NQ = L::NQ, NB2 = L::NB2, ND = L::ND, NQ3 = L::NQ3;
  const WgsLane lc = wgs_lane_constants();
  const int lane = lc.lane;
  double* AH = lds + L::off_ah + I * ND * NQ3;
  double* ST = lds + L::off_st + I * L::st_size;
  const int n_seq = p.seg_len;
  ColumnWalk c(p, unit);
  auto block_of = [&](int64_t e) -> double* { return p.scratch_k + e * (int64_t)P2Block::size; };

  double C[3][NB2];  // packed carry [j][a1b1]
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < NB2; ++k) C[j][k] = 0.0;
  double aS0[4], aS2[4];
  double uB1[NB][NQ], uD1[NB][NQ];
  auto load_slice = [&](int j, double (&ah)[9]) {
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int n = 0; n < 3; ++n) ah[m * 3 + n] = AH[((m * 3 + j) * 3 + n) * NQ3 + lane];
  };
  // prologue: X writes the rows of element 0
  wgs_barrier();
  for (int it = 0; it < n_seq; ++it) {
    // ---- free running: tables, column components j = 0, 1 (the store-transposition buffer of this wave is private;
    // the operands read here were written before the previous barrier and are rewritten after the next one) -----
    // (all three directions at every element: with the column's tables held from its first element on, as the symmetric-half
    // kernel holds them, this kernel spills 30 registers -- profiles/p2_point_wave_refactor.txt)
    wgs_load_tables(lds + L::off_tab + (it & 1) * WgsOperands::NT, lane, true, aS0, aS2, uB1, uD1);
    {
      double ah[9];
      load_slice(0, ah);
      wgs_contract_block<0>(lc, ah, aS0, aS2, uB1, uD1, C[0], ST, 0, ST, 0);
    }
    {
      double ah[9];
      load_slice(1, ah);
      wgs_contract_block<0>(lc, ah, aS0, aS2, uB1, uD1, C[1], ST, 1, ST, 1);
    }
    // ---- lock step: column component j = 2 while X rewrites the rows for the next element ----------------------
    {
      double ah[9];
      load_slice(2, ah);
      wgs_barrier();
      wgs_contract_block<0>(lc, ah, aS0, aS2, uB1, uD1, C[2], ST, 2, ST, 2);
      // this wave's piece of the element is complete: buffer -> scratch
      __builtin_amdgcn_wave_barrier();
      wgs_flush_final(lane, ST, block_of(c.e), I);
      __builtin_amdgcn_wave_barrier();
      wgs_barrier();
    }
    if (it + 1 < n_seq) c.advance(p);
  }
  // the carried rows of the last element have no successor: straight from the registers into the third part of the piece
  {
    double* Sc = P2Block::carry_of(block_of(c.e), I);
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) wgs_stage_carry<0>(lc, C[jj], Sc, jj, Sc, jj);
  }
}

// Two workgroups per CU (256 registers per wave) for every material.
template<int KIND>
__global__ __launch_bounds__(256, 2) void tensor_wgs_kernel(TensorArgs p) {
  extern __shared__ __align__(16) double smem_wgs[];
  // Wave w of a workgroup lands on SIMD w; the point wave idles more than the contraction waves, so
  // the role of a wave rotates with the workgroup and every SIMD hosts a mix of roles.
#ifndef WGS_ROT
#define WGS_ROT(b) ((b) >> 3)
#endif
  const int role = __builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) + WGS_ROT(blockIdx.x)) & 3);
  const int unit = blockIdx.x;   // one element column per workgroup
  if (role == 0) wgs_x_loop<KIND>(p, smem_wgs, unit);
  else if (role == 1) wgs_y_loop<0>(p, smem_wgs, unit);
  else if (role == 2) wgs_y_loop<1>(p, smem_wgs, unit);
  else wgs_y_loop<2>(p, smem_wgs, unit);
}

inline void launch_tensor_wgs(mimi_hip_domain_s* h, const DomainCall& c, TensorArgs a) {
  h->scratch_k.resize((size_t)h->n_el * P2Block::size);
  h->scratch_r.resize((size_t)h->n_el * 3 * 27);
  a.scratch_k = h->scratch_k.ptr;
  a.scratch_r = h->scratch_r.ptr;
  a.n_units_u = a.box_n[0];
  a.n_units_v = a.box_n[1];
  const size_t lds = WgsLds::total * sizeof(double);
  const int kind = h->mat.m.kind;
  h->scratch_pt.resize((size_t)h->n_el * (material_closed_form(kind) ? WGS_PT_FIELDS : WGS_REC_FIELDS) * 64);
  a.scratch_pt = h->scratch_pt.ptr;
  // phase 1 = material pre-pass + nine-block kernel (the neo-Hookean law goes to launch_tensor_wgsym)
  by_material_family(kind, [&](auto K) {
    constexpr int FK = decltype(K)::value;
    run_two_phase(
        h, c, true,
        [&] { launch(tensor_point_kernel<FK>, dim3((unsigned)((h->n_el + 3) / 4)), dim3(256), 0, h->stream, a, (int)h->n_el); },
        [&] {
          // (the other four materials come to the nine-block kernel as the pre-pass's tangent record)
          auto kernel = FK != 0 ? tensor_wgs_kernel<WGS_KIND_RECORD> : tensor_wgs_kernel<MIMI_HIP_MAT_J2>;
          launch(kernel, dim3(a.box_n[0] * a.box_n[1]), dim3(256), lds, h->stream, a);
        },
        [&] { launch_tensor_p2(h, a); });
  });
}

// DomainPostTimeAdvance at degree 2: the pre-pass kernel in its commit mode
inline void launch_tensor_p2_post(mimi_hip_domain_s* h, TensorArgs a) {
  by_material_family(h->mat.m.kind, [&](auto K) {
    launch(tensor_point_kernel<decltype(K)::value, 1>, dim3((unsigned)((h->n_el + 3) / 4)), dim3(256), 0, h->stream, a, (int)h->n_el);
  });
}

}  // namespace mimi_hip
