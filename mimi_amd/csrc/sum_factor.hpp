// The forward stages of the sum-factorised element kernels (field_tensor_kernel, apply_tensor_kernel), written once: the
// element's 1-D table block into LDS, NC vector components through two parametric directions, and at a point the third --
// the parametric gradient H and the value.  NT threads work on one element; `sync` is their barrier (a workgroup's, a
// wave's, or nothing at all on the host: tests/host_patch_index.hip runs these with NT = 1).  The backward stages contract
// different things per kernel and stay there.  Also the general route's gather of an element vector into LDS.
#pragma once

#include "patch_index.hpp"

namespace mimi_hip {

// tab[dir][B, D][a][q] of the element's spans (element_table_entry)
template<int DIM, int P, int NT>
MH_DEV void load_element_tables(const TensorArgs& p, const int (&el)[3], int tid, double* tab) {
  for (int t = tid; t < 3 * 2 * (P + 1) * (P + 2); t += NT) tab[t] = element_table_entry<DIM, P>(p, el, t);
}

// ve[c][ND] -> T1 (X), then T2 (Y); a barrier behind each
template<int DIM, int P, int NC, int NT, class Sync>
MH_DEV void forward_stages(const double* tab, const double* ve, double* X, double* Y, int tid, Sync&& sync) {
  using S = ElementShape<DIM, P>;
  constexpr int NB = S::NB, NQ = S::NQ, NBZ = S::NBZ, ND = S::ND, NB12 = NB * NBZ, NQ01 = NQ * NQ, TS = NB * NQ;
  // T1[c][k][a12][q0] = sum_a0 tab0[k][a0][q0] v_c[a0 + NB a12]                        (k: 0 B, 1 D)
  for (int t = tid; t < NC * 2 * NB12 * NQ; t += NT) {
    const int q0 = t % NQ, a12 = (t / NQ) % NB12, k = (t / (NQ * NB12)) % 2, c = t / (NQ * NB12 * 2);
    double s = 0.0;
#pragma unroll
    for (int a0 = 0; a0 < NB; ++a0) s += tab[(k * NB + a0) * NQ + q0] * ve[c * ND + a0 + NB * a12];
    X[t] = s;
  }
  sync();
  // T2[c][k][a2][q0 + NQ q1] = sum_a1 tab1[k == 1][a1][q1] T1[c][k == 0][a1 + NB a2][q0]   (k: 0 D0 B1, 1 B0 D1, 2 B0 B1)
  for (int t = tid; t < NC * 3 * NBZ * NQ01; t += NT) {
    const int q01 = t % NQ01, q0 = q01 % NQ, q1 = q01 / NQ, a2 = (t / NQ01) % NBZ, k = (t / (NQ01 * NBZ)) % 3, c = t / (NQ01 * NBZ * 3);
    const double* t1 = X + ((c * 2 + (k == 0 ? 1 : 0)) * NB12 + NB * a2) * NQ + q0;
    const double* tb = tab + (2 + (k == 1 ? 1 : 0)) * TS + q1;
    double s = 0.0;
#pragma unroll
    for (int a1 = 0; a1 < NB; ++a1) s += tb[a1 * NQ] * t1[a1 * NQ];
    Y[t] = s;
  }
  sync();
}

// H[c DIM + m] = d v_c / dxi_m of component set `set` (components set DIM .. set DIM + DIM - 1 of T2) at point (q01, q2)
template<int DIM, int P>
MH_DEV void parametric_gradient(const double* tab, const double* Y, int set, int q01, int q2, double* H) {
  using S = ElementShape<DIM, P>;
  constexpr int NQ = S::NQ, NBZ = S::NBZ, NQ01 = NQ * NQ, TS = S::NB * NQ;
#pragma unroll
  for (int c = 0; c < DIM; ++c)
#pragma unroll
    for (int m = 0; m < DIM; ++m) {
      const double* t2 = Y + (((set * DIM + c) * 3 + (m < 2 ? m : 2)) * NBZ) * NQ01 + q01;
      const double* tb = tab + (4 + (m == 2 ? 1 : 0)) * TS + q2;
      double s = 0.0;
#pragma unroll
      for (int a2 = 0; a2 < NBZ; ++a2) s += tb[a2 * NQ] * t2[a2 * NQ01];
      H[c * DIM + m] = s;
    }
}

// v[c] = v_c of component set 0 at point (q01, q2)
template<int DIM, int P>
MH_DEV void point_value(const double* tab, const double* Y, int q01, int q2, double* v) {
  using S = ElementShape<DIM, P>;
  constexpr int NQ = S::NQ, NBZ = S::NBZ, NQ01 = NQ * NQ, TS = S::NB * NQ;
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    const double* t2 = Y + ((c * 3 + 2) * NBZ) * NQ01 + q01;
    const double* tb = tab + 4 * TS + q2;
    double s = 0.0;
#pragma unroll
    for (int a2 = 0; a2 < NBZ; ++a2) s += tb[a2 * NQ] * t2[a2 * NQ01];
    v[c] = s;
  }
}

// general route: v of the element's nodes -> v_e[i * n_dof + a] (LDS), zeros without a v; nt threads
template<int DIM>
MH_DEV void gather_element_vector(const int32_t* __restrict__ dofs, int64_t e, int n_dof, const double* __restrict__ v, double* v_e,
                                  int tid, int nt) {
  for (int t = tid; t < n_dof * DIM; t += nt) {
    const int a = t % n_dof, i = t / n_dof;
    v_e[t] = v ? v[(int64_t)dofs[e * n_dof + a] * DIM + i] : 0.0;
  }
}

}  // namespace mimi_hip
