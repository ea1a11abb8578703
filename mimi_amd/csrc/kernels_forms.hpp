// The linear forms of set-up (include/mimi_hip.h, "mass, damping and body-force forms"), assembled into the caller's CSR:
//   mass        A[(A,i),(B,i)] += density   sum_e sum_q w det N_a N_b                  VectorMassIntegrator
//   diffusion   A[(A,i),(B,i)] += viscosity sum_e sum_q w det dN_a/dX_J dN_b/dX_J      VectorDiffusionIntegrator
//   body force  r[(A,i)]       += b_i       sum_e sum_q w det N_a                      VectorDomainLFIntegrator
// (reference: py_nonlinear_solid.cpp:155-192,221-283).  The rule, w det and dN/dX are the handle's own.  One scalar per node
// pair goes to the dim diagonal-component entries of the node block; the i != j entries are not touched.  No atomics, and
// a summation order that is a function of the patch alone: two calls give the same bytes.
//
//   form_tensor_kernel    every tensor_usable patch handle: a row gather with no element pieces.  One workgroup per node A
//                         of the handle's node box, one thread per column B of A's (2p+1)^dim window.  The workgroup walks
//                         the <= (p+1)^dim elements of the box around A in ascending order; per element it stages w det (and
//                         for the diffusion form w det (dxi/dX)(dxi/dX)^T, 6 doubles) of the element's points in LDS, and
//                         the threads whose B lies in the element add its points, shape values and parametric gradients
//                         from the 1-D tables.  Positions: arithmetic on the lexicographic pattern, nbr_pos / nbr_pos16 on
//                         the permuted one, pair_pos for the small-element handles (which build it at create).  No
//                         per-point table of the patch is read or built.
//   form_general_kernel   every other handle, on the general tables (dN_dX / wdet, N from shape_N): one wave per node, the
//                         node -> (element, local node) adjacency in its order, lanes over the element's nodes b, one image
//                         of the row in LDS as in general_gather_kernel.
// The body force is the lumped weight of the nodal field output (kernels_fields.hpp: element pieces of w det N_a, then
// node_gather_kernel) times b.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_general.hpp"
#include "patch_index.hpp"

namespace mimi_hip {

enum { FORM_MASS = 0, FORM_DIFFUSION = 1 };

struct FormArgs {
  double factor;
  double* A;
  int node_lo[3], node_n[3];   // the nodes the handle's elements touch, per direction
  int pos_mode;                // 0 lexicographic structured pattern, 1 permuted (125-wide ranks), 2 permuted (343-wide), 3 pair_pos
  const int64_t* node_ids;     // lexicographic -> caller's node id, nullptr = identity
};

template<int DIM, int P>
struct FormShape : ElementShape<DIM, P> {
  static constexpr int W1 = 2 * P + 1, W1Z = DIM == 3 ? W1 : 1, NW = W1 * W1 * W1Z;
  static constexpr int NK = DIM * (DIM + 1) / 2 + 1;        // upper triangle of w det Ji Ji^T, then w det
  static constexpr int THREADS = (NW + 63) / 64 * 64;
  __host__ __device__ static constexpr int sym(int d, int e) { return d * DIM - d * (d - 1) / 2 + (e - d); }   // d <= e
};

template<int DIM, int P, int KIND>
__global__ __launch_bounds__((FormShape<DIM, P>::THREADS)) void form_tensor_kernel(TensorArgs p, FormArgs fa) {
  using S = FormShape<DIM, P>;
  constexpr int NB = S::NB, NQ = S::NQ, NQZ = S::NQZ, W1 = S::W1, ND = S::ND, NPT = S::NPT, NW = S::NW, DD = S::DD, NK = S::NK;
  __shared__ double Ks[NK * NPT];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  int Am[3] = {0, 0, 0};
  Am[0] = fa.node_lo[0] + (int)(n % fa.node_n[0]);
  Am[1] = fa.node_lo[1] + (int)((n / fa.node_n[0]) % fa.node_n[1]);
  if (DIM == 3) Am[2] = fa.node_lo[2] + (int)(n / ((int64_t)fa.node_n[0] * fa.node_n[1]));
  // the spans of the box that hold A, per direction: first[s] <= A <= first[s] + P (first[s] >= s, strictly increasing)
  int s_lo[3] = {0, 0, 0}, s_n[3] = {1, 1, 1};
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const int32_t* first = p.first[d];
    const int lo = p.box_begin[d];
    int s = min(Am[d], lo + p.box_n[d] - 1);
    while (s >= lo && first[s] > Am[d]) --s;
    const int hi = s;
    while (s >= lo && first[s] + P >= Am[d]) --s;
    s_lo[d] = s + 1;
    s_n[d] = hi - s;
  }
  if (s_n[0] <= 0 || s_n[1] <= 0 || s_n[2] <= 0) return;   // (the same for the whole workgroup)
  // this thread's column: B = A - P + window index, when that is a node of the patch
  int Bm[3] = {0, 0, 0};
  bool valid = tid < NW;
  {
    const int tw[3] = {tid % W1, (tid / W1) % W1, DIM == 3 ? tid / (W1 * W1) : 0};
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      Bm[d] = Am[d] - P + tw[d];
      valid = valid && Bm[d] >= 0 && Bm[d] < p.n_ctrl[d];
    }
  }
  double acc = 0.0;
  bool hit = false;
  int32_t off = 0;
  for (int e2 = 0; e2 < s_n[2]; ++e2)
    for (int e1 = 0; e1 < s_n[1]; ++e1)
      for (int e0 = 0; e0 < s_n[0]; ++e0) {
        const int sp[3] = {s_lo[0] + e0, s_lo[1] + e1, s_lo[2] + e2};
        int64_t el = sp[0] - p.box_begin[0] + (int64_t)p.box_n[0] * (sp[1] - p.box_begin[1]);
        if (DIM == 3) el += (int64_t)p.box_n[0] * p.box_n[1] * (sp[2] - p.box_begin[2]);
        __syncthreads();   // (the previous element's points have been read)
        for (int q = tid; q < NPT; q += S::THREADS) {
          const double* g = p.geo + el * (int64_t)((DD + 1) * NPT) + q;
          const double wd = g[(int64_t)DD * NPT];
          if constexpr (KIND == FORM_DIFFUSION) {
            double Ji[DD];
#pragma unroll
            for (int k = 0; k < DD; ++k) Ji[k] = g[(int64_t)k * NPT];     // dxi_d / dX_J at (d DIM + J)
#pragma unroll
            for (int d = 0; d < DIM; ++d)
#pragma unroll
              for (int e = d; e < DIM; ++e) {
                double s = 0.0;
#pragma unroll
                for (int J = 0; J < DIM; ++J) s += Ji[d * DIM + J] * Ji[e * DIM + J];
                Ks[S::sym(d, e) * NPT + q] = wd * s;
              }
          }
          Ks[(NK - 1) * NPT + q] = wd;
        }
        __syncthreads();
        int al[3] = {0, 0, 0}, bl[3] = {0, 0, 0};
        bool in = valid;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          const int f = p.first[d][sp[d]];
          al[d] = Am[d] - f;
          bl[d] = Bm[d] - f;
          in = in && bl[d] >= 0 && bl[d] <= P;
        }
        if (!in) continue;
        hit = true;
        if (fa.pos_mode == 3) {
          const int a = al[0] + NB * (al[1] + NB * al[2]), b = bl[0] + NB * (bl[1] + NB * bl[2]);
          off = p.pair_pos[(el * ND + a) * ND + b];
        }
        // 1-D table rows of a and b, [NQ] each; the direction a 2-D patch lacks: B = 1, D = 0
        const double *Ba[3], *Bb[3], *Da[3], *Db[3];
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          const int64_t oa = ((int64_t)sp[d] * NB + al[d]) * NQ, ob = ((int64_t)sp[d] * NB + bl[d]) * NQ;
          Ba[d] = p.tabB[d] + oa;
          Bb[d] = p.tabB[d] + ob;
          Da[d] = p.tabD[d] + oa;
          Db[d] = p.tabD[d] + ob;
        }
        for (int q2 = 0; q2 < NQZ; ++q2) {
          double ba2 = 1.0, bb2 = 1.0, da2 = 0.0, db2 = 0.0;
          if constexpr (DIM == 3) {
            ba2 = Ba[2][q2];
            bb2 = Bb[2][q2];
            da2 = Da[2][q2];
            db2 = Db[2][q2];
          }
          for (int q1 = 0; q1 < NQ; ++q1) {
            const double ba1 = Ba[1][q1], bb1 = Bb[1][q1], da1 = Da[1][q1], db1 = Db[1][q1];
            double s = 0.0;
#pragma unroll
            for (int q0 = 0; q0 < NQ; ++q0) {
              const int q = q0 + NQ * (q1 + NQ * q2);
              const double ba0 = Ba[0][q0], bb0 = Bb[0][q0];
              if constexpr (KIND == FORM_MASS) {
                s += Ks[(NK - 1) * NPT + q] * (ba0 * bb0);
              } else {
                const double da0 = Da[0][q0], db0 = Db[0][q0];
                const double ga[3] = {da0 * ba1 * ba2, ba0 * da1 * ba2, ba0 * ba1 * da2};
                const double gb[3] = {db0 * bb1 * bb2, bb0 * db1 * bb2, bb0 * bb1 * db2};
                double v = 0.0;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                  double t = 0.0;
#pragma unroll
                  for (int e = 0; e < DIM; ++e) t += Ks[S::sym(d < e ? d : e, d < e ? e : d) * NPT + q] * gb[e];
                  v += ga[d] * t;
                }
                s += v;
              }
            }
            if constexpr (KIND == FORM_MASS) acc += s * ((ba1 * bb1) * (ba2 * bb2));
            else acc += s;
          }
        }
      }
  if (!hit) return;
  // the dim diagonal-component entries of block (A, B)
  int lo[3] = {0, 0, 0}, w[3] = {1, 1, 1};
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    lo[d] = Am[d] - P < 0 ? 0 : Am[d] - P;
    const int hi = Am[d] + P > p.n_ctrl[d] - 1 ? p.n_ctrl[d] - 1 : Am[d] + P;
    w[d] = hi - lo[d] + 1;
  }
  const int rank = (Bm[0] - lo[0]) + w[0] * ((Bm[1] - lo[1]) + w[1] * (Bm[2] - lo[2]));
  const int64_t Alex = Am[0] + (int64_t)p.n_ctrl[0] * (Am[1] + (int64_t)p.n_ctrl[1] * Am[2]);
  const int64_t gA = fa.node_ids ? fa.node_ids[Alex] : Alex;
  if (fa.pos_mode == 0) off = DIM * rank;
  else if (fa.pos_mode == 1) off = DIM * (int)p.nbr_pos[Alex * 125 + rank];
  else if (fa.pos_mode == 2) off = DIM * (int)p.nbr_pos16[Alex * 343 + rank];
  const double v = fa.factor * acc;
#pragma unroll
  for (int i = 0; i < DIM; ++i) fa.A[p.rowptr[gA * DIM + i] + off + i] += v;
}

// one wave per node; N [n_el][n_q][n_dof] (mass), dN_dX [n_el][n_q][DIM][n_dof] (diffusion)
template<int DIM, int KIND>
__global__ __launch_bounds__(64 * GG_WAVES) void form_general_kernel(int64_t n_nodes, int n_dof, int n_q, const int64_t* __restrict__ rowptr,
                                                                     const int64_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj,
                                                                     const int32_t* __restrict__ pair_pos, const double* __restrict__ N,
                                                                     const double* __restrict__ dN_dX, const double* __restrict__ wdet,
                                                                     double factor, double* A) {
  __shared__ double img_all[GG_WAVES][GG_MAX_ROW];
  __shared__ unsigned char hit_all[GG_WAVES][GG_MAX_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = (int64_t)blockIdx.x * GG_WAVES + wave;
  if (node >= n_nodes) return;
  const int64_t a_beg = adj_ptr[node], a_end = adj_ptr[node + 1];
  if (a_beg == a_end) return;   // no element of this handle touches the node (element boxes)
  double* img = img_all[wave];
  unsigned char* hit = hit_all[wave];
  const int64_t beg = rowptr[node * DIM];
  const int len = (int)(rowptr[node * DIM + 1] - beg);
  for (int k = lane; k < len; k += 64) {
    img[k] = 0.0;
    hit[k] = 0;
  }
  __builtin_amdgcn_wave_barrier();
  for (int64_t t = a_beg; t < a_end; ++t) {
    const int32_t ea = adj[t];
    const int64_t e = ea >> 6;
    const int a = ea & 63;
    for (int b = lane; b < n_dof; b += 64) {    // (distinct b: distinct positions within an instruction)
      double s = 0.0;
      for (int q = 0; q < n_q; ++q) {
        const int64_t pt = e * n_q + q;
        if constexpr (KIND == FORM_MASS) {
          s += wdet[pt] * (N[pt * n_dof + a] * N[pt * n_dof + b]);
        } else {
          const double* g = dN_dX + pt * DIM * n_dof;
          double v = 0.0;
#pragma unroll
          for (int J = 0; J < DIM; ++J) v += g[J * n_dof + a] * g[J * n_dof + b];
          s += wdet[pt] * v;
        }
      }
      const int32_t off = pair_pos[(e * n_dof + a) * n_dof + b];
      img[off] += s;
      hit[off] = 1;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < len; k += 64) {
    if (!hit[k]) continue;
    const double v = factor * img[k];
#pragma unroll
    for (int i = 0; i < DIM; ++i) A[rowptr[node * DIM + i] + k + i] += v;
  }
}

// r[(A, i)] += b_i weight[A] on the nodes this handle's elements touch
template<int DIM>
__global__ void form_body_force_kernel(int64_t n_nodes, const double* __restrict__ weight, double b0, double b1, double b2,
                                       double* __restrict__ r) {
  const int64_t A = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= n_nodes) return;
  const double w = weight[A];
  if (w == 0.0) return;
  const double b[3] = {b0, b1, b2};
#pragma unroll
  for (int i = 0; i < DIM; ++i) r[A * DIM + i] += b[i] * w;
}

}  // namespace mimi_hip
