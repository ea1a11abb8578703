// Device-resident linear solve of the Newton step and the caller-side eliminations around it (SURVEY 8 rows a10,
// f-4): what the reference does after the assembly returns.
//
//   forms::Nonlinear::AddMult / AddMultGrad  (forms/nonlinear.hpp:76-80,112-115): r[ess] = 0;
//       grad.EliminateRowCol(ess, DIAG_ONE) -- serial loops over the essential dofs there, one kernel each here.
//   PyNonlinearSolid::Setup, "use_iterative_solver" (py/py_nonlinear_solid.cpp:329-339): mfem::GMRESSolver with an
//       mfem::DSmoother (Jacobi) preconditioner, rel 1e-8, abs 1e-12, 300 iterations.  MFEM is an absent, un-pinned
//       submodule of the reference; what is restated here is its published algorithm (mfem linalg/solvers.cpp,
//       GMRESSolver::Mult): left-preconditioned restarted GMRES(m = 50), modified Gram-Schmidt, Givens rotations,
//       convergence on the preconditioned residual  |s_{i+1}| <= max(rel_tol * ||M r_0||, abs_tol).
//   Beyond the reference: the matrix may be a domain handle's matrix-free tangent action (mimi_hip_linear_set_operator:
//       A_values == NULL in a solve), eliminated like the matrix by two vector kernels around it; M may be the Kronecker (fast-diagonalisation) operator of kronecker.hpp instead of Jacobi
//       (preconditioner id 2 of both solvers); ids 0 and 1 run the kernels and give the bits they always did.
//       Jacobi without the matrix: with mimi_hip_linear_set_operator_diagonal armed, id 1 of a solve without values takes
//       1 / diag from the operator's domain (mimi_hip_domain_tangent_diagonal, kernels_diagonal.hpp), built once per solve on
//       the solver's stream behind the event wait of the product, essential dofs 1, fused into the kernel behind the actions.
//       Node-block Jacobi (id 3, mimi_hip_linear_set_node_block): z_A = B_A^-1 r_A with B_A the dim x dim block of node A --
//       read out of the CSR values (a missing entry is zero) or taken from the operator's domain (block mode) -- eliminated
//       like the matrix and inverted per node in closed form, once per solve.
//       With an operator fold the unwrapped diagonal or blocks are summed over the copies of each folded node in the fold's
//       ascending order.  That is the diagonal of P^T A P whenever no element holds both copies of a node, i.e. when the
//       periodic axis has at least two knot spans; with a single span the cross blocks between the two copies are left out.
//       Boundary terms (mimi_hip_linear_add_boundary_operator) contribute nothing to either: for frozen contact and follower
//       pressure the scalar diagonal is identically zero (d m_i / d x_a,i = (e_i x t)_i = 0 in 3-D, m = (t_y, -t_x) in 2-D), so
//       id 1 is exactly the assembled route's Jacobi there; their skew node blocks, the friction action and the
//       consistent-tangent terms are not carried -- the solution is the same, the preconditioner weaker.  With a periodic
//       fold beside the operator (mimi_hip_linear_set_operator_fold) the solver works in the folded numbering and the two
//       vector kernels also expand the input and fold the output: y_f = mask(P^T A_u P (mask x_f)) + x_f[ess], no extra pass.
//
// Everything vector-sized stays in HBM; per Arnoldi step the host sees one Hessenberg column.  Reductions are
// deterministic: a fixed grid writes per-block partial sums, every consumer adds them in the same order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mimi_hip.h"
#include "apply_seam.hpp"
#include "common.hpp"
#include "gmres_host.hpp"
#include "kronecker.hpp"

namespace mimi_hip {

constexpr int KR_BLOCKS = 512;    // reduction grid (two blocks per CU), also the number of partial sums per dot
constexpr int KR_THREADS = 256;

__device__ __forceinline__ double kr_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// sum over the block, result valid in thread 0
__device__ __forceinline__ double kr_block_sum(double v, double* sh) {
  v = kr_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < KR_THREADS / 64; ++w) t += sh[w];
  __syncthreads();
  return t;
}

// the scalar behind KR_BLOCKS partial sums, same order for every reader (every thread gets it)
__device__ __forceinline__ double kr_total(const double* partial, double* sh) {
  double v = 0.0;
  for (int k = threadIdx.x; k < KR_BLOCKS; k += KR_THREADS) v += partial[k];
  v = kr_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < KR_THREADS / 64; ++w) t += sh[w];
  __syncthreads();
  return t;
}

// The products of one wave: ROWS consecutive rows that share ONE column list (ROWS = 3: the three dofs of a node in the
// byVDIM numbering of py_nonlinear_solid.cpp:63, whose CSR rows have identical columns; ROWS = 1: any CSR matrix).  The
// column indices and the gathered x are read once for the ROWS rows; four entries per lane are in flight per trip.  Every
// lane adds its entries in increasing position and the lanes are combined by the same shuffle tree for both values of
// ROWS, so a row's sum does not depend on which form ran.
// NODECOL (ROWS == 3 only): the columns of a row come in triples 3 c, 3 c + 1, 3 c + 2 (the dofs of node c), and `col` is the
// list of the nodes c instead -- a third of the index bytes of the group form, a ninth of the plain one.
template<int ROWS, bool NODECOL>
__device__ __forceinline__ void kr_row_products(int64_t row0, int lane, const int64_t* __restrict__ rowptr,
                                                const int32_t* __restrict__ col, const double* __restrict__ val,
                                                const double* __restrict__ x, double (&s)[ROWS]) {
  const double* v[ROWS];
  const int64_t beg = rowptr[row0];
  const int len = (int)(rowptr[row0 + 1] - beg);
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    v[j] = val + (j == 0 ? beg : rowptr[row0 + j]);
    s[j] = 0.0;
  }
  const int32_t* c = col + (NODECOL ? beg / 9 : beg);
  // four entries per lane and trip, every load of the trip issued before the first product
  for (int k0 = lane; k0 < len; k0 += 256) {
    int32_t cc[4];
    double a[4][ROWS], xx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 64 * u;
      if constexpr (NODECOL) cc[u] = k < len ? 3 * c[k / 3] + k % 3 : 0;
      else cc[u] = k < len ? c[k] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < ROWS; ++j) a[u][j] = k0 + 64 * u < len ? v[j][k0 + 64 * u] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) xx[u] = k0 + 64 * u < len ? x[cc[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + 64 * u < len) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) s[j] = __builtin_fma(a[u][j], xx[u], s[j]);
      }
  }
#pragma unroll
  for (int j = 0; j < ROWS; ++j) s[j] = kr_wave_sum(s[j]);
}

// y = Dinv (A x) (or A x when dinv == nullptr; y = Dinv (b - A x) when b != nullptr): one wave per unit of ROWS rows
template<int ROWS, bool NODECOL>
__global__ __launch_bounds__(256) void kr_spmv_kernel(int64_t n_units, const int64_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const double* __restrict__ val,
                                                      const double* __restrict__ x, const double* __restrict__ b,
                                                      const double* __restrict__ dinv, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int64_t row0 = unit * ROWS;
  double s[ROWS];
  kr_row_products<ROWS, NODECOL>(row0, lane, rowptr, col, val, x, s);
  if (lane == 0) {   // kr_wave_sum leaves the sums in lane 0
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const double t = b ? b[row0 + j] - s[j] : s[j];
      y[row0 + j] = dinv ? dinv[row0 + j] * t : t;
    }
  }
}

// y += alpha A x (mfem::SparseMatrix::AddMult)
template<int ROWS, bool NODECOL>
__global__ __launch_bounds__(256) void kr_add_mult_kernel(int64_t n_units, const int64_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col, const double* __restrict__ val,
                                                          const double* __restrict__ x, double alpha, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int64_t row0 = unit * ROWS;
  double s[ROWS];
  kr_row_products<ROWS, NODECOL>(row0, lane, rowptr, col, val, x, s);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) y[row0 + j] += alpha * s[j];
  }
}

// do rows g b, ..., g b + g - 1 hold the same column list for every b?  One wave per row that is not the first of its
// group; a difference sets `bit` of *status
__global__ __launch_bounds__(256) void kr_groups_kernel(int64_t n, int g, const int64_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, int bit, int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n || row % g == 0) return;
  const int64_t first = row - row % g;
  const int64_t beg = rowptr[row], beg0 = rowptr[first];
  const int64_t len = rowptr[row + 1] - beg;
  bool differ = len != rowptr[first + 1] - beg0;
  if (!differ)
    for (int64_t k = lane; k < len; k += 64) differ |= col[beg + k] != col[beg0 + k];
  if (differ) atomicOr(status, bit);
}

// rows in groups of three with one column list: is that list made of triples 3 c, 3 c + 1, 3 c + 2?  (one wave per group;
// a difference sets `bit` of *status); and the list of the c, at rowptr[3 u] / 9
__global__ __launch_bounds__(256) void kr_nodecol_kernel(int64_t n_units, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         int bit, int* __restrict__ status, int32_t* __restrict__ ncol) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int64_t beg = rowptr[3 * unit];
  const int len = (int)(rowptr[3 * unit + 1] - beg);
  if (!ncol) {
    bool differ = len % 3 != 0 || beg % 9 != 0;
    for (int m = lane; 3 * m + 2 < len; m += 64) {
      const int32_t c0 = col[beg + 3 * m];
      differ |= c0 % 3 != 0 || col[beg + 3 * m + 1] != c0 + 1 || col[beg + 3 * m + 2] != c0 + 2;
    }
    if (differ) atomicOr(status, bit);
  } else {
    for (int m = lane; m < len / 3; m += 64) ncol[beg / 9 + m] = col[beg + 3 * m] / 3;
  }
}

// dinv[row] = 1 / A(row, row)   (mfem::DSmoother, type 0, scale 1)
__global__ void kr_diag_kernel(int64_t n, const int64_t* __restrict__ rowptr, const int64_t* __restrict__ diag_pos,
                               const double* __restrict__ val, double* __restrict__ dinv) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row < n) dinv[row] = 1.0 / val[rowptr[row] + diag_pos[row]];
}

__global__ void kr_diag_pos_kernel(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                   int64_t* __restrict__ diag_pos, int* __restrict__ status) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  int64_t lo = rowptr[row], hi = rowptr[row + 1];
  const int64_t base = lo;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < row) lo = mid + 1; else hi = mid;
  }
  if (lo >= rowptr[row + 1] || col[lo] != row) {
    atomicOr(status, 1);
    diag_pos[row] = 0;
    return;
  }
  diag_pos[row] = lo - base;
}

// one modified Gram-Schmidt stage: w -= h_prev * v_prev (h_prev = total of partial_prev; skipped when v_prev is null),
// then partial_out[block] = sum_block w * v_next (v_next == w itself gives the squared norm)
__global__ __launch_bounds__(KR_THREADS) void kr_mgs_kernel(int64_t n, double* __restrict__ w, const double* __restrict__ v_prev,
                                                            const double* __restrict__ partial_prev, const double* v_next,
                                                            double* __restrict__ partial_out) {
  __shared__ double sh[KR_THREADS / 64];
  constexpr int B = 8;   // entries of a thread whose loads are in flight together (n <= 1 M: all of them)
  const int64_t stride = (int64_t)KR_BLOCKS * KR_THREADS;
  const bool self = (v_next == w);
  double h = 0.0, acc = 0.0;
  const int64_t first = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x;
  int64_t base = first;
  do {   // (every thread makes the first trip, entries or not: the total below holds block barriers)
    double wv[B], pv[B], nv[B];
#pragma unroll
    for (int e = 0; e < B; ++e) {
      const int64_t i = base + e * stride;
      wv[e] = i < n ? w[i] : 0.0;
      pv[e] = (v_prev && i < n) ? v_prev[i] : 0.0;
      nv[e] = (!self && i < n) ? v_next[i] : 0.0;
    }
    if (v_prev && base == first) h = kr_total(partial_prev, sh);   // after the loads are issued
#pragma unroll
    for (int e = 0; e < B; ++e) {
      const int64_t i = base + e * stride;
      if (i < n) {
        double wi = wv[e];
        if (v_prev) {
          wi -= h * pv[e];
          w[i] = wi;
        }
        acc += wi * (self ? wi : nv[e]);
      }
    }
    base += B * stride;
  } while (base < n);
  const double t = kr_block_sum(acc, sh);
  if (threadIdx.x == 0) partial_out[blockIdx.x] = t;
}

// v = w / sqrt(total(partial_norm2)), v = 0 where that norm is 0
__global__ __launch_bounds__(KR_THREADS) void kr_normalize_kernel(int64_t n, const double* __restrict__ w,
                                                                  const double* __restrict__ partial_norm2, double* __restrict__ v) {
  __shared__ double sh[KR_THREADS / 64];
  const double nrm = sqrt(kr_total(partial_norm2, sh));
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)KR_BLOCKS * KR_THREADS) v[i] = w[i] * inv;
}

// totals[c] = total of partial array c, c < n_cols (one block per column; same order as kr_total)
__global__ __launch_bounds__(KR_THREADS) void kr_totals_kernel(const double* __restrict__ partials, double* __restrict__ totals) {
  __shared__ double sh[KR_THREADS / 64];
  const double t = kr_total(partials + (int64_t)blockIdx.x * KR_BLOCKS, sh);
  if (threadIdx.x == 0) totals[blockIdx.x] = t;
}

// x += sum_k y[k] V[k]
__global__ __launch_bounds__(KR_THREADS) void kr_update_kernel(int64_t n, int k_count, const double* __restrict__ V, int64_t ldv,
                                                               const double* __restrict__ y, double* __restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KR_THREADS) {
    double s = x[i];
    for (int k = 0; k < k_count; ++k) s += y[k] * V[(int64_t)k * ldv + i];
    x[i] = s;
  }
}

// conjugate gradients: z = dinv o r (or r), partial_out = partial sums of r . z
__global__ __launch_bounds__(KR_THREADS) void kr_cg_precond_kernel(int64_t n, const double* __restrict__ r, const double* __restrict__ dinv,
                                                                   double* __restrict__ z, double* __restrict__ partial_out) {
  __shared__ double sh[KR_THREADS / 64];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)KR_BLOCKS * KR_THREADS) {
    const double ri = r[i], zi = dinv ? dinv[i] * ri : ri;
    z[i] = zi;
    acc += ri * zi;
  }
  const double t = kr_block_sum(acc, sh);
  if (threadIdx.x == 0) partial_out[blockIdx.x] = t;
}

// x += alpha d; r -= alpha q
__global__ __launch_bounds__(KR_THREADS) void kr_cg_update_kernel(int64_t n, double alpha, const double* __restrict__ d,
                                                                  const double* __restrict__ q, double* __restrict__ x, double* __restrict__ r) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KR_THREADS) {
    x[i] += alpha * d[i];
    r[i] -= alpha * q[i];
  }
}

// d = z + beta d
__global__ __launch_bounds__(KR_THREADS) void kr_cg_direction_kernel(int64_t n, double beta, const double* __restrict__ z, double* __restrict__ d) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KR_THREADS) d[i] = z[i] + beta * d[i];
}

// forms/nonlinear.hpp:76-80: r[ess] = 0
__global__ void kr_zero_entries_kernel(int64_t n_ess, const int64_t* __restrict__ ess, double* __restrict__ r) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n_ess) r[ess[k]] = 0.0;
}

// SparseMatrix::EliminateRowCol(rc, DIAG_ONE) for every essential dof (forms/nonlinear.hpp:112-115): one wave per row;
// an entry goes when its row or its column is essential, the diagonal of an essential row becomes 1
__global__ __launch_bounds__(256) void kr_eliminate_kernel(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const unsigned char* __restrict__ is_ess, double* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const bool row_ess = is_ess[row];
  for (int64_t k = rowptr[row] + lane; k < rowptr[row + 1]; k += 64) {
    const int32_t c = col[k];
    if (row_ess) val[k] = (c == row) ? 1.0 : 0.0;
    else if (is_ess[c]) val[k] = 0.0;
  }
}

// the eliminated product with an operator, y = mask(A (mask x)) + x[ess], around the action "y += A xm":
// before it xm = mask x, y = 0 ...
__global__ __launch_bounds__(KR_THREADS) void kr_operator_mask_kernel(int64_t n, const unsigned char* __restrict__ is_ess,
                                                                      const double* __restrict__ x, double* __restrict__ xm,
                                                                      double* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KR_THREADS) {
    xm[i] = is_ess[i] ? 0.0 : x[i];
    y[i] = 0.0;
  }
}

// ... behind it y[ess] = x[ess], y = b - y with b, and y = dinv o y with dinv (Jacobi from the operator's diagonal)
__global__ __launch_bounds__(KR_THREADS) void kr_operator_restore_kernel(int64_t n, const unsigned char* __restrict__ is_ess,
                                                                         const double* __restrict__ x, const double* __restrict__ b,
                                                                         const double* __restrict__ dinv, double* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KR_THREADS) {
    double t = is_ess[i] ? x[i] : y[i];
    if (b) t = b[i] - t;
    y[i] = dinv ? dinv[i] * t : t;
  }
}

// The same pair with a periodic fold (mimi_hip_linear_set_operator_fold): x, y and is_ess are in the folded numbering, the
// actions run between the two kernels in the unwrapped one, y_f = mask(P^T A_u P (mask x_f)) + x_f[ess].
// Before the actions, per unwrapped dof: xu = (mask x_f)[map], yu = 0 (the folded dof of node n, component c is
// node_map[n] DIM + c) ...
template<int DIM>
__global__ __launch_bounds__(KR_THREADS) void kr_operator_mask_expand_kernel(int64_t n_u, const int32_t* __restrict__ node_map,
                                                                             const unsigned char* __restrict__ is_ess,
                                                                             const double* __restrict__ x, double* __restrict__ xu,
                                                                             double* __restrict__ yu) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n_u; i += (int64_t)gridDim.x * KR_THREADS) {
    const int64_t node = i / DIM;
    const int64_t j = (int64_t)node_map[node] * DIM + (i - node * DIM);
    xu[i] = is_ess[j] ? 0.0 : x[j];
    yu[i] = 0.0;
  }
}

// ... behind them, per folded dof: the copies of its node added in ascending order from zero (the order and the start of
// fold.hip's residual fold, so the sum has its bits), y[ess] = x[ess], and y = b - y with b.  One thread writes an entry.
template<int DIM>
__global__ __launch_bounds__(KR_THREADS) void kr_operator_fold_restore_kernel(int64_t n_f, const int32_t* __restrict__ copy_ptr,
                                                                              const int32_t* __restrict__ copies,
                                                                              const unsigned char* __restrict__ is_ess,
                                                                              const double* __restrict__ x, const double* __restrict__ b,
                                                                              const double* __restrict__ dinv,
                                                                              const double* __restrict__ yu, double* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; i < n_f; i += (int64_t)gridDim.x * KR_THREADS) {
    double t;
    if (is_ess[i]) {
      t = x[i];
    } else {
      const int64_t node = i / DIM;
      const int c = (int)(i - node * DIM);
      t = 0.0;
      for (int k = copy_ptr[node]; k < copy_ptr[node + 1]; ++k) t += yu[(int64_t)copies[k] * DIM + c];
    }
    if (b) t = b[i] - t;
    y[i] = dinv ? dinv[i] * t : t;
  }
}

// ---- Jacobi from the operator's diagonal, node-block Jacobi ---------------------------------------------------------------

// d[F][c] = the sum of du[copy][c] over the copies of folded node F, ascending from zero (the order of the folded product);
// nc values per node
__global__ void kr_fold_sum_kernel(int64_t n_nodes_f, int nc, const int32_t* __restrict__ copy_ptr, const int32_t* __restrict__ copies,
                                   const double* __restrict__ du, double* __restrict__ d) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_nodes_f * nc) return;
  const int64_t node = idx / nc;
  const int c = (int)(idx - node * nc);
  double t = 0.0;
  for (int k = copy_ptr[node]; k < copy_ptr[node + 1]; ++k) t += du[(int64_t)copies[k] * nc + c];
  d[idx] = t;
}

// dinv = 1 / d, 1 on the essential dofs (the diagonal EliminateRowCol(DIAG_ONE) leaves), in place; a free dof whose
// diagonal is zero or not finite leaves the smallest such dof in *bad
__global__ void kr_operator_dinv_kernel(int64_t n, const unsigned char* __restrict__ is_ess, double* __restrict__ d,
                                        unsigned long long* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (is_ess[i]) {
    d[i] = 1.0;
    return;
  }
  const double v = d[i];
  if (!(v != 0.0) || !isfinite(v)) atomicMin(bad, (unsigned long long)i);
  d[i] = 1.0 / v;
}

// pos[row][j] = where column (node of row) dim + j stands in the row, -1 when the pattern lacks it (as kr_diag_pos_kernel)
__global__ void kr_block_pos_kernel(int64_t n, int dim, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                    int64_t* __restrict__ pos) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * dim) return;
  const int64_t row = idx / dim;
  const int64_t want = (row / dim) * dim + (idx - row * dim);
  int64_t lo = rowptr[row], hi = rowptr[row + 1];
  const int64_t base = lo, end = hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] < want) lo = mid + 1; else hi = mid;
  }
  pos[idx] = (lo < end && col[lo] == want) ? lo - base : -1;
}

// B[A][i][j] = A((A, i), (A, j)), zero where the pattern has no such entry
__global__ void kr_block_values_kernel(int64_t n, int dim, const int64_t* __restrict__ rowptr, const int64_t* __restrict__ pos,
                                       const double* __restrict__ val, double* __restrict__ B) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * dim) return;
  B[idx] = pos[idx] >= 0 ? val[rowptr[idx / dim] + pos[idx]] : 0.0;
}

// B_A <- (the block eliminated like the matrix: row and column of an essential dof zero, its diagonal 1)^-1 in closed form;
// a determinant that is zero or not finite leaves the smallest such node in *bad
template<int DIM>
__global__ void kr_block_invert_kernel(int64_t n_nodes, const unsigned char* __restrict__ is_ess, double* __restrict__ B,
                                       unsigned long long* __restrict__ bad) {
  const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n_nodes) return;
  double m[DIM][DIM], inv[DIM][DIM];
  bool e[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) e[i] = is_ess[node * DIM + i] != 0;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) m[i][j] = (e[i] || e[j]) ? (i == j ? 1.0 : 0.0) : B[(node * DIM + i) * DIM + j];
  double det;
  if constexpr (DIM == 1) {
    det = m[0][0];
    inv[0][0] = 1.0;
  } else if constexpr (DIM == 2) {
    det = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    inv[0][0] = m[1][1], inv[0][1] = -m[0][1], inv[1][0] = -m[1][0], inv[1][1] = m[0][0];
  } else {
    inv[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    inv[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
    inv[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    inv[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    inv[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
    inv[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    inv[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    inv[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
    inv[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    det = m[0][0] * inv[0][0] + m[0][1] * inv[1][0] + m[0][2] * inv[2][0];
  }
  if (!(det != 0.0) || !isfinite(det)) {
    atomicMin(bad, (unsigned long long)node);
    return;
  }
  const double over = 1.0 / det;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j)   // (row and column of an essential dof: the identity's, without the rounding of det / det)
      B[(node * DIM + i) * DIM + j] = (e[i] || e[j]) ? (i == j ? 1.0 : 0.0) : inv[i][j] * over;
}

// z_A = Binv_A r_A (z == r allowed: a thread reads its node's r before it writes), partial_out = partial sums of r . z
template<int DIM>
__global__ __launch_bounds__(KR_THREADS) void kr_block_apply_kernel(int64_t n_nodes, const double* __restrict__ binv, const double* r,
                                                                    double* z, double* __restrict__ partial_out) {
  __shared__ double sh[KR_THREADS / 64];
  double acc = 0.0;
  for (int64_t node = (int64_t)blockIdx.x * KR_THREADS + threadIdx.x; node < n_nodes; node += (int64_t)KR_BLOCKS * KR_THREADS) {
    double rv[DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j) rv[j] = r[node * DIM + j];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < DIM; ++j) s += binv[(node * DIM + i) * DIM + j] * rv[j];
      z[node * DIM + i] = s;
      acc += rv[i] * s;
    }
  }
  const double t = kr_block_sum(acc, sh);
  if (threadIdx.x == 0 && partial_out) partial_out[blockIdx.x] = t;
}

__global__ void kr_mark_kernel(int64_t n_ess, const int64_t* __restrict__ ess, unsigned char* __restrict__ is_ess) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n_ess) is_ess[ess[k]] = 1;
}

}  // namespace mimi_hip

using namespace mimi_hip;

struct mimi_hip_linear_s : StreamHandle {
  int64_t n = 0, nnz = 0;
  int kdim = 50;
  DeviceBuffer<int64_t> rowptr_own, diag_pos, ess;
  DeviceBuffer<int32_t> col_own;
  const int64_t* rowptr = nullptr;
  const int32_t* col = nullptr;
  DeviceBuffer<unsigned char> is_ess;
  int64_t n_ess = 0;
  int group = 1;          // rows g b .. g b + g - 1 share their column list (kr_groups_kernel; g = 3, 2 or 1): read once per group
  bool nodecol = false;   // ... and, g = 3, the list is made of node triples: `ncol` holds the nodes (kr_nodecol_kernel)
  DeviceBuffer<int32_t> ncol;
  DeviceBuffer<double> dinv, V, w, r, partials, totals, ycoef, stage_val, stage_b, stage_x;
  Kronecker kron;         // mimi_hip_linear_set_kronecker: preconditioner id 2
  // mimi_hip_linear_set_operator: the domain handle whose tangent action is the product of a solve without matrix values
  mimi_hip_domain_s* op_domain = nullptr;
  double op_density = 0.0, op_stiffness = 0.0, op_viscosity = 0.0;
  DeviceBuffer<double> op_x;   // the masked input of the action
  // mimi_hip_linear_add_boundary_operator: face tangents added to the domain's action, in the order they were set
  struct BoundaryTerm {
    int kind;        // mimi_hip_boundary_operator_kind
    void* handle;
    double factor;
  };
  static constexpr int kMaxBoundaryTerms = 8;
  BoundaryTerm op_terms[kMaxBoundaryTerms];
  int n_op_terms = 0;
  // mimi_hip_linear_set_operator_fold: the operator handles live in the unwrapped numbering of this fold, the solver in the
  // folded one; the expanded input and the unwrapped output of the actions
  mimi_hip_fold_s* op_fold = nullptr;
  DeviceBuffer<double> op_xu, op_yu;
  // mimi_hip_linear_set_operator_diagonal: id 1 of a solve without values takes its diagonal from the operator's domain
  bool op_diagonal = false;
  DeviceBuffer<double> op_du;   // with a fold: the unwrapped diagonal or blocks, before the copies are summed
  // mimi_hip_linear_set_node_block: the handle's n is n_nodes * node_block in byVDIM order (0: not set); preconditioner id 3
  int node_block = 0;
  DeviceBuffer<int64_t> block_pos;     // [n][node_block]: where the block's entries stand in their CSR rows, found at first use
  bool have_block_pos = false;
  DeviceBuffer<double> binv;           // [n_nodes][node_block][node_block]: the inverted blocks of this solve
  DeviceBuffer<unsigned long long> bad_node;
  // dofs an operator handle must have: the unwrapped size with a fold, the solver's own without
  int64_t operator_n() const {
    if (!op_fold) return n;
    const OperatorFold f = operator_fold(op_fold);
    return f.n_nodes_u * f.dim;
  }
  DeviceBuffer<int> status;                      // one word: what the pattern checks of create found
  double* column_host[2] = {nullptr, nullptr};   // pinned: the Hessenberg column of the step before last and of the last one
  hipEvent_t column_ready[2] = {nullptr, nullptr};
  int column_cap = 0;
  void reserve_columns(int count) {
    if (count <= column_cap) return;
    for (int k = 0; k < 2; ++k) {
      if (column_host[k]) MH_HIP(hipHostFree(column_host[k]));
      column_host[k] = nullptr;
      MH_HIP(hipHostMalloc(reinterpret_cast<void**>(&column_host[k]), sizeof(double) * count, hipHostMallocDefault));
      if (!column_ready[k]) MH_HIP(hipEventCreateWithFlags(&column_ready[k], hipEventDisableTiming));
    }
    column_cap = count;
  }
  ~mimi_hip_linear_s() {
    for (int k = 0; k < 2; ++k) {
      if (column_host[k]) (void)hipHostFree(column_host[k]);
      if (column_ready[k]) (void)hipEventDestroy(column_ready[k]);
    }
  }
};

namespace {

const dim3 KR_GRID(KR_BLOCKS), KR_BLOCK(KR_THREADS);   // of every reduction and vector kernel

// The product form of the pattern, found at create (kr_groups_kernel, kr_nodecol_kernel): the one switch over it.
// f(ROWS, NODECOL, units of ROWS rows, the column list the form reads)
template<class F>
void by_product_form(const mimi_hip_linear_s* h, F&& f) {
  using std::integral_constant;
  if (h->nodecol) f(integral_constant<int, 3>{}, std::true_type{}, h->n / 3, (const int32_t*)h->ncol.ptr);
  else if (h->group == 3) f(integral_constant<int, 3>{}, std::false_type{}, h->n / 3, h->col);
  else if (h->group == 2) f(integral_constant<int, 2>{}, std::false_type{}, h->n / 2, h->col);
  else f(integral_constant<int, 1>{}, std::false_type{}, h->n, h->col);
}

// the handle of a boundary term by its kind: the one switch over it.  f(handle)
template<class F>
void by_boundary_kind(const mimi_hip_linear_s::BoundaryTerm& t, F&& f) {
  if (t.kind == MIMI_HIP_BOUNDARY_CONTACT) f(static_cast<mimi_hip_contact_s*>(t.handle));
  else f(static_cast<mimi_hip_pressure_s*>(t.handle));
}

// the components per node of a fold (1 to 3: mimi_hip_fold_create), a compile-time divisor of its two kernels.  f(DIM)
template<class F>
void by_fold_dim(int dim, F&& f) {
  using std::integral_constant;
  if (dim == 3) f(integral_constant<int, 3>{});
  else if (dim == 2) f(integral_constant<int, 2>{});
  else f(integral_constant<int, 1>{});
}

dim3 wave_per_unit(int64_t units) { return dim3((unsigned)((units + 3) / 4)); }   // workgroups of 256: four waves

// y = dinv o (A x), dinv o (b - A x) with b, plain without dinv.  val == nullptr: A is the handle's operator,
// y = mask(A (mask x)) + x[ess] (dinv then comes from the operator's diagonal)
void spmv(mimi_hip_linear_s* h, const double* val, const double* x, const double* b, const double* dinv, double* y) {
  if (!val) {
    const unsigned char* is_ess = h->is_ess.ptr;
    // the actions' vectors: the solver's own, or with a fold the unwrapped scratch between the fold's two kernels
    const double* ax = h->op_fold ? h->op_xu.ptr : h->op_x.ptr;
    double* ay = h->op_fold ? h->op_yu.ptr : y;
    OperatorFold f{};
    if (h->op_fold) {
      f = operator_fold(h->op_fold);
      by_fold_dim(f.dim, [&](auto D) {
        launch(kr_operator_mask_expand_kernel<decltype(D)::value>, KR_GRID, KR_BLOCK, 0, h->stream, f.n_nodes_u * f.dim, f.node_map,
               is_ess, x, h->op_xu.ptr, h->op_yu.ptr);
      });
    } else {
      launch(kr_operator_mask_kernel, KR_GRID, KR_BLOCK, 0, h->stream, h->n, is_ess, x, h->op_x.ptr, y);
    }
    operator_add_action(h->op_domain, h->op_density, h->op_stiffness, h->op_viscosity, ax, ay, h->stream);
    for (int k = 0; k < h->n_op_terms; ++k)
      by_boundary_kind(h->op_terms[k], [&](auto* face) { operator_add_action(face, h->op_terms[k].factor, ax, ay, h->stream); });
    if (h->op_fold) {
      by_fold_dim(f.dim, [&](auto D) {
        launch(kr_operator_fold_restore_kernel<decltype(D)::value>, KR_GRID, KR_BLOCK, 0, h->stream, h->n, f.copy_ptr, f.copies, is_ess, x,
               b, dinv, (const double*)h->op_yu.ptr, y);
      });
    } else {
      launch(kr_operator_restore_kernel, KR_GRID, KR_BLOCK, 0, h->stream, h->n, is_ess, x, b, dinv, y);
    }
    return;
  }
  by_product_form(h, [&](auto R, auto NC, int64_t n_units, const int32_t* col) {
    launch(kr_spmv_kernel<decltype(R)::value, decltype(NC)::value>, wave_per_unit(n_units), dim3(256), 0, h->stream, n_units, h->rowptr,
           col, val, x, b, dinv, y);
  });
}

// partial_out = the partial sums of a . b (a == b: of the squared norm)
void dot(mimi_hip_linear_s* h, const double* a, const double* b, double* partial_out) {
  launch(kr_mgs_kernel, KR_GRID, KR_BLOCK, 0, h->stream, h->n, const_cast<double*>(a), nullptr, nullptr, b, partial_out);
}

// the scalar behind the first partial array of the handle, on the host
double total_to_host(mimi_hip_linear_s* h) {
  launch(kr_totals_kernel, dim3(1), KR_BLOCK, 0, h->stream, h->partials.ptr, h->totals.ptr);
  double t = 0.0;
  MH_HIP(hipMemcpyAsync(&t, h->totals.ptr, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  MH_HIP(hipStreamSynchronize(h->stream));
  return t;
}

// d = the diagonal (block == 0: n doubles) or the node blocks (block != 0: n dim doubles) of the handle's operator in the
// solver's numbering, on the solver's stream; solve_matrix has run.  The boundary terms contribute nothing (header comment).
void operator_diagonal(mimi_hip_linear_s* h, int block, double* d) {
  const int dim = operator_dim(h->op_domain);
  const int nc = block ? dim * dim : dim;
  operator_begin_diagonal(h->op_domain, h->op_density, h->op_stiffness, block, h->stream);
  MH_HIP(hipSetDevice(h->device));
  if (h->op_fold) {
    const OperatorFold f = operator_fold(h->op_fold);
    if (f.dim != dim) fail("operator diagonal: the fold has %d components per node, the domain handle %d", f.dim, dim);
    const size_t n_u = (size_t)f.n_nodes_u * nc;
    h->op_du.resize(n_u);
    MH_HIP(hipMemsetAsync(h->op_du.ptr, 0, n_u * sizeof(double), h->stream));
    operator_add_diagonal(h->op_domain, h->op_density, h->op_stiffness, h->op_viscosity, block, h->op_du.ptr, h->stream);
    launch(kr_fold_sum_kernel, dim3((unsigned)((f.n_nodes_f * nc + 255) / 256)), dim3(256), 0, h->stream, f.n_nodes_f, nc, f.copy_ptr,
           f.copies, (const double*)h->op_du.ptr, d);
  } else {
    MH_HIP(hipMemsetAsync(d, 0, (size_t)(h->n / dim) * nc * sizeof(double), h->stream));
    operator_add_diagonal(h->op_domain, h->op_density, h->op_stiffness, h->op_viscosity, block, d, h->stream);
  }
}

// M of one solve: the identity, 1 / diag(A) of THIS solve's values (mfem::DSmoother; the values change between Newton
// iterations, so nothing of it outlives the solve) or of the operator (armed, no values), the Kronecker operator the handle
// holds, or the inverted node blocks of this solve's values or operator.  Which kernels apply M is decided here and nowhere
// else.
struct Preconditioner {
  mimi_hip_linear_s* h;
  int id;
  const double* dinv = nullptr;   // Jacobi; fused into the kernels that take it

  Preconditioner(mimi_hip_linear_s* h_, int id_, const double* val) : h(h_), id(id_) {
    if (id < MIMI_HIP_PRECOND_NONE || id > MIMI_HIP_PRECOND_BLOCK_JACOBI)
      fail("unknown preconditioner id %d (0 none, 1 Jacobi, 2 Kronecker, 3 node-block Jacobi)", id);
    if (id == MIMI_HIP_PRECOND_KRONECKER) {
      if (!h->kron.set) fail("preconditioner id 2 (Kronecker) needs mimi_hip_linear_set_kronecker first");
      if (!h->kron.have_coefficients) fail("preconditioner id 2 (Kronecker) needs mimi_hip_linear_set_kronecker_coefficients first");
    } else if (id == MIMI_HIP_PRECOND_JACOBI) {
      if (!val && !(h->op_diagonal && h->op_domain)) fail("the Jacobi preconditioner needs the matrix values");
      h->dinv.resize((size_t)h->n);
      const dim3 grid((unsigned)((h->n + 255) / 256));
      if (val) {
        launch(kr_diag_kernel, grid, dim3(256), 0, h->stream, h->n, h->rowptr, h->diag_pos.ptr, val, h->dinv.ptr);
      } else {
        operator_diagonal(h, 0, h->dinv.ptr);
        reset_bad();
        launch(kr_operator_dinv_kernel, grid, dim3(256), 0, h->stream, h->n, (const unsigned char*)h->is_ess.ptr, h->dinv.ptr,
               h->bad_node.ptr);
        const unsigned long long bad = read_bad();
        if (bad != ~0ull)
          fail("Jacobi from the operator's diagonal: the diagonal entry of dof %llu is zero or not finite", bad);
      }
      dinv = h->dinv.ptr;
    } else if (id == MIMI_HIP_PRECOND_BLOCK_JACOBI) {
      build_blocks(val);
    }
  }

  // the one word a build of M reports its first bad node or dof in: all ones before, read back once per solve
  void reset_bad() const {
    h->bad_node.resize(1);
    MH_HIP(hipMemsetAsync(h->bad_node.ptr, 0xff, sizeof(unsigned long long), h->stream));
  }
  unsigned long long read_bad() const {
    unsigned long long bad = 0;
    MH_HIP(hipMemcpyAsync(&bad, h->bad_node.ptr, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    MH_HIP(hipStreamSynchronize(h->stream));
    return bad;
  }

  // the inverted node blocks of this solve into h->binv
  void build_blocks(const double* val) const {
    const int dim = h->node_block;
    if (!dim) fail("preconditioner id 3 (node-block Jacobi) needs mimi_hip_linear_set_node_block first");
    const int64_t n_nodes = h->n / dim;
    const dim3 grid((unsigned)((h->n * dim + 255) / 256));
    h->binv.resize((size_t)h->n * dim);
    if (val) {
      if (!h->have_block_pos) {
        h->block_pos.resize((size_t)h->n * dim);
        launch(kr_block_pos_kernel, grid, dim3(256), 0, h->stream, h->n, dim, h->rowptr, h->col, h->block_pos.ptr);
        h->have_block_pos = true;
      }
      launch(kr_block_values_kernel, grid, dim3(256), 0, h->stream, h->n, dim, h->rowptr, (const int64_t*)h->block_pos.ptr, val,
             h->binv.ptr);
    } else {
      if (!h->op_domain) fail("the node-block Jacobi preconditioner needs the matrix values or an operator");
      if (operator_dim(h->op_domain) != dim)
        fail("node-block Jacobi: the operator's domain has %d components per node, mimi_hip_linear_set_node_block gave %d",
             operator_dim(h->op_domain), dim);
      operator_diagonal(h, 1, h->binv.ptr);
    }
    reset_bad();
    by_fold_dim(dim, [&](auto D) {
      launch(kr_block_invert_kernel<decltype(D)::value>, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, h->stream, n_nodes,
             (const unsigned char*)h->is_ess.ptr, h->binv.ptr, h->bad_node.ptr);
    });
    const unsigned long long bad = read_bad();
    if (bad != ~0ull) fail("node-block Jacobi: the block of node %llu is singular or not finite", bad);
  }

  // z_A = B_A^-1 r_A  (z == r allowed)
  void blocks(const double* r, double* z, double* partial_rz) const {
    by_fold_dim(h->node_block, [&](auto D) {
      launch(kr_block_apply_kernel<decltype(D)::value>, KR_GRID, KR_BLOCK, 0, h->stream, h->n / h->node_block, (const double*)h->binv.ptr, r,
             z, partial_rz);
    });
  }

  // z = P^-1 r, z[ess] = r[ess]  (z == r allowed)
  void kronecker(const double* r, double* z) const { h->kron.apply(r, z, h->n_ess > 0 ? h->is_ess.ptr : nullptr, h->stream); }

  // y = M (b - A x), or M A x without b: Jacobi inside the product, the Kronecker operator or the node blocks in place
  // behind a plain one
  void product(const double* val, const double* x, const double* b, double* y) const {
    spmv(h, val, x, b, dinv, y);
    if (id == MIMI_HIP_PRECOND_KRONECKER) kronecker(y, y);
    else if (id == MIMI_HIP_PRECOND_BLOCK_JACOBI) blocks(y, y, nullptr);
  }

  // z = M r, and the partial sums of r . z into partial_rz when the caller wants them
  void apply(const double* r, double* z, double* partial_rz) const {
    if (id == MIMI_HIP_PRECOND_KRONECKER) {
      kronecker(r, z);
      if (partial_rz) dot(h, z, r, partial_rz);
      return;
    }
    if (id == MIMI_HIP_PRECOND_BLOCK_JACOBI) {
      blocks(r, z, partial_rz);
      return;
    }
    if (!partial_rz) {   // (the fused kernel writes them always)
      h->partials.resize((size_t)KR_BLOCKS);
      partial_rz = h->partials.ptr;
    }
    launch(kr_cg_precond_kernel, KR_GRID, KR_BLOCK, 0, h->stream, h->n, r, dinv, z, partial_rz);
  }
};

// the matrix of one solve: the caller's values, or (none given) the operator of the handle, made ready for this solve
Mirror<double> solve_matrix(mimi_hip_linear_s* h, const double* A_values, int preconditioner) {
  if (A_values) return Mirror<double>::in(A_values, (size_t)h->nnz, h->stage_val, h->stream);
  if (!h->op_domain) fail("null argument (no matrix values, and no operator is set: mimi_hip_linear_set_operator)");
  if (preconditioner == MIMI_HIP_PRECOND_JACOBI && !h->op_diagonal) fail("the Jacobi preconditioner needs the matrix values");
  if (h->op_fold) {
    // (set_operator_fold and set_operator checked these against what was set then; either may have changed since)
    const OperatorFold f = operator_fold(h->op_fold);
    if (f.n_nodes_f * f.dim != h->n)
      fail("operator fold: the fold has %lld folded dofs, the solver %lld", (long long)(f.n_nodes_f * f.dim), (long long)h->n);
    h->op_xu.resize((size_t)(f.n_nodes_u * f.dim));
    h->op_yu.resize((size_t)(f.n_nodes_u * f.dim));
  } else {
    h->op_x.resize((size_t)h->n);
  }
  if (operator_size(h->op_domain) != h->operator_n())
    fail("operator: the domain handle has %lld dofs, the %s %lld", (long long)operator_size(h->op_domain),
         h->op_fold ? "unwrapped side of the operator fold" : "solver", (long long)h->operator_n());
  for (int k = 0; k < h->n_op_terms; ++k)
    by_boundary_kind(h->op_terms[k], [&](auto* face) {
      if (operator_size(face) != h->operator_n())
        fail("boundary operator: the handle has %lld dofs, the %s %lld", (long long)operator_size(face),
             h->op_fold ? "unwrapped side of the operator fold" : "solver", (long long)h->operator_n());
    });
  operator_begin_solve(h->op_domain, h->op_density, h->op_stiffness, h->stream);
  for (int k = 0; k < h->n_op_terms; ++k)
    by_boundary_kind(h->op_terms[k], [&](auto* face) { operator_begin_solve(face, h->stream); });
  MH_HIP(hipSetDevice(h->device));
  return Mirror<double>{};
}

// every exit of a solve: what it reports, and x back to a caller on the host
struct SolveExit {
  mimi_hip_linear_s* h;
  Mirror<double>& x;
  int32_t* iterations;
  double* final_norm;
  int32_t* converged;
  void operator()(int it, double nrm, bool conv) const {
    if (iterations) *iterations = it;
    if (final_norm) *final_norm = nrm;
    if (converged) *converged = conv ? 1 : 0;
    x.finish(h->stream);
    MH_HIP(hipStreamSynchronize(h->stream));
  }
};

// the status word of create after the checks launched so far
int read_status(mimi_hip_linear_s* h) {
  int status = 0;
  MH_HIP(hipMemcpyAsync(&status, h->status.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MH_HIP(hipStreamSynchronize(h->stream));
  return status;
}

}  // namespace

extern "C" {

int mimi_hip_linear_create(int64_t n, const int64_t* csr_rowptr, const int32_t* csr_col, const int64_t* ess_dofs,
                           int64_t n_ess, int device, mimi_hip_linear_t* out) {
  return guarded([&] {
    if (!out || !csr_rowptr || !csr_col || n < 1) fail("null / empty argument");
    auto h = std::make_unique<mimi_hip_linear_s>();
    h->open(device);
    h->n = n;
    if (is_device_pointer(csr_rowptr)) {
      h->rowptr = csr_rowptr;
    } else {
      h->rowptr_own.assign(csr_rowptr, (size_t)n + 1, h->stream);
      h->rowptr = h->rowptr_own.ptr;
    }
    int64_t nnz = 0;
    MH_HIP(hipMemcpy(&nnz, h->rowptr + n, sizeof(int64_t), hipMemcpyDeviceToHost));
    h->nnz = nnz;
    if (is_device_pointer(csr_col)) {
      h->col = csr_col;
    } else {
      h->col_own.assign(csr_col, (size_t)nnz, h->stream);
      h->col = h->col_own.ptr;
    }
    h->status.resize(1);
    MH_HIP(hipMemsetAsync(h->status.ptr, 0, sizeof(int), h->stream));
    h->diag_pos.resize((size_t)n);
    launch(kr_diag_pos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, h->rowptr, h->col, h->diag_pos.ptr,
           h->status.ptr);
    if (read_status(h.get())) fail("CSR pattern has a row without a diagonal entry");
    // the dofs of a node (byVDIM numbering) have identical rows in the pattern the integrators assemble into
    for (int g = 3; g >= 2; --g)
      if (n % g == 0)
        launch(kr_groups_kernel, wave_per_unit(n), dim3(256), 0, h->stream, n, g, h->rowptr, h->col, 1 << g, h->status.ptr);
    const int status = read_status(h.get());
    h->group = (n % 3 == 0 && !(status & 8)) ? 3 : (n % 2 == 0 && !(status & 4)) ? 2 : 1;
    if (h->group == 3 && nnz % 9 == 0) {
      launch(kr_nodecol_kernel, wave_per_unit(n / 3), dim3(256), 0, h->stream, n / 3, h->rowptr, h->col, 16, h->status.ptr, nullptr);
      if (!(read_status(h.get()) & 16)) {
        h->ncol.resize((size_t)(nnz / 9));
        launch(kr_nodecol_kernel, wave_per_unit(n / 3), dim3(256), 0, h->stream, n / 3, h->rowptr, h->col, 16, h->status.ptr, h->ncol.ptr);
        h->nodecol = true;
      }
    }
    h->is_ess.resize((size_t)n);
    MH_HIP(hipMemsetAsync(h->is_ess.ptr, 0, (size_t)n, h->stream));
    h->n_ess = n_ess;
    if (n_ess > 0) {
      if (!ess_dofs) fail("null essential dof list");
      h->ess.assign(ess_dofs, (size_t)n_ess, h->stream);
      launch(kr_mark_kernel, dim3((unsigned)((n_ess + 255) / 256)), dim3(256), 0, h->stream, n_ess, h->ess.ptr, h->is_ess.ptr);
    }
    MH_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
  });
}

int mimi_hip_linear_destroy(mimi_hip_linear_t h) { return handle_destroy(h); }
int mimi_hip_linear_set_stream(mimi_hip_linear_t h, void* stream) { return handle_set_stream(h, stream); }

int64_t mimi_hip_linear_info(mimi_hip_linear_t h, int what) {
  if (!h) return -1;
  switch (what) {
    case MIMI_HIP_LINEAR_INFO_ROWS: return h->n;
    case MIMI_HIP_LINEAR_INFO_NNZ: return h->nnz;
    case MIMI_HIP_LINEAR_INFO_ROW_GROUP: return h->group;
    case MIMI_HIP_LINEAR_INFO_NODE_COLUMNS: return h->nodecol ? 1 : 0;
    default: return -1;
  }
}

int mimi_hip_linear_eliminate(mimi_hip_linear_t h, double* r, double* A_values) {
  return guarded([&] {
    if (!h) fail("null handle");
    MH_HIP(hipSetDevice(h->device));
    if (h->n_ess == 0) return;
    if (r) {
      Mirror<double> mr = Mirror<double>::inout(r, (size_t)h->n, h->stage_b, h->stream);
      launch(kr_zero_entries_kernel, dim3((unsigned)((h->n_ess + 255) / 256)), dim3(256), 0, h->stream, h->n_ess, h->ess.ptr, mr.dev);
      mr.finish(h->stream);
      if (mr.host) MH_HIP(hipStreamSynchronize(h->stream));
    }
    if (A_values) {
      Mirror<double> mA = Mirror<double>::inout(A_values, (size_t)h->nnz, h->stage_val, h->stream);
      launch(kr_eliminate_kernel, wave_per_unit(h->n), dim3(256), 0, h->stream, h->n, h->rowptr, h->col, h->is_ess.ptr, mA.dev);
      mA.finish(h->stream);
      if (mA.host) MH_HIP(hipStreamSynchronize(h->stream));
    }
  });
}

int mimi_hip_linear_add_mult(mimi_hip_linear_t h, const double* A_values, const double* x, double alpha, double* y) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (!A_values || !x || !y) fail("null vector argument");
    MH_HIP(hipSetDevice(h->device));
    Mirror<double> mA = Mirror<double>::in(A_values, (size_t)h->nnz, h->stage_val, h->stream);
    Mirror<double> mx = Mirror<double>::in(x, (size_t)h->n, h->stage_x, h->stream);
    Mirror<double> my = Mirror<double>::inout(y, (size_t)h->n, h->stage_b, h->stream);
    by_product_form(h, [&](auto R, auto NC, int64_t n_units, const int32_t* col) {
      launch(kr_add_mult_kernel<decltype(R)::value, decltype(NC)::value>, wave_per_unit(n_units), dim3(256), 0, h->stream, n_units,
             h->rowptr, col, mA.dev, mx.dev, alpha, my.dev);
    });
    my.finish(h->stream);
    if (mA.host || mx.host || my.host) MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_linear_gmres(mimi_hip_linear_t h, const double* A_values, const double* b, double* x, double rel_tol, double abs_tol,
                          int max_iter, int kdim, int preconditioner, int32_t* iterations, double* final_norm, int32_t* converged) {
  return guarded([&] {
    if (!h || !b || !x) fail("null argument");
    if (kdim < 1) kdim = 50;   // mfem::GMRESSolver default m
    MH_HIP(hipSetDevice(h->device));
    const int64_t n = h->n;
    hipStream_t s = h->stream;
    Mirror<double> mA = solve_matrix(h, A_values, preconditioner);
    Mirror<double> mb = Mirror<double>::in(b, (size_t)n, h->stage_b, s);
    Mirror<double> mx = Mirror<double>::inout(x, (size_t)n, h->stage_x, s);   // overwritten: iterative_mode == false
    h->V.resize((size_t)(kdim + 1) * n);
    h->w.resize((size_t)n);
    h->r.resize((size_t)n);
    h->partials.resize((size_t)(kdim + 2) * KR_BLOCKS);
    h->totals.resize((size_t)(kdim + 2));
    h->ycoef.resize((size_t)kdim);
    h->reserve_columns(kdim + 2);
    const Preconditioner M(h, preconditioner, mA.dev);
    const SolveExit finish{h, mx, iterations, final_norm, converged};
    double* V = h->V.ptr;
    double* w = h->w.ptr;
    double* r = h->r.ptr;
    double* part = h->partials.ptr;
    GmresLeastSquares ls(kdim);
    auto norm_of_r = [&]() -> double {   // its partial sums stay in part[0..) for the normalisation that follows
      dot(h, r, r, part);
      return std::sqrt(total_to_host(h));
    };
    auto update = [&](int k_count) {   // GMRESSolver: Update(x, k, H, s, v)
      MH_HIP(hipMemcpyAsync(h->ycoef.ptr, ls.solve(k_count), sizeof(double) * k_count, hipMemcpyHostToDevice, s));
      launch(kr_update_kernel, KR_GRID, KR_BLOCK, 0, s, n, k_count, V, n, h->ycoef.ptr, mx.dev);
      MH_HIP(hipStreamSynchronize(s));   // y is host memory reused by the next cycle
    };

    // x = 0; r = M (b - A x)
    MH_HIP(hipMemsetAsync(mx.dev, 0, sizeof(double) * n, s));
    M.product(mA.dev, mx.dev, mb.dev, r);
    double beta = norm_of_r();
    const double goal = std::fmax(rel_tol * beta, abs_tol);
    if (beta <= goal) {
      finish(0, beta, true);
      return;
    }
    // One Arnoldi step on the stream: w = M A v_i, the i + 2 modified Gram-Schmidt stages (stage k subtracts
    // h_{k-1} v_{k-1} and forms h_k = w . v_k; the last one forms ||w||^2), v_{i+1}, and the Hessenberg column into
    // pinned host memory.  Nothing here waits for the host, so step i + 1 is launched BEFORE the host reads column i:
    // the round trip of the column is hidden behind the next step, and when column i ends the solve the step that was
    // launched ahead is simply not used (the update reads v_0 .. v_i only).
    auto launch_step = [&](int i) {
      M.product(mA.dev, V + (int64_t)i * n, nullptr, w);
      for (int k = 0; k <= i + 1; ++k) {
        const double* v_prev = k > 0 ? V + (int64_t)(k - 1) * n : nullptr;
        const double* p_prev = k > 0 ? part + (int64_t)(k - 1) * KR_BLOCKS : nullptr;
        const double* v_next = k <= i ? V + (int64_t)k * n : w;
        launch(kr_mgs_kernel, KR_GRID, KR_BLOCK, 0, s, n, w, v_prev, p_prev, v_next, part + (int64_t)k * KR_BLOCKS);
      }
      launch(kr_normalize_kernel, KR_GRID, KR_BLOCK, 0, s, n, w, part + (int64_t)(i + 1) * KR_BLOCKS, V + (int64_t)(i + 1) * n);
      launch(kr_totals_kernel, dim3(i + 2), KR_BLOCK, 0, s, part, h->totals.ptr);
      MH_HIP(hipMemcpyAsync(h->column_host[i & 1], h->totals.ptr, sizeof(double) * (i + 2), hipMemcpyDeviceToHost, s));
      MH_HIP(hipEventRecord(h->column_ready[i & 1], s));
    };
    int j = 1;
    while (j <= max_iter) {
      // v_0 = r / beta (partials of ||r||^2 are in part[0..))
      launch(kr_normalize_kernel, KR_GRID, KR_BLOCK, 0, s, n, r, part, V);
      ls.start_cycle(beta);
      const int steps = std::min(kdim, max_iter - j + 1);   // of this cycle, unless one of them converges
      launch_step(0);
      int i = 0;
      for (; i < steps; ++i, ++j) {
        if (i + 1 < steps) launch_step(i + 1);
        MH_HIP(hipEventSynchronize(h->column_ready[i & 1]));
        const double resid = ls.push_column(i, h->column_host[i & 1]);
        if (resid <= goal) {
          update(i + 1);
          finish(j, resid, true);
          return;
        }
      }
      update(i);
      M.product(mA.dev, mx.dev, mb.dev, r);
      beta = norm_of_r();
      if (beta <= goal) {
        finish(j - 1, beta, true);
        return;
      }
    }
    finish(max_iter, beta, false);
  });
}

/* mfem::CGSolver + mfem::DSmoother as operators::NonlinearSolid configures its mass solve (operators/nonlinear_solid.cpp:
 * 39-50, .hpp:38-42: rel 1e-8, abs 1e-12, 1000 iterations, iterative_mode false): preconditioned conjugate gradients,
 * stops when (r, M r) <= max(rel_tol^2 (r0, M r0), abs_tol^2)  (mfem linalg/solvers.cpp, CGSolver::Mult) */
int mimi_hip_linear_cg(mimi_hip_linear_t h, const double* A_values, const double* b, double* x, double rel_tol, double abs_tol,
                       int max_iter, int preconditioner, int32_t* iterations, double* final_norm, int32_t* converged) {
  return guarded([&] {
    if (!h || !b || !x) fail("null argument");
    MH_HIP(hipSetDevice(h->device));
    const int64_t n = h->n;
    hipStream_t s = h->stream;
    Mirror<double> mA = solve_matrix(h, A_values, preconditioner);
    Mirror<double> mb = Mirror<double>::in(b, (size_t)n, h->stage_b, s);
    Mirror<double> mx = Mirror<double>::inout(x, (size_t)n, h->stage_x, s);
    h->V.resize((size_t)3 * n);            // d, z, q
    h->r.resize((size_t)n);
    h->partials.resize((size_t)2 * KR_BLOCKS);
    h->totals.resize(2);
    const Preconditioner M(h, preconditioner, mA.dev);
    const SolveExit report{h, mx, iterations, final_norm, converged};
    auto finish = [&](int it, double nom, bool conv) { report(it, std::sqrt(std::fabs(nom)), conv); };   // reports sqrt|(r, M r)|
    double* d = h->V.ptr;
    double* z = d + n;
    double* q = z + n;
    double* r = h->r.ptr;
    double* part = h->partials.ptr;
    // x = 0, r = b, z = M r, d = z
    MH_HIP(hipMemsetAsync(mx.dev, 0, sizeof(double) * n, s));
    MH_HIP(hipMemcpyAsync(r, mb.dev, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    M.apply(r, z, part);
    MH_HIP(hipMemcpyAsync(d, z, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    double nom = total_to_host(h);
    const double r0 = std::fmax(nom * rel_tol * rel_tol, abs_tol * abs_tol);
    if (nom <= r0) {
      finish(0, nom, true);
      return;
    }
    spmv(h, mA.dev, d, nullptr, nullptr, q);
    dot(h, q, d, part);
    double den = total_to_host(h);
    if (!(den > 0.0)) {   // not positive definite: mfem warns and stops
      finish(0, nom, false);
      return;
    }
    int it = 1;
    for (;; ++it) {
      const double alpha = nom / den;
      launch(kr_cg_update_kernel, KR_GRID, KR_BLOCK, 0, s, n, alpha, d, q, mx.dev, r);
      M.apply(r, z, part);
      const double betanom = total_to_host(h);
      if (betanom <= r0) {
        finish(it, betanom, true);
        return;
      }
      if (it >= max_iter) {
        finish(it, betanom, false);
        return;
      }
      const double beta = betanom / nom;
      launch(kr_cg_direction_kernel, KR_GRID, KR_BLOCK, 0, s, n, beta, z, d);
      spmv(h, mA.dev, d, nullptr, nullptr, q);
      dot(h, q, d, part);
      den = total_to_host(h);
      if (!(den > 0.0)) {
        finish(it, betanom, false);
        return;
      }
      nom = betanom;
    }
  });
}

int mimi_hip_linear_set_kronecker(mimi_hip_linear_t h, int32_t dim, const int32_t* n_dir, const double* U, const double* lambda) {
  return guarded([&] {
    if (!h || !n_dir || !U || !lambda) fail("null argument");
    if (dim != 2 && dim != 3) fail("Kronecker preconditioner: dim %d (2 or 3)", dim);
    int64_t n = dim;
    for (int d = 0; d < dim; ++d) {
      if (n_dir[d] < 1) fail("Kronecker preconditioner: %d nodes along axis %d", n_dir[d], d);
      n *= n_dir[d];
    }
    if (n != h->n)
      fail("Kronecker preconditioner: a grid of %d x %d x %d nodes with %d components has %lld dofs, the handle has %lld", n_dir[0],
           n_dir[1], dim == 3 ? n_dir[2] : 1, dim, (long long)n, (long long)h->n);
    MH_HIP(hipSetDevice(h->device));
    h->kron.assign(dim, n_dir, U, lambda, h->stream);
    MH_HIP(hipStreamSynchronize(h->stream));
  });
}

int mimi_hip_linear_set_kronecker_coefficients(mimi_hip_linear_t h, double mass_coef, const double* stiff_coef) {
  return guarded([&] {
    if (!h || !stiff_coef) fail("null argument");
    if (!h->kron.set) fail("mimi_hip_linear_set_kronecker_coefficients needs mimi_hip_linear_set_kronecker first");
    MH_HIP(hipSetDevice(h->device));
    KronCoefficients k{};
    k.mass = mass_coef;
    for (int e = 0; e < h->kron.dim * h->kron.dim; ++e) k.stiff[e] = stiff_coef[e];
    h->kron.set_coefficients(k, h->stream);
  });
}

int mimi_hip_linear_set_operator(mimi_hip_linear_t h, mimi_hip_domain_t domain, double density, double stiffness, double viscosity) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (domain) {
      if (operator_device(domain) != h->device)
        fail("operator: the domain handle is on device %d, the solver on device %d", operator_device(domain), h->device);
      if (operator_size(domain) != h->operator_n())
        fail("operator: the domain handle has %lld dofs, the %s %lld", (long long)operator_size(domain),
             h->op_fold ? "unwrapped side of the operator fold" : "solver", (long long)h->operator_n());
    }
    h->op_domain = domain;
    h->op_density = density;
    h->op_stiffness = stiffness;
    h->op_viscosity = viscosity;
    h->n_op_terms = 0;   // the boundary terms belong to the setting they were added to
  });
}

int mimi_hip_linear_add_boundary_operator(mimi_hip_linear_t h, int kind, void* handle, double factor) {
  return guarded([&] {
    if (!h || !handle) fail("null argument");
    if (kind != MIMI_HIP_BOUNDARY_CONTACT && kind != MIMI_HIP_BOUNDARY_PRESSURE) fail("boundary operator kind %d (0 contact, 1 pressure)", kind);
    if (!h->op_domain) fail("boundary operator: no domain operator is set (mimi_hip_linear_set_operator comes first)");
    if (h->n_op_terms >= mimi_hip_linear_s::kMaxBoundaryTerms)
      fail("boundary operator: at most %d terms", mimi_hip_linear_s::kMaxBoundaryTerms);
    const mimi_hip_linear_s::BoundaryTerm term{kind, handle, factor};
    by_boundary_kind(term, [&](auto* face) {
      if (operator_device(face) != h->device)
        fail("boundary operator: the handle is on device %d, the solver on device %d", operator_device(face), h->device);
      if (operator_size(face) != h->operator_n())
        fail("boundary operator: the handle has %lld dofs, the %s %lld", (long long)operator_size(face),
             h->op_fold ? "unwrapped side of the operator fold" : "solver", (long long)h->operator_n());
    });
    h->op_terms[h->n_op_terms++] = term;
  });
}

int mimi_hip_linear_set_operator_fold(mimi_hip_linear_t h, mimi_hip_fold_t fold) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (fold) {
      if (operator_device(fold) != h->device)
        fail("operator fold: the fold is on device %d, the solver on device %d", operator_device(fold), h->device);
      const OperatorFold f = operator_fold(fold);
      if (f.n_nodes_f * f.dim != h->n)
        fail("operator fold: the fold has %lld folded dofs (%lld nodes x %d), the solver %lld", (long long)(f.n_nodes_f * f.dim),
             (long long)f.n_nodes_f, f.dim, (long long)h->n);
    }
    h->op_fold = fold;   // (the operator and its boundary terms stay: a solve checks their size against the new setting)
  });
}

int mimi_hip_linear_set_node_block(mimi_hip_linear_t h, int32_t dim) {
  return guarded([&] {
    if (!h) fail("null handle");
    if (dim < 1 || dim > 3) fail("node block: dim %d (1 to 3)", dim);
    if (h->n % dim != 0) fail("node block: the handle's %lld dofs are no multiple of dim %d", (long long)h->n, dim);
    if (h->node_block != dim) h->have_block_pos = false;
    h->node_block = dim;
  });
}

int mimi_hip_linear_set_operator_diagonal(mimi_hip_linear_t h, int32_t on) {
  return guarded([&] {
    if (!h) fail("null handle");
    h->op_diagonal = on != 0;
  });
}

int mimi_hip_linear_operator_mult(mimi_hip_linear_t h, const double* x, double* y) {
  return guarded([&] {
    if (!h || !x || !y) fail("null argument");
    if (x == y) fail("operator product: x and y must be different vectors");
    MH_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    solve_matrix(h, nullptr, MIMI_HIP_PRECOND_NONE);
    Mirror<double> mx = Mirror<double>::in(x, (size_t)h->n, h->stage_x, s);
    Mirror<double> my;   // written whole: a host y has nothing to upload
    my.count = (size_t)h->n;
    if (is_device_pointer(y)) {
      my.dev = y;
    } else {
      h->stage_b.resize((size_t)h->n);
      my.dev = h->stage_b.ptr;
      my.host = y;
    }
    spmv(h, nullptr, mx.dev, nullptr, nullptr, my.dev);
    my.finish(s);
    if (mx.host || my.host) MH_HIP(hipStreamSynchronize(s));
  });
}

int mimi_hip_linear_apply_preconditioner(mimi_hip_linear_t h, int kind, const double* A_values, const double* r, double* z) {
  return guarded([&] {
    if (!h || !r || !z) fail("null argument");
    if (kind < MIMI_HIP_PRECOND_JACOBI || kind > MIMI_HIP_PRECOND_BLOCK_JACOBI) fail("preconditioner kind %d (1 Jacobi, 2 Kronecker, 3 node-block Jacobi)", kind);
    MH_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    Mirror<double> mr = Mirror<double>::in(r, (size_t)h->n, h->stage_b, s);
    Mirror<double> mz = Mirror<double>::inout(z, (size_t)h->n, h->stage_x, s);
    Mirror<double> mA;   // the values: the two Jacobis alone read them; without them theirs is the operator's diagonal
    if (kind != MIMI_HIP_PRECOND_KRONECKER) {
      if (A_values) mA = Mirror<double>::in(A_values, (size_t)h->nnz, h->stage_val, s);
      else if (h->op_domain && (kind == MIMI_HIP_PRECOND_BLOCK_JACOBI || h->op_diagonal)) solve_matrix(h, nullptr, kind);
    }
    const Preconditioner M(h, kind, mA.dev);
    M.apply(mr.dev, mz.dev, nullptr);
    mz.finish(s);
    if (mr.host || mz.host || mA.host) MH_HIP(hipStreamSynchronize(s));
  });
}

}  // extern "C"
