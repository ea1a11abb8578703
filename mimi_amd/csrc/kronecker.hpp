// Fast-diagonalisation (Kronecker) preconditioner of the device Krylov solvers (Sangalli & Tani): on one
// tensor-product patch  J = M + fac0 K (+ fac1 C)  is replaced, per displacement component c, by
//   P_c = rho (x)_d M_d + sum_d s_cd K_d (x) (M of the other axes),       P_c^-1 = (U_c0 (x) U_c1 (x) U_c2) D_c (...)^T,
// with the generalised eigenpairs  K_d U_cd = M_d U_cd diag(lambda_cd),  U_cd^T M_d U_cd = I  of the 1-D matrices (host,
// mimi_amd/kronecker.py) and  D_c[i0, i1, i2] = 1 / (rho + sum_d s_cd lambda_cd[i_d]).
//
// One application = a mode product per axis with U^T, the scaling, a mode product per axis with U: 2 dim passes over two
// ping-pong vectors.  Vectors are in the solver's byVDIM layout, index ((i2 n1 + i1) n0 + i0) vdim + c.  A pass along axis
// d is a batch of vdim GEMMs  Y[o][i'][q] = sum_i W_c[i][i'] X[o][i][q],  c = q % vdim, with q the contiguous index below
// the axis (`inner` = vdim prod_{e<d} n_e entries) and o the index above it; W = U (towards the eigenbasis) or U^T (back).
//   axis >= 1: a thread owns one (o, q) column and KQ_TI outputs i'; lanes run along q, so every load and store of a wave
//              is one contiguous run (two at an o boundary).                                  kq_mode_strided_kernel
//   axis 0:    inner = vdim, the line itself is contiguous with the components interleaved.  A workgroup stages KQ_LB
//              lines x KQ_KC nodes through LDS with whole-run loads (the vdim components come in with one read), thread
//              (line, c) contracts out of LDS, and the outputs go back through the same tile.  kq_mode_contiguous_kernel
// W is tiled through LDS in KQ_KC x KQ_TI pieces per component (it is 135 KB at n_d = 130), edges padded with zeros.  The
// sums run over i in increasing order in one thread: no atomics, equal bits from equal inputs.
// The scaling is fused into the store of the last pass towards the eigenbasis, z[ess] = r[ess] into the last pass back.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.hpp"

namespace mimi_hip {

constexpr int KQ_TI = 16;            // outputs i' per thread
constexpr int KQ_KC = 16;            // summands i per LDS tile of W
constexpr int KQ_UP = KQ_TI + 2;     // pitch of a (k, c) row of the W tile: the vdim rows a wave reads at once lie 36 banks apart
constexpr int KQ_THREADS = 128;      // kq_mode_strided_kernel
constexpr int KQ_LB = 32;            // lines per workgroup of kq_mode_contiguous_kernel (KQ_LB * vdim threads)

// what the store of a pass does on top of the product: v *= scale[idx]; v = fix[idx] where is_ess[idx] (each may be null)
struct KronEpilogue {
  const double* scale;
  const unsigned char* is_ess;
  const double* fix;   // may be the pass's own output (an application in place): every entry is read by the thread that writes it
};

__device__ __forceinline__ double kq_finish(double v, int64_t idx, const KronEpilogue& ep) {
  if (ep.scale) v *= ep.scale[idx];
  if (ep.is_ess && ep.is_ess[idx]) v = ep.fix[idx];
  return v;
}

// Ws[(kk VDIM + c) KQ_UP + t] = W_c[k0 + kk][i0 + t], zero outside the matrix
template<int VDIM, int NT>
__device__ __forceinline__ void kq_load_w_tile(int nd, int k0, int i0, const double* __restrict__ W, int64_t w_comp_stride,
                                               double* Ws) {
  for (int e = threadIdx.x; e < KQ_KC * VDIM * KQ_TI; e += NT) {
    const int t = e % KQ_TI, c = (e / KQ_TI) % VDIM, kk = e / (KQ_TI * VDIM);
    const int k = k0 + kk, i = i0 + t;
    Ws[(kk * VDIM + c) * KQ_UP + t] = (k < nd && i < nd) ? W[c * w_comp_stride + (int64_t)k * nd + i] : 0.0;
  }
}

// axis >= 1.  total = (entries of the vector) / nd columns (o, q), flattened as o * inner + q; grid (total / KQ_THREADS, nd / KQ_TI)
template<int VDIM>
__global__ __launch_bounds__(KQ_THREADS) void kq_mode_strided_kernel(int nd, int64_t inner, int64_t total, const double* __restrict__ W,
                                                                     int64_t w_comp_stride, const double* __restrict__ X, double* Y,
                                                                     KronEpilogue ep) {
  __shared__ double Ws[KQ_KC * VDIM * KQ_UP];
  const int64_t f = (int64_t)blockIdx.x * KQ_THREADS + threadIdx.x;
  const bool live = f < total;
  const int64_t o = live ? f / inner : 0, q = live ? f % inner : 0;
  const int c = (int)(q % VDIM);
  const int i0 = blockIdx.y * KQ_TI;
  const int64_t base = o * nd * inner + q;
  double acc[KQ_TI];
#pragma unroll
  for (int t = 0; t < KQ_TI; ++t) acc[t] = 0.0;
  for (int k0 = 0; k0 < nd; k0 += KQ_KC) {
    __syncthreads();   // the tile of the chunk before has been read
    kq_load_w_tile<VDIM, KQ_THREADS>(nd, k0, i0, W, w_comp_stride, Ws);
    double x[KQ_KC];
#pragma unroll
    for (int kk = 0; kk < KQ_KC; ++kk) x[kk] = (live && k0 + kk < nd) ? X[base + (int64_t)(k0 + kk) * inner] : 0.0;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KQ_KC; ++kk) {
      const double* u = Ws + (kk * VDIM + c) * KQ_UP;
#pragma unroll
      for (int t = 0; t < KQ_TI; ++t) acc[t] = __builtin_fma(u[t], x[kk], acc[t]);
    }
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < KQ_TI; ++t) {
    if (i0 + t < nd) {
      const int64_t idx = base + (int64_t)(i0 + t) * inner;
      Y[idx] = kq_finish(acc[t], idx, ep);
    }
  }
}

// axis 0.  A line = nd nodes x VDIM components, contiguous; grid (lines / KQ_LB, nd / KQ_TI), KQ_LB * VDIM threads: thread =
// line * VDIM + c.  The pitch of a line in the tile is = VDIM modulo 32, so the 32 lanes LDS serves together read 32 banks.
template<int VDIM>
__global__ __launch_bounds__(KQ_LB * VDIM) void kq_mode_contiguous_kernel(int nd, int64_t lines, const double* __restrict__ W,
                                                                          int64_t w_comp_stride, const double* __restrict__ X, double* Y,
                                                                          KronEpilogue ep) {
  static_assert(KQ_KC == KQ_TI, "the tile of the inputs is reused for the outputs");
  constexpr int NT = KQ_LB * VDIM;
  constexpr int SEG = KQ_KC * VDIM;                                // entries of a line per chunk
  constexpr int XP = SEG + ((VDIM - SEG % 32) % 32 + 32) % 32;     // 67 (vdim 3), 34 (vdim 2)
  __shared__ double Ws[KQ_KC * VDIM * KQ_UP];
  __shared__ double Xs[KQ_LB * XP];
  const int l = threadIdx.x / VDIM, c = threadIdx.x % VDIM;
  const int64_t line0 = (int64_t)blockIdx.x * KQ_LB;
  const int i0 = blockIdx.y * KQ_TI;
  const int64_t rowlen = (int64_t)nd * VDIM;
  double acc[KQ_TI];
#pragma unroll
  for (int t = 0; t < KQ_TI; ++t) acc[t] = 0.0;
  for (int k0 = 0; k0 < nd; k0 += KQ_KC) {
    __syncthreads();
    kq_load_w_tile<VDIM, NT>(nd, k0, i0, W, w_comp_stride, Ws);
    for (int e = threadIdx.x; e < KQ_LB * SEG; e += NT) {
      const int ll = e / SEG, s = e % SEG;
      const int64_t line = line0 + ll, pos = (int64_t)k0 * VDIM + s;
      Xs[ll * XP + s] = (line < lines && pos < rowlen) ? X[line * rowlen + pos] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KQ_KC; ++kk) {
      const double x = Xs[l * XP + kk * VDIM + c];
      const double* u = Ws + (kk * VDIM + c) * KQ_UP;
#pragma unroll
      for (int t = 0; t < KQ_TI; ++t) acc[t] = __builtin_fma(u[t], x, acc[t]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < KQ_TI; ++t) Xs[l * XP + t * VDIM + c] = acc[t];
  __syncthreads();
  for (int e = threadIdx.x; e < KQ_LB * SEG; e += NT) {
    const int ll = e / SEG, s = e % SEG;
    const int64_t line = line0 + ll, pos = (int64_t)i0 * VDIM + s;
    if (line < lines && pos < rowlen) {
      const int64_t idx = line * rowlen + pos;
      Y[idx] = kq_finish(Xs[ll * XP + s], idx, ep);
    }
  }
}

struct KronCoefficients {
  double mass;
  double stiff[9];   // [c * dim + d]
};

// D[(node, c)] = 1 / (mass + sum_d stiff[c][d] lambda_cd[i_d]); 0 where an index is a removed function (lambda < 0) or the
// sum is not positive
__global__ void kq_scaling_kernel(int64_t n, int dim, int n0, int n1, int n2, const double* __restrict__ lambda, KronCoefficients k,
                                  double* __restrict__ D) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int c = (int)(idx % dim);
  int64_t node = idx / dim;
  const int nd[3] = {n0, n1, n2};
  const int n_sum = n0 + n1 + (dim == 3 ? n2 : 0);
  double s = k.mass;
  bool removed = false;
  int off = 0;
  for (int d = 0; d < dim; ++d) {
    const int i = (int)(node % nd[d]);
    node /= nd[d];
    const double lam = lambda[c * n_sum + off + i];
    removed |= lam < 0.0;
    s += k.stiff[c * dim + d] * lam;
    off += nd[d];
  }
  D[idx] = (!removed && s > 0.0) ? 1.0 / s : 0.0;
}

// what a linear-solver handle keeps of the operator
struct Kronecker {
  bool set = false, have_coefficients = false;
  int dim = 0, nd[3] = {1, 1, 1};
  int64_t n = 0, u_comp_stride = 0;          // entries of U of one component: sum_d n_d^2
  int64_t u_off[3] = {0, 0, 0};              // of axis d inside a component
  DeviceBuffer<double> W_fwd, W_bwd, lambda, D, t0, t1;   // U, its transposes, ..., the two ping-pong vectors

  void assign(int dim_, const int32_t* n_dir, const double* U, const double* lam, hipStream_t s) {
    dim = dim_;
    n = dim;
    u_comp_stride = 0;
    int n_sum = 0;
    for (int d = 0; d < 3; ++d) {
      nd[d] = d < dim ? n_dir[d] : 1;
      if (d < dim) {
        u_off[d] = u_comp_stride;
        u_comp_stride += (int64_t)nd[d] * nd[d];
        n_sum += nd[d];
        n *= nd[d];
      }
    }
    const std::vector<double> Uh = to_host(U, (size_t)(dim * u_comp_stride));
    std::vector<double> Ut(Uh.size());
    for (int c = 0; c < dim; ++c)
      for (int d = 0; d < dim; ++d) {
        const double* a = Uh.data() + c * u_comp_stride + u_off[d];
        double* b = Ut.data() + c * u_comp_stride + u_off[d];
        for (int i = 0; i < nd[d]; ++i)
          for (int j = 0; j < nd[d]; ++j) b[(int64_t)j * nd[d] + i] = a[(int64_t)i * nd[d] + j];
      }
    // towards the eigenbasis  y[i'] = sum_i U[i][i'] x[i]  is the kernels' own form with W = U; back, W = U^T
    W_fwd.assign(Uh.data(), Uh.size(), s);
    W_bwd.assign(Ut.data(), Ut.size(), s);
    lambda.assign(lam, (size_t)(dim * n_sum), s);
    D.resize((size_t)n);
    t0.resize((size_t)n);
    t1.resize((size_t)n);
    set = true;
    have_coefficients = false;
  }

  void set_coefficients(const KronCoefficients& k, hipStream_t s) {
    launch(kq_scaling_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, dim, nd[0], nd[1], nd[2], lambda.ptr, k, D.ptr);
    have_coefficients = true;
  }

  template<int VDIM>
  void pass(int d, const double* W, const double* X, double* Y, const KronEpilogue& ep, hipStream_t s) const {
    const unsigned tiles = (unsigned)((nd[d] + KQ_TI - 1) / KQ_TI);
    if (d == 0) {
      const int64_t lines = n / ((int64_t)nd[0] * VDIM);
      launch(kq_mode_contiguous_kernel<VDIM>, dim3((unsigned)((lines + KQ_LB - 1) / KQ_LB), tiles), dim3(KQ_LB * VDIM), 0, s, nd[0], lines,
             W + u_off[0], u_comp_stride, X, Y, ep);
    } else {
      int64_t inner = VDIM;
      for (int e = 0; e < d; ++e) inner *= nd[e];
      const int64_t total = n / nd[d];
      launch(kq_mode_strided_kernel<VDIM>, dim3((unsigned)((total + KQ_THREADS - 1) / KQ_THREADS), tiles), dim3(KQ_THREADS), 0, s, nd[d],
             inner, total, W + u_off[d], u_comp_stride, X, Y, ep);
    }
  }

  // out = P^-1 in, then out[ess] = in[ess] (is_ess may be null).  out == in is allowed; neither may be t0 / t1.
  void apply(const double* in, double* out, const unsigned char* is_ess, hipStream_t s) const {
    if (!set) fail("the Kronecker preconditioner was asked for before mimi_hip_linear_set_kronecker");
    if (!have_coefficients) fail("the Kronecker preconditioner was asked for before mimi_hip_linear_set_kronecker_coefficients");
    const int passes = 2 * dim;
    const double* src = in;
    for (int p = 0; p < passes; ++p) {
      const bool forward = p < dim, last = p == passes - 1;
      const int d = forward ? p : passes - 1 - p;
      double* dst = last ? out : (p % 2 == 0 ? t0.ptr : t1.ptr);
      KronEpilogue ep{p == dim - 1 ? D.ptr : nullptr, last ? is_ess : nullptr, last ? in : nullptr};
      const double* W = forward ? W_fwd.ptr : W_bwd.ptr;
      if (dim == 3) pass<3>(d, W, src, dst, ep, s);
      else pass<2>(d, W, src, dst, ep, s);
      src = dst;
    }
  }
};

}  // namespace mimi_hip
