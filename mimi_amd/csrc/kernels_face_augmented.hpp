// Augmented-Lagrangian mortar contact: the nodal multipliers lambda_i <= 0 (the sign of the nodal pressure: compressive is
// negative) of a contact handle in the mode "augmented", and the Uzawa update.  The law, per marked node:
//   pass 1    the point gap enters the nodal sum UNCLAMPED: g_q = true_g, 0 where the angle rule (mortar_contact.cpp:172-181)
//             rejects the point; Gt_i = sum_q w |J| g_q N_i, gt_i = Gt_i / A_i     (contact_gap_area_kernel<DIM, true>)
//   pressure  p_i = min(0, lambda_i + eps gt_i): the clamp sits at the node      (contact_pressure_kernel<true>)
//   update    dlambda_i = p_i - lambda_i = min(-lambda_i, eps gt_i), then lambda_i <- p_i; KKT holds when every dlambda_i = 0
// Pass 2, the frozen tangent and its action, and the friction kernels read p_i and know nothing of the mode.  The consistent
// action differs in its record (unclamped g_q, chi_q = "the angle rule accepted the point") and in its nodal kernel,
//   dp_l = eps (dGt_l - gt_l dA_l) / A_l on the nodes with p_l < 0, 0 on the others,
// which are launch flags of contact_consistent_record_kernel and contact_consistent_nodal_kernel in
// kernels_face_consistent.hpp.  This header holds what only the mode needs:
//   update    one thread per marked node: p_i from lambda_i and the nodal sums of pass 1, the node's four numbers
//             A_i dlambda_i^2, [p_i < 0], |dlambda_i|, |lambda_i| afterwards; with apply, lambda_i <- p_i (a released node holds +0.0)
//   measure   ONE workgroup: every thread a fixed subset of the nodes, then a fixed-shape tree -- sums for the first two
//             numbers, maxima for the last two -- and out4 = max |dlambda| / eps, sqrt(sum A dlambda^2), count, max |lambda|
//   project   lambda_i <- min(lambda_i, 0) behind a set (a NaN becomes 0)
// No atomics, no LDS but the measure's tree: equal inputs give equal bytes.  No face wave is needed here: every kernel is
// nodal.  Only contact.hip includes this header.
#pragma once

#include "face_common.hpp"

namespace mimi_hip {
namespace {

constexpr int kAugmentedNodeScalars = 4;

__global__ __launch_bounds__(256) void contact_augmented_update_kernel(int n_marked, const double* __restrict__ area,
                                                                       const double* __restrict__ gap, double penalty, int apply,
                                                                       double* __restrict__ lambda, double* __restrict__ node_scal) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_marked) return;
  const double lam = lambda[i];
  const double v = lam + gap[i] / area[i] * penalty;   // (the text of contact_pressure_kernel<true>)
  const double p = v < 0.0 ? v : 0.0;
  const double d = p - lam;
  const double after = apply ? p : lam;
  node_scal[(int64_t)i * kAugmentedNodeScalars + 0] = area[i] * d * d;
  node_scal[(int64_t)i * kAugmentedNodeScalars + 1] = p < 0.0 ? 1.0 : 0.0;
  node_scal[(int64_t)i * kAugmentedNodeScalars + 2] = fabs(d);
  node_scal[(int64_t)i * kAugmentedNodeScalars + 3] = fabs(after);
  if (apply) lambda[i] = p;
}

__global__ __launch_bounds__(1024) void contact_augmented_measure_kernel(int n_marked, const double* __restrict__ node_scal,
                                                                         double penalty, double* __restrict__ out4) {
  __shared__ double part[1024];
  double res[kAugmentedNodeScalars];
  for (int k = 0; k < kAugmentedNodeScalars; ++k) {
    const bool is_max = k >= 2;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_marked; i += 1024) {
      const double x = node_scal[(int64_t)i * kAugmentedNodeScalars + k];
      s = is_max ? (x > s ? x : s) : s + x;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
      if ((int)threadIdx.x < w) {
        const double a = part[threadIdx.x], b = part[threadIdx.x + w];
        part[threadIdx.x] = is_max ? (b > a ? b : a) : a + b;
      }
      __syncthreads();
    }
    res[k] = part[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out4[0] = res[2] / penalty;
    out4[1] = sqrt(res[0]);
    out4[2] = res[1];
    out4[3] = res[3];
  }
}

__global__ __launch_bounds__(256) void contact_augmented_project_kernel(int n_marked, double* __restrict__ lambda) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_marked) return;
  const double lam = lambda[i];
  lambda[i] = lam < 0.0 ? lam : 0.0;
}

// The multipliers of one contact handle: nothing exists before the first switch-on
struct AugmentedState {
  bool on = false;
  DeviceBuffer<double> lambda;      // [n_marked]
  DeviceBuffer<double> node_scal;   // [n_marked][4] of the last update
  DeviceBuffer<double> out4;

  // off -> on: the multipliers start at zero; on -> on keeps them
  void set(FaceSet& h, bool want) {
    if (want && !on) {
      lambda.resize((size_t)h.n_fnodes);
      node_scal.resize((size_t)h.n_fnodes * kAugmentedNodeScalars);
      out4.resize(kAugmentedNodeScalars);
      MH_HIP(hipMemsetAsync(lambda.ptr, 0, (size_t)h.n_fnodes * sizeof(double), h.stream));
    }
    on = want;
  }

  void project(FaceSet& h) {
    launch(contact_augmented_project_kernel, dim3((unsigned)((h.n_fnodes + 255) / 256)), dim3(256), 0, h.stream, (int)h.n_fnodes,
           lambda.ptr);
  }

  // behind pass 1 at the configuration in question: area / gap are the handle's nodal sums
  void update(FaceSet& h, const double* area, const double* gap, double penalty, bool apply) {
    launch(contact_augmented_update_kernel, dim3((unsigned)((h.n_fnodes + 255) / 256)), dim3(256), 0, h.stream, (int)h.n_fnodes, area,
           gap, penalty, apply ? 1 : 0, lambda.ptr, node_scal.ptr);
    launch(contact_augmented_measure_kernel, dim3(1), dim3(1024), 0, h.stream, (int)h.n_fnodes, (const double*)node_scal.ptr, penalty,
           out4.ptr);
  }
};

}  // namespace
}  // namespace mimi_hip
