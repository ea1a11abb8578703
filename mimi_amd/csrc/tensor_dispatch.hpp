// Dispatch of a tensor-path assembly to its kernel family.
#pragma once

#include "kernels_tensor_residual.hpp"
#include "kernels_tensor_small.hpp"
#include "kernels_tensor_wgsym.hpp"
#include "tensor_p3.hpp"

namespace mimi_hip {

// can this handle's assembly run on the tensor kernels?  (3-D degree 2 and 3 have the two-phase kernels only: a patch
// whose CSR is not the structured pattern, or with repeated interior knots, takes the general kernels)
inline bool tensor_usable(const mimi_hip_domain_s* h) {
  if (h->path != 1) return false;
  if (tensor_small_shape(h->dim, h->degree, h->nq1[0])) return true;
  return h->degree[0] == 3 ? tensor_p3_ready(h) : two_phase_supported(h);
}

// returns the kernel family that ran (mimi_hip_domain_s::last_family)
inline int launch_tensor(mimi_hip_domain_s* h, const DomainCall& c) {
  TensorArgs a = tensor_args(h, c);
  if (h->degree[0] == 3) {
    launch_tensor_p3(h, c, a);
    return MIMI_HIP_FAMILY_TENSOR_P3_TWO_PHASE;
  }
  // the symmetric-half kernel for the hyperelastic law, the nine-block kernel behind the material pre-pass for the others
  if (!c.grad) launch_tensor_residual(h, a);
  else if (h->mat.m.kind == MIMI_HIP_MAT_NEOHOOKEAN) launch_tensor_wgsym(h, c, a);
  else launch_tensor_wgs(h, c, a);
  return MIMI_HIP_FAMILY_TENSOR_P2_TWO_PHASE;
}

inline void launch_tensor_post(mimi_hip_domain_s* h, const DomainCall& c) {
  if (h->degree[0] == 3) launch_tensor_p3_post(h, tensor_args(h, c));
  else launch_tensor_p2_post(h, tensor_args(h, c));
}

}  // namespace mimi_hip
