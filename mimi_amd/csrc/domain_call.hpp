// What one call of the domain integrator is, as the C entry describes it and every launcher below it reads it (nothing
// about a call is kept on the handle); the one map from a material kind to its kernel instantiation; the skeleton of a
// two-phase assembly.  Included by both translation units that launch domain kernels (domain.hip, tensor_p3.hip).
#pragma once

#include <type_traits>

#include "domain.hpp"

namespace mimi_hip {

struct DomainCall {
  const double* u = nullptr;
  double* r = nullptr;
  double* A = nullptr;
  // mimi_hip_domain_add_residual_and_grad_from, both arrays on the device: the array the row gathers read the old values
  // from (nullptr: A itself, the plain "+=").  A route without a row gather copies it into A first (launch_general).
  const double* A_base = nullptr;
  double grad_factor = 0.0;
  int grad = 0;   // 0 residual, 1 residual + tangent, 2 residual + the reference's finite-difference tangent
  // a two-phase assembly runs both phases; mimi_hip_domain_integrate phase 1 only; mimi_hip_domain_gather phase 2 only,
  // over the node window [gather_begin, gather_end)
  enum Phases { BOTH, INTEGRATE_ONLY, GATHER_ONLY } phases = BOTH;
  int gather_begin[3] = {0, 0, 0}, gather_end[3] = {0, 0, 0};

  bool integrates() const { return phases != GATHER_ONLY; }
  bool gathers() const { return phases != INTEGRATE_ONLY; }
  const double* A_old() const { return (A_base && A) ? A_base : A; }   // what a row gather adds grad_factor K to
};

inline bool material_has_state(int kind) { return kind != MIMI_HIP_MAT_NEOHOOKEAN && kind != MIMI_HIP_MAT_STVK; }
// closed-form tangents inside the kernels (every kernel family) vs the other materials (materials_other.hpp: general
// kernels, and the two-phase tensor kernels through the tangent record of the material pre-pass)
inline bool material_closed_form(int kind) { return kind == MIMI_HIP_MAT_NEOHOOKEAN || kind == MIMI_HIP_MAT_J2; }

// calls f(std::integral_constant<int, FAMILY>) for a material kind: family 0 for the two closed-form materials, the kind
// itself for the other four -- the kernels take it as a compile-time constant (one instantiation per material: no spilled
// registers).  A site whose kernel tells neo-Hookean from J2, or reads the other materials through a record, derives
// that from the family and the kind.
template<class F>
void by_material_family(int kind, F&& f) {
  switch (kind) {
  case MIMI_HIP_MAT_NEOHOOKEAN:
  case MIMI_HIP_MAT_J2: f(std::integral_constant<int, 0>{}); break;
  case MIMI_HIP_MAT_STVK: f(std::integral_constant<int, MIMI_HIP_MAT_STVK>{}); break;
  case MIMI_HIP_MAT_J2LINEAR: f(std::integral_constant<int, MIMI_HIP_MAT_J2LINEAR>{}); break;
  case MIMI_HIP_MAT_J2SIMO: f(std::integral_constant<int, MIMI_HIP_MAT_J2SIMO>{}); break;
  default: f(std::integral_constant<int, MIMI_HIP_MAT_J2LOG>{}); break;
  }
}

// A two-phase assembly: [material pre-pass,] integration kernel(s), row gather, with the phase events around them
// (mimi_hip_domain_phase_ms*: [0] start, [3] end of the pre-pass when the family has one, [1] end of phase 1, [2] end).
// has_prepass describes the kernel family, not this call: a gather-only call records the same events.
template<class Pre, class Integrate, class Gather>
void run_two_phase(mimi_hip_domain_s* h, const DomainCall& c, bool has_prepass, Pre&& prepass, Integrate&& integrate,
                   Gather&& gather) {
  auto mark = [&](int k) {
    if (h->phase_timing) MH_HIP(hipEventRecord(h->phase_ev[k], h->stream));
  };
  h->phase_has_prepass = has_prepass;
  mark(0);
  if (has_prepass) {
    if (c.integrates()) prepass();
    mark(3);
  }
  if (c.integrates()) integrate();
  mark(1);
  if (c.gathers()) gather();
  mark(2);
}

}  // namespace mimi_hip
