// TEST HARNESS ONLY: field_at_point of mimi_amd/csrc/kernels_fields.hpp -- what a lane of the field kernels computes at its
// quadrature point -- compiled for the HOST, so that every field of every material can be checked against the yardstick
// point by point without a GPU (tests/test_fields_cpu.py).  Nothing in mimi_amd builds or loads this.
#define MH_DEV __host__ __device__ inline
#include "../mimi_amd/csrc/common.hpp"
#include "../mimi_amd/csrc/kernels_fields.hpp"

namespace mimi_hip {
void set_last_error(const std::string&) {}
}
using namespace mimi_hip;

// the instantiation the dispatch picks for the material (by_field_family, domain_dispatch.hpp)
template<int DIM>
static int field_of_kind(const MaterialDev& md, double dt, const StateView& sv, int field, const double* F, double* f) {
  switch (md.m.kind) {
  case MIMI_HIP_MAT_NEOHOOKEAN: return field_at_point<DIM, FIELD_NEOHOOKEAN>(md, dt, sv, 0, field, F, f);
  case MIMI_HIP_MAT_J2: return field_at_point<DIM, 0>(md, dt, sv, 0, field, F, f);
  case MIMI_HIP_MAT_STVK: return field_at_point<DIM, MIMI_HIP_MAT_STVK>(md, dt, sv, 0, field, F, f);
  case MIMI_HIP_MAT_J2LINEAR: return field_at_point<DIM, MIMI_HIP_MAT_J2LINEAR>(md, dt, sv, 0, field, F, f);
  case MIMI_HIP_MAT_J2SIMO: return field_at_point<DIM, MIMI_HIP_MAT_J2SIMO>(md, dt, sv, 0, field, F, f);
  default: return field_at_point<DIM, MIMI_HIP_MAT_J2LOG>(md, dt, sv, 0, field, F, f);
  }
}

// state arrays address ONE point (SoA with n_pts = 1 = plain column-major matrices); f: dim * dim doubles
extern "C" int host_field(const mimi_hip_material* m, int dim, double dt, int field, const double* F, double* m1, double* m2,
                          double eqps, double T, double* f) {
  const MaterialDev md = make_material_dev(*m);
  const StateView sv{&eqps, &T, m1, 1, m2};
  return dim == 2 ? field_of_kind<2>(md, dt, sv, field, F, f) : field_of_kind<3>(md, dt, sv, field, F, f);
}
