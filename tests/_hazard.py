"""A kernel with a real hazard, shared by test_isa_lint_cpu.py and test_build_cpu.py: an asm fp64 matrix instruction whose
result a vector instruction reads PAD + 1 wait states later (19 are needed on gfx950; one `s_nop` gives 16 at the most)."""

HAZARD = r"""
#include <hip/hip_runtime.h>
typedef double d4 __attribute__((ext_vector_type(4)));
extern "C" __global__ void hazard_kernel(const double* a, const double* b, double* out) {
  d4 c;
  const double x = a[threadIdx.x], y = b[threadIdx.x];
  asm volatile("s_nop 1\n\tv_mfma_f64_16x16x4_f64 %0, %1, %2, 0" : "=&v"(c) : "v"(x), "v"(y));
  asm volatile("s_nop %0" :: "n"(PAD));
  double s;
  asm volatile("v_add_f64 %0, %1, %2" : "=v"(s) : "v"(c[0]), "v"(c[1]));
  out[threadIdx.x] = s;
}
"""

PAD_STATEMENT = 'asm volatile("s_nop %0" :: "n"(PAD));'
SAFE_STATEMENT = 'asm volatile("s_nop 15\\n\\ts_nop 2");'
assert PAD_STATEMENT in HAZARD
