// TEST HARNESS ONLY: the rigid spline body of the contact integrator (mimi_amd/csrc/spline_body.hpp) compiled for the
// HOST, so that its evaluation and its closest-point search can be checked point by point without a GPU
// (tests/test_spline_body_cpu.py).  The body is set up by sb_fill_host, the function upload_spline_body of
// csrc/contact.hip calls: the real set-up, not a copy.  Nothing in mimi_amd builds or loads this.
#include "../include/mimi_hip.h"
#include "../mimi_amd/csrc/spline_body.hpp"

using namespace mimi_hip;

namespace {
void fill(SplineBodyHost& h, const mimi_hip_spline_body* sp, int dim) {
  int res = sp->kdtree_resolution > 1 ? sp->kdtree_resolution : 100;
  const int degree[2] = {sp->degree[0], sp->degree[1]}, n_knots[2] = {sp->n_knots[0], sp->n_knots[1]};
  sb_fill_host(h, sp->para_dim, dim, degree, n_knots, sp->knots, sp->control_points, sp->weights, res, sp->max_iterations);
}
}  // namespace

// the closed directions sb_fill_host found
extern "C" void host_sb_closed(const mimi_hip_spline_body* body, int dim, int* closed) {
  SplineBodyHost h;
  fill(h, body, dim);
  closed[0] = h.dev.closed[0];
  closed[1] = h.dev.closed[1];
}

// n points: xi [n][para_dim] -> S [n][dim], S1 [n][para_dim][dim], S2 [n][para_dim][para_dim][dim]
extern "C" void host_sb_evaluate(const mimi_hip_spline_body* body, int dim, int n, const double* xi, double* S, double* S1,
                                 double* S2) {
  SplineBodyHost h;
  fill(h, body, dim);
  const int pd = h.dev.para_dim;
  for (int k = 0; k < n; ++k)
    sb_evaluate(h.dev, xi + (size_t)k * pd, S + (size_t)k * dim, S1 + (size_t)k * pd * dim, S2 + (size_t)k * pd * pd * dim);
}

// n queries: xq [n][dim] -> xi [n][para_dim], S [n][dim], S1 [n][para_dim][dim], true gap and distance of sb_nearest
extern "C" void host_sb_closest(const mimi_hip_spline_body* body, int dim, int n, const double* xq, double* xi, double* S,
                                double* S1, double* true_g, double* distance) {
  SplineBodyHost h;
  fill(h, body, dim);
  const int pd = h.dev.para_dim;
  for (int k = 0; k < n; ++k) {
    sb_closest_point(h.dev, xq + (size_t)k * dim, xi + (size_t)k * pd, S + (size_t)k * dim, S1 + (size_t)k * pd * dim);
    sb_nearest(h.dev, xq + (size_t)k * dim, true_g[k], distance[k]);
  }
}
