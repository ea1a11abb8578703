// The least-squares side of restarted GMRES as mfem::GMRESSolver::Mult runs it (linalg/solvers.cpp: ApplyPlaneRotation,
// GeneratePlaneRotation, Update): the Hessenberg matrix of a cycle, kept triangular by Givens rotations, and the rotated
// right-hand side, whose last entry is the residual estimate.  Pure host arithmetic, no HIP: krylov.hip feeds it the columns
// the device sends, tests/host_gmres_main.cpp the columns of a file (tests/test_gmres_host_cpu.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace mimi_hip {

struct GmresLeastSquares {
  int kdim;
  std::vector<double> H, sv, cs, sn, y;   // H: (kdim + 1) x kdim, column-major

  explicit GmresLeastSquares(int kdim_)
      : kdim(kdim_), H((size_t)(kdim_ + 1) * kdim_, 0.0), sv(kdim_ + 1, 0.0), cs(kdim_ + 1, 0.0), sn(kdim_ + 1, 0.0), y(kdim_) {}

  double& Hat(int i, int j) { return H[(size_t)i + (size_t)j * (kdim + 1)]; }

  // a cycle starts from v_0 = r / beta
  void start_cycle(double beta) {
    std::fill(sv.begin(), sv.end(), 0.0);
    sv[0] = beta;
  }

  // Column i of the cycle in the wire format of the device: col[0 .. i] = h_0 .. h_i, col[i + 1] = ||w||^2 after the last
  // projection.  Returns the residual estimate |s_{i+1}|.
  double push_column(int i, const double* col) {
    for (int k = 0; k <= i; ++k) Hat(k, i) = col[k];
    Hat(i + 1, i) = std::sqrt(col[i + 1]);
    // Givens rotations (GMRESSolver: ApplyPlaneRotation / GeneratePlaneRotation)
    for (int k = 0; k < i; ++k) {
      const double t = cs[k] * Hat(k, i) + sn[k] * Hat(k + 1, i);
      Hat(k + 1, i) = -sn[k] * Hat(k, i) + cs[k] * Hat(k + 1, i);
      Hat(k, i) = t;
    }
    const double dx = Hat(i, i), dy = Hat(i + 1, i);
    if (dy == 0.0) {
      cs[i] = 1.0;
      sn[i] = 0.0;
    } else if (std::fabs(dy) > std::fabs(dx)) {
      const double t = dx / dy;
      sn[i] = 1.0 / std::sqrt(1.0 + t * t);
      cs[i] = t * sn[i];
    } else {
      const double t = dy / dx;
      cs[i] = 1.0 / std::sqrt(1.0 + t * t);
      sn[i] = t * cs[i];
    }
    Hat(i, i) = cs[i] * dx + sn[i] * dy;
    Hat(i + 1, i) = 0.0;
    sv[i + 1] = -sn[i] * sv[i];
    sv[i] = cs[i] * sv[i];
    return std::fabs(sv[i + 1]);
  }

  // the coefficients y[0 .. k) of the first k basis vectors: back substitution (GMRESSolver: Update(x, k, H, s, v))
  const double* solve(int k) {
    for (int i = k - 1; i >= 0; --i) {
      double t = sv[i];
      for (int j = i + 1; j < k; ++j) t -= Hat(i, j) * y[j];
      y[i] = t / Hat(i, i);
    }
    return y.data();
  }
};

}  // namespace mimi_hip
