/* TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.
 *
 * Plain-C restatement of the reference's CPU element-integration / assembly path
 * ("restated reference path").  Same algorithm and loop structure as the
 * reference; every function cites the reference lines it follows
 * (paths relative to /root/reference/src/mimi/).  The reference itself cannot be
 * compiled here: every translation unit includes <mfem.hpp> and
 * third_party/mfem is an empty, un-pinned submodule, so the small dense MFEM
 * kernels it calls (MultAtB, MultABt, AddMult_a_ABt, CalcInverse, Det) are
 * restated inline from their published definitions.
 *
 * Parity pinning: tests/test_oracle_golden.py drives this file through an
 * in-repo gen-alpha/Newton harness and reproduces the reference's golden
 * fixtures tests/data/ref/{neohook,j2}_h1_p2/x_{0..9}.txt.
 *
 * Layout conventions (identical to the reference):
 *   u, r        : fp64[n_vdofs], byVDIM  (u[node*dim + c])
 *   v_dofs[e]   : [dofs*dim+0 ..., dofs*dim+1 ..., ...]      (precomputed.cpp:84)
 *   element x   : (n_dof x dim) column-major                  (integrator_utils.cpp:27)
 *   dN_dX[e][q] : (n_dof x dim) column-major                  (precomputed.cpp:316-321)
 *   K_e         : (n_tdof x n_tdof) column-major              (nonlinear_solid.cpp:55-74)
 *   A_ids[e]    : A_ids[c*n_tdof + r] -> CSR value position   (precomputed.cpp:185-199)
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define MAXD 3
#define MAX_TDOF 192 /* 3-D p=3 */

enum { MAT_NEOHOOKEAN = 0, MAT_J2 = 1, MAT_STVK = 2, MAT_J2LINEAR = 3, MAT_J2SIMO = 4, MAT_J2LOG = 5 };
enum { HARD_POWERLAW = 0, HARD_VOCE = 1, HARD_JC = 2, HARD_JC_RATE = 3, HARD_JC_TEMP_RATE = 4,
       HARD_JC_CONST_TEMP = 5 };
enum { TANGENT_FD = 0, TANGENT_EXACT = 1, TANGENT_NONE = 2 };   /* NONE: no elements, only the zeroing + reduction passes (timing probe) */

typedef struct {
  int kind;
  /* MaterialBase (materials.hpp:31-38) */
  double density, lambda, mu, K, G;
  /* J2 (materials.hpp:268-273) */
  double heat_fraction, specific_heat, initial_temperature, melting_temperature;
  /* hardening (material_hardening.hpp) */
  int hard_kind;
  double sigma_y, n, eps0;                 /* PowerLaw */
  double sigma_sat, strain_constant;       /* Voce */
  double A, B, C, eps0_dot;                /* JohnsonCook (+rate) */
  double reference_temperature, m;         /* + temperature */
  double const_temperature_contribution;   /* JohnsonCookConstantTemperature */
  /* J2Linear (materials.hpp:149-151) */
  double lin_isotropic_hardening, lin_kinematic_hardening, lin_sigma_y;
} oracle_material;

typedef struct {
  int dim, n_el, n_dof, n_q, n_vdofs;
  const int* v_dofs;      /* [n_el][n_tdof] */
  const int* a_ids;       /* [n_el][n_tdof^2] or NULL */
  const double* dN_dX;    /* [n_el][n_q][dim][n_dof] */
  const double* weight;   /* [n_el][n_q]  integration_weight */
  const double* det;      /* [n_el][n_q]  det_dX_dxi */
  oracle_material mat;
  /* J2 state (materials.hpp:278-286), one record per (element, quad point) */
  double* plastic_strain; /* [n_el][n_q][dim*dim] column-major */
  double* eqps;           /* [n_el][n_q] accumulated plastic strain */
  double* temperature;    /* [n_el][n_q] */
  double dt;              /* material_->dt_ (nonlinear_solid.cpp:154,167) */
  /* the other materials' first state matrix lives in plastic_strain (J2Linear: plastic strain; J2Simo: be_old;
   * J2Log: Fp_inv), their second one here (J2Linear: beta, J2Simo: F_old)  (materials.hpp:153-161,428-437,576-584) */
  double* state2;         /* [n_el][n_q][dim*dim] or NULL */
} oracle_domain;

/* ---- utils/n_thread_exe.hpp:12-26 ---------------------------------------- */
static void chunk_rule(long total, long nthread, long ithread, long* from, long* to) {
  const long chunk = (total + nthread - 1) / nthread;
  if (ithread < nthread - 1) {
    *from = ithread * chunk;
    *to = (ithread + 1) * chunk;
  } else {
    *from = (nthread - 1) * chunk;
    *to = total;
  }
  if (*from > total) *from = total;
  if (*to > total) *to = total;
}

/* ---- small dense helpers (column-major dim x dim) ------------------------- */
static double det_d(const double* F, int dim) {
  if (dim == 2) return F[0] * F[3] - F[1] * F[2];
  return F[0] * (F[4] * F[8] - F[5] * F[7]) - F[3] * (F[1] * F[8] - F[2] * F[7])
         + F[6] * (F[1] * F[5] - F[2] * F[4]);
}

static void inv_d(const double* F, int dim, double* Fi) {
  const double d = det_d(F, dim);
  const double t = 1.0 / d;
  if (dim == 2) {
    Fi[0] = F[3] * t;
    Fi[1] = -F[1] * t;
    Fi[2] = -F[2] * t;
    Fi[3] = F[0] * t;
    return;
  }
  Fi[0] = (F[4] * F[8] - F[5] * F[7]) * t;
  Fi[1] = (F[2] * F[7] - F[1] * F[8]) * t;
  Fi[2] = (F[1] * F[5] - F[2] * F[4]) * t;
  Fi[3] = (F[5] * F[6] - F[3] * F[8]) * t;
  Fi[4] = (F[0] * F[8] - F[2] * F[6]) * t;
  Fi[5] = (F[2] * F[3] - F[0] * F[5]) * t;
  Fi[6] = (F[3] * F[7] - F[4] * F[6]) * t;
  Fi[7] = (F[1] * F[6] - F[0] * F[7]) * t;
  Fi[8] = (F[0] * F[4] - F[1] * F[3]) * t;
}

#define M(A, i, j) (A)[(i) + (j) * dim]

/* ---- hardening: ADScalar<double,1> restated as (value, derivative) -------- */
typedef struct { double v, d; } dual;

/* material_hardening.hpp:75-77,261-279,326-333 */
static double thermo_contribution(const oracle_material* m, double T) {
  if (m->hard_kind == HARD_JC_TEMP_RATE) {
    double c = 1.0;
    if (T < m->reference_temperature) {
    } else if (T > m->melting_temperature) {
      c = 0.0;
    } else {
      c -= pow((T - m->reference_temperature) / (m->melting_temperature - m->reference_temperature), m->m);
    }
    return c;
  }
  if (m->hard_kind == HARD_JC_CONST_TEMP) return m->const_temperature_contribution;
  return 1.0;
}

/* material_hardening.hpp:62-64,162-173 */
static double rate_contribution(const oracle_material* m, double rate) {
  if (m->hard_kind >= HARD_JC_RATE) {
    double v = 1.0;
    if (rate > m->eps0_dot) v += m->C * log(rate / m->eps0_dot);
    return v;
  }
  return 1.0;
}

/* d/d(rate) of the above (only for the exact tangent; the reference's return-map
 * Newton does not differentiate it: material_hardening.hpp:69-71) */
static double rate_contribution_derivative(const oracle_material* m, double rate) {
  if (m->hard_kind >= HARD_JC_RATE && rate > m->eps0_dot) return m->C / rate;
  return 0.0;
}

/* utils/ad.inl:263-279  pow(ADScalar, double) */
static dual dual_pow(dual b, double power) {
  const double tmp = pow(b.v, power - 1.0);
  dual r;
  r.v = b.v * tmp;
  r.d = b.d * (power * tmp);
  return r;
}

/* material_hardening.hpp:88-95 (PowerLaw), 108-116 (Voce), 131-140 (JohnsonCook) */
static dual hardening_evaluate(const oracle_material* m, dual eqps) {
  dual r;
  switch (m->hard_kind) {
  case HARD_POWERLAW: {
    dual b = {1.0 + eqps.v / m->eps0, eqps.d / m->eps0};
    dual p = dual_pow(b, 1.0 / m->n);
    r.v = m->sigma_y * p.v;
    r.d = m->sigma_y * p.d;
    return r;
  }
  case HARD_VOCE: {
    const double e = exp(-eqps.v / m->strain_constant);
    r.v = m->sigma_sat - (m->sigma_sat - m->sigma_y) * e;
    r.d = (m->sigma_sat - m->sigma_y) * e * (eqps.d / m->strain_constant);
    return r;
  }
  default: {
    if (fabs(eqps.v) < 1.e-13) {
      r.v = m->A;
      r.d = 0.0;
      return r;
    }
    dual p = dual_pow(eqps, m->n);
    r.v = m->A + m->B * p.v;
    r.d = m->B * p.d;
    return r;
  }
  }
}

static double sigma_y_of(const oracle_material* m) {
  return (m->hard_kind == HARD_POWERLAW || m->hard_kind == HARD_VOCE) ? m->sigma_y : m->A;
}

/* materials.hpp:343-349  the return-mapping residual lambda */
typedef struct {
  const oracle_material* m;
  double eqps_old, q, thermo, dt;
  double slope;   /* 3G (J2, J2Log: materials.hpp:345,622) or G tr(be) (J2Simo: materials.hpp:495) */
} rm_ctx;

static dual rm_residual(const rm_ctx* c, dual delta) {
  dual e = {c->eqps_old + delta.v, delta.d};
  dual H = hardening_evaluate(c->m, e);
  const double fac = rate_contribution(c->m, delta.v / c->dt) * c->thermo;
  dual r;
  r.v = c->q - c->slope * delta.v - H.v * fac;
  r.d = -c->slope * delta.d - H.d * fac;
  return r;
}

/* solvers/newton.hpp:53-169  ScalarSolve; returns x, *status != 0 on the
 * reference's throw paths (not bracketed / not converged). */
static double scalar_solve(const rm_ctx* c, double x0, double lower, double upper, double xtol,
                           double rtol, unsigned max_iter, int* status) {
  double x, df_dx;
  dual a = {lower, 0.0}, b = {upper, 0.0};
  double fl = rm_residual(c, a).v;
  double fh = rm_residual(c, b).v;
  unsigned iterations = 0;
  int converged = 0;
  *status = 0;
  if (fabs(fl) < xtol) return lower;
  if (fabs(fh) < xtol) return upper;
  if (fl * fh > 0.) {
    *status = 1;
    return lower;
  }
  double xl = lower, xh = upper;
  if (fl > 0) {
    xl = upper;
    xh = lower;
  }
  if (x0 < lower || x0 > upper) x0 = 0.5 * (lower + upper);
  x = x0;
  double delta_x_old = fabs(upper - lower);
  double delta_x = delta_x_old;
  dual xx = {x, 1.0};
  dual R = rm_residual(c, xx);
  double fval = R.v;
  df_dx = R.d;
  while (!converged) {
    if (iterations == max_iter) {
      *status = 2;
      break;
    }
    if ((x - xh) * df_dx - fval > 0 || (x - xl) * df_dx - fval < 0
        || fabs(2. * fval) > fabs(delta_x_old * df_dx)) {
      delta_x_old = delta_x;
      delta_x = 0.5 * (xh - xl);
      x = xl + delta_x;
    } else {
      delta_x_old = delta_x;
      delta_x = fval / df_dx;
      x -= delta_x;
    }
    xx.v = x;
    R = rm_residual(c, xx);
    fval = R.v;
    df_dx = R.d;
    converged = converged || (fabs(delta_x) < xtol) || (fabs(fval) < rtol);
    if (fval < 0) xl = x; else xh = x;
    ++iterations;
  }
  return x;
}

/* ---- materials ------------------------------------------------------------ */
typedef struct {
  /* per-point scratch = NonlinearSolidWorkData (integrator_utils.hpp:14-115) */
  double F[9], Finv[9], detF, P[9];
  /* J2 by-products needed by the exact tangent */
  double s_trial[9], q, delta, hprime, sigma[9];
  int plastic;
} point_work;

/* materials.cpp:96-118 (EvaluateCauchy) + materials.cpp:60-71 (base EvaluatePK1) */
static void neo_hookean_pk1(const oracle_material* m, int dim, point_work* w) {
  double B[9], sigma[9];
  const double detF = w->detF;
  const double mu_over = m->mu / detF;
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double s = 0;
      for (int k = 0; k < dim; ++k) s += M(w->F, i, k) * M(w->F, j, k);
      M(B, i, j) = s;
    }
  const double diag = -mu_over + m->lambda * (detF - 1.);
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) M(sigma, i, j) = mu_over * M(B, i, j) + (i == j ? diag : 0.0);
  /* P = det(F) * sigma * F^-T */
  for (int i = 0; i < dim; ++i)
    for (int J = 0; J < dim; ++J) {
      double s = 0;
      for (int k = 0; k < dim; ++k) s += M(sigma, i, k) * M(w->Finv, J, k);
      M(w->P, i, J) = s * detF;
    }
  memcpy(w->sigma, sigma, sizeof(sigma));
}

/* materials.hpp:311-391  J2::PlasticStress<accumulate>, then base EvaluatePK1.
 * state pointers address ONE quadrature point.  Returns non-zero on the
 * reference's ScalarSolve throw paths. */
static int j2_plastic_stress(const oracle_material* m, int dim, double dt, int accumulate,
                             double* plastic_strain, double* eqps, double* temperature,
                             point_work* w) {
  double eps[9], s[9], Np[9];
  const int dd = dim * dim;
  /* material_utils.hpp:60-84 ElasticStrain: sym(F) - I - eps_p */
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) M(eps, i, j) = 0.5 * (M(w->F, i, j) + M(w->F, j, i));
  for (int i = 0; i < dim; ++i) M(eps, i, i) -= 1.;
  for (int i = 0; i < dd; ++i) eps[i] -= plastic_strain[i];
  double tr = 0;
  for (int i = 0; i < dim; ++i) tr += M(eps, i, i);
  const double p = m->K * tr;
  /* material_utils.hpp:22-56 Dev(eps, dim, 2G, s): trace divided by dim */
  const double tr_over_dim = tr / (double)dim;
  for (int i = 0; i < dd; ++i) s[i] = eps[i] * (2.0 * m->G);
  for (int i = 0; i < dim; ++i) M(s, i, i) = (M(eps, i, i) - tr_over_dim) * (2.0 * m->G);
  double nrm = 0;
  for (int i = 0; i < dd; ++i) nrm += s[i] * s[i];
  nrm = sqrt(nrm);
  const double q = sqrt(3.0 / 2.0) * nrm;
  memcpy(w->s_trial, s, sizeof(s));
  w->q = q;
  w->plastic = 0;
  w->delta = 0;
  w->hprime = 0;

  rm_ctx c;
  c.m = m;
  c.eqps_old = *eqps;
  c.q = q;
  c.thermo = thermo_contribution(m, *temperature);
  c.dt = dt;
  c.slope = 3.0 * m->G;
  const double tolerance = sigma_y_of(m) * 1.e-10;
  dual zero = {0.0, 0.0};
  int status = 0;
  if (rm_residual(&c, zero).v > tolerance) {
    dual e0 = {c.eqps_old, 0.0};
    const double upper = (q - hardening_evaluate(m, e0).v * c.thermo) / (3.0 * m->G);
    const double delta = scalar_solve(&c, 0.0, 0.0, upper, 1.e-10, tolerance, 100, &status);
    for (int i = 0; i < dd; ++i) Np[i] = (1.5 / q) * s[i];
    w->plastic = 1;
    w->delta = delta;
    {
      /* total derivative of H(eqps+D)*rate(D/dt)*thermo wrt D, for the exact tangent */
      dual e1 = {c.eqps_old + delta, 1.0};
      dual H = hardening_evaluate(m, e1);
      const double rc = rate_contribution(m, delta / dt);
      w->hprime = H.d * rc * c.thermo + H.v * rate_contribution_derivative(m, delta / dt) / dt * c.thermo;
    }
    if (!accumulate) {
      for (int i = 0; i < dd; ++i) s[i] += -2.0 * m->G * delta * Np[i];
    } else {
      *eqps += delta;
      for (int i = 0; i < dd; ++i) plastic_strain[i] += delta * Np[i];
      if (m->hard_kind == HARD_JC_TEMP_RATE) {
        *temperature += m->heat_fraction * q * delta / (m->density * m->specific_heat);
      }
    }
  }
  if (!accumulate) {
    double sigma[9];
    for (int i = 0; i < dd; ++i) sigma[i] = s[i];
    for (int i = 0; i < dim; ++i) M(sigma, i, i) += p;
    memcpy(w->sigma, sigma, sizeof(sigma));
    /* materials.cpp:60-71: P = det(F) * sigma * F^-T */
    for (int i = 0; i < dim; ++i)
      for (int J = 0; J < dim; ++J) {
        double t = 0;
        for (int k = 0; k < dim; ++k) t += M(sigma, i, k) * M(w->Finv, J, k);
        M(w->P, i, J) = t * w->detF;
      }
  }
  return status;
}


/* ---- the other materials ------------------------------------------------------ */
/* symmetric eigen-decomposition (the reference calls mfem::DenseMatrix::CalcEigenvalues = LAPACK dsyev,
 * material_utils.hpp:104; materials.hpp:665): cyclic Jacobi, Q columns = eigenvectors */
static void sym_eig(const double* A, int dim, double* lam, double* Q) {
  double a[9];
  for (int i = 0; i < dim * dim; ++i) a[i] = A[i];
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) M(Q, i, j) = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int i = 0; i < dim; ++i)
      for (int j = 0; j < dim; ++j) {
        if (i != j) off += M(a, i, j) * M(a, i, j);
        else diag += M(a, i, i) * M(a, i, i);
      }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < dim - 1; ++p)
      for (int q = p + 1; q < dim; ++q) {
        const double apq = M(a, p, q);
        if (apq == 0.0) continue;
        const double theta = (M(a, q, q) - M(a, p, p)) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < dim; ++k) {   /* a <- a G */
          const double akp = M(a, k, p), akq = M(a, k, q);
          M(a, k, p) = c * akp - sn * akq;
          M(a, k, q) = sn * akp + c * akq;
        }
        for (int k = 0; k < dim; ++k) {   /* a <- G^T a */
          const double apk = M(a, p, k), aqk = M(a, q, k);
          M(a, p, k) = c * apk - sn * aqk;
          M(a, q, k) = sn * apk + c * aqk;
        }
        for (int k = 0; k < dim; ++k) {
          const double qkp = M(Q, k, p), qkq = M(Q, k, q);
          M(Q, k, p) = c * qkp - sn * qkq;
          M(Q, k, q) = sn * qkp + c * qkq;
        }
      }
  }
  for (int i = 0; i < dim; ++i) lam[i] = M(a, i, i);
}

/* out = Q diag(f(lam)) Q^T (mfem::MultADAt), f = log (is_exp 0) or exp (1) */
static void sym_fun(const double* A, int dim, int is_exp, double* out) {
  double lam[3], Q[9];
  sym_eig(A, dim, lam, Q);
  for (int i = 0; i < dim; ++i) lam[i] = is_exp ? exp(lam[i]) : log(lam[i]);
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double t = 0;
      for (int k = 0; k < dim; ++k) t += M(Q, i, k) * lam[k] * M(Q, j, k);
      M(out, i, j) = t;
    }
}

static void mat_mul(const double* A, const double* B, int dim, double* C_) { /* C = A B */
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double t = 0;
      for (int k = 0; k < dim; ++k) t += M(A, i, k) * M(B, k, j);
      M(C_, i, j) = t;
    }
}

static void mat_mul_abt(const double* A, const double* B, int dim, double* C_) { /* C = A B^T */
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double t = 0;
      for (int k = 0; k < dim; ++k) t += M(A, i, k) * M(B, j, k);
      M(C_, i, j) = t;
    }
}

/* material_utils.hpp:22-56 Dev(A, dim, factor): the trace is divided by dim */
static void dev_d(const double* A, int dim, double factor, double* out) {
  double tr = 0;
  for (int i = 0; i < dim; ++i) tr += M(A, i, i);
  const double tr_over_dim = tr / (double)dim;
  for (int i = 0; i < dim * dim; ++i) out[i] = A[i] * factor;
  for (int i = 0; i < dim; ++i) M(out, i, i) = (M(A, i, i) - tr_over_dim) * factor;
}

static double norm_d(const double* A, int dim) {
  double a = 0;
  for (int i = 0; i < dim * dim; ++i) a += A[i] * A[i];
  return sqrt(a);
}

/* polish != 0 (only for the oracle's difference-quotient tangent, never for the restated path): plain Newton steps on
 * top of ScalarSolve's answer, so that the stress is a smooth function of F to rounding */
static double polish_root(const rm_ctx* c, double x, double lower, double upper) {
  for (int it = 0; it < 6; ++it) {
    dual xx = {x, 1.0};
    dual R = rm_residual(c, xx);
    if (R.d == 0.0) break;
    const double xn = x - R.v / R.d;
    if (!(xn > lower && xn < upper) || xn == x) break;
    dual xt = {xn, 0.0};
    if (!(fabs(rm_residual(c, xt).v) < fabs(R.v))) break;   /* only steps that improve (first yield: H' unbounded) */
    x = xn;
  }
  return x;
}

/* -d residual / d delta at delta, including the rate term the reference's own Newton leaves out
 * (material_hardening.hpp:69-71) -- for the oracle tangent */
static double return_map_slope(const rm_ctx* c, double delta) {
  dual e1 = {c->eqps_old + delta, 1.0};
  dual H = hardening_evaluate(c->m, e1);
  const double rc = rate_contribution(c->m, delta / c->dt);
  return c->slope + H.d * rc * c->thermo + H.v * rate_contribution_derivative(c->m, delta / c->dt) / c->dt * c->thermo;
}

/* materials.cpp:72-94 StVenantKirchhoff::EvaluatePK1: S = lambda tr(E) I + 2 mu E, P = F S */
static void stvk_pk1(const oracle_material* m, int dim, point_work* w) {
  double C_[9], E[9], S[9];
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double t = 0;
      for (int k = 0; k < dim; ++k) t += M(w->F, k, i) * M(w->F, k, j);
      M(C_, i, j) = t;
    }
  double tr = 0;
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) M(E, i, j) = 0.5 * M(C_, i, j) - (i == j ? 0.5 : 0.0);
  for (int i = 0; i < dim; ++i) tr += M(E, i, i);
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) M(S, i, j) = 2 * m->mu * M(E, i, j) + (i == j ? m->lambda * tr : 0.0);
  mat_mul(w->F, S, dim, w->P);
}

static void pk1_from_sigma(int dim, const double* sigma, point_work* w) {
  /* materials.cpp:60-71: P = det(F) * sigma * F^-T */
  for (int i = 0; i < dim; ++i)
    for (int J = 0; J < dim; ++J) {
      double t = 0;
      for (int k = 0; k < dim; ++k) t += M(sigma, i, k) * M(w->Finv, J, k);
      M(w->P, i, J) = t * w->detF;
    }
}

/* materials.hpp:185-236  J2Linear::PlasticStress<accumulate>, then base EvaluatePK1 */
static int j2linear_stress(const oracle_material* m, int dim, int accumulate, double* plastic_strain, double* beta,
                           double* eqps, point_work* w) {
  double eps[9], s[9], eta[9];
  const int dd = dim * dim;
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) M(eps, i, j) = 0.5 * (M(w->F, i, j) + M(w->F, j, i));
  for (int i = 0; i < dim; ++i) M(eps, i, i) -= 1.;
  for (int i = 0; i < dd; ++i) eps[i] -= plastic_strain[i];
  double tr = 0;
  for (int i = 0; i < dim; ++i) tr += M(eps, i, i);
  const double p = m->K * tr;
  dev_d(eps, dim, 2.0 * m->G, s);
  for (int i = 0; i < dd; ++i) eta[i] = s[i] - beta[i];
  const double eta_norm = norm_d(eta, dim);
  const double q = sqrt(3.0 / 2.0) * eta_norm;
  const double phi = q - (m->lin_sigma_y + m->lin_isotropic_hardening * *eqps);
  /* by-products for the closed-form tangent (exact_tangent, J2 branch, with the relative stress eta in the place of the
   * trial deviator and the constant hardening slope) */
  memcpy(w->s_trial, eta, sizeof(eta));
  w->q = q;
  w->plastic = 0;
  w->delta = 0;
  w->hprime = m->lin_kinematic_hardening + m->lin_isotropic_hardening;
  if (phi > 0.) {
    const double inc = phi / (3. * m->G + m->lin_kinematic_hardening + m->lin_isotropic_hardening);
    w->plastic = 1;
    w->delta = inc;
    for (int i = 0; i < dd; ++i) eta[i] *= 1. / eta_norm;
    if (!accumulate) {
      for (int i = 0; i < dd; ++i) s[i] += -sqrt(6.0) * m->G * inc * eta[i];
    } else {
      *eqps += inc;
      for (int i = 0; i < dd; ++i) plastic_strain[i] += sqrt(3.0 / 2.0) * inc * eta[i];
      for (int i = 0; i < dd; ++i) beta[i] += sqrt(2.0 / 3.0) * m->lin_kinematic_hardening * inc * eta[i];
    }
  }
  if (!accumulate) {
    double sigma[9];
    for (int i = 0; i < dd; ++i) sigma[i] = s[i];
    for (int i = 0; i < dim; ++i) M(sigma, i, i) += p;
    memcpy(w->sigma, sigma, sizeof(sigma));
    pk1_from_sigma(dim, sigma, w);
  }
  return 0;
}

/* materials.hpp:452-545  J2Simo::PlasticStress<accumulate> (EvaluatePK1 is overridden: P straight from here) */
/* delta_fixed / r_out (oracle tangent only): take the plastic branch with the given increment instead of solving, and
 * report the return-map residual at it */
static int j2simo_stress(const oracle_material* m, int dim, double dt, int accumulate, int polish, double* be_old,
                         double* F_old, double* eqps, double* temperature, point_work* w, const double* delta_fixed,
                         double* r_out) {
  double f_inv[9] = {0}, f_bar[9] = {0}, be[9], fbbo[9], s[9], Np[9];
  const int dd = dim * dim;
  int status = 0;
  mat_mul(F_old, w->Finv, dim, f_inv);
  inv_d(f_inv, dim, f_bar);
  {
    /* materials.hpp:466-469: f_bar *= cbrt(det f_bar) -- multiplied, as written there */
    const double c = cbrt(det_d(f_bar, dim));
    for (int i = 0; i < dd; ++i) f_bar[i] *= c;
  }
  mat_mul(f_bar, be_old, dim, fbbo);
  mat_mul_abt(fbbo, f_bar, dim, be);
  dev_d(be, dim, m->G, s);
  const double s_norm = norm_d(s, dim);
  if (fabs(s_norm) < 2.220446049250313e-16) {
    for (int i = 0; i < dd; ++i) Np[i] = 0.0;
    for (int i = 0; i < dim; ++i) M(Np, i, i) = sqrt(1. / 2.);
  } else {
    for (int i = 0; i < dd; ++i) Np[i] = sqrt(3. / 2.) / s_norm * s[i];
  }
  double s_effective = 0;
  for (int i = 0; i < dd; ++i) s_effective += Np[i] * s[i];
  double be_trace = 0;
  for (int i = 0; i < dim; ++i) be_trace += M(be, i, i);

  rm_ctx c;
  c.m = m;
  c.eqps_old = *eqps;
  c.q = s_effective;
  w->q = s_effective;
  c.thermo = thermo_contribution(m, *temperature);
  c.dt = dt;
  c.slope = m->G * be_trace;
  const double tolerance = sigma_y_of(m) * 1.e-10;
  dual zero = {0.0, 0.0};
  w->plastic = 0;
  if (delta_fixed || rm_residual(&c, zero).v > tolerance) {
    dual e0 = {c.eqps_old, 0.0};
    const double upper = (s_effective - hardening_evaluate(m, e0).v * c.thermo) / (m->G * be_trace);
    double delta;
    if (delta_fixed) {
      dual df = {*delta_fixed, 0.0};
      delta = *delta_fixed;
      *r_out = rm_residual(&c, df).v;
    } else {
      delta = scalar_solve(&c, 0.0, 0.0, upper, 1.e-10, tolerance, 100, &status);
      if (polish) delta = polish_root(&c, delta, 0.0, upper);
    }
    w->plastic = 1;
    w->delta = delta;
    w->hprime = return_map_slope(&c, delta);
    for (int i = 0; i < dd; ++i) be[i] += -2. / 3. * delta * be_trace * Np[i];
    dev_d(be, dim, m->G, s);
    if (accumulate) {
      *eqps += delta;
      if (m->hard_kind == HARD_JC_TEMP_RATE)
        *temperature += m->heat_fraction * s_effective * delta / (m->density * m->specific_heat);
    }
  }
  if (!accumulate) {
    double tau[9];
    for (int i = 0; i < dd; ++i) tau[i] = s[i];
    for (int i = 0; i < dim; ++i) M(tau, i, i) += m->K * (w->detF * w->detF - 1.) * .5;
    mat_mul_abt(tau, w->Finv, dim, w->P);
  } else {
    memcpy(F_old, w->F, sizeof(double) * dd);
    memcpy(be_old, be, sizeof(double) * dd);
  }
  return status;
}

/* materials.hpp:592-713  J2Log::PlasticStress<accumulate> under the base EvaluatePK1 (materials.cpp:60-71), which
 * takes alternative_stress_ = s + (p / det F) I as the Cauchy stress and overwrites what PlasticStress left in
 * tmp.stress_:  P = det F (s + p/det F I) F^-T.  (The golden series j2_log_h1_p2 is reproduced by exactly this.) */
static int j2log_stress(const oracle_material* m, int dim, double dt, int accumulate, int polish, double* Fp_inv,
                        double* eqps, double* temperature, point_work* w, const double* delta_fixed, double* r_out) {
  double F_e[9], C_e[9], E_e[9], s[9], Np[9];
  const int dd = dim * dim;
  int status = 0;
  mat_mul(w->F, Fp_inv, dim, F_e);
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < dim; ++j) {
      double t = 0;
      for (int k = 0; k < dim; ++k) t += M(F_e, k, i) * M(F_e, k, j);
      M(C_e, i, j) = t;
    }
  sym_fun(C_e, dim, 0, E_e);   /* material_utils.hpp:91-114 LogarithmicStrain */
  for (int i = 0; i < dd; ++i) E_e[i] *= 0.5;
  double tr = 0;
  for (int i = 0; i < dim; ++i) tr += M(E_e, i, i);
  const double p = m->K * tr;
  dev_d(E_e, dim, 2.0 * m->G, s);
  const double q = sqrt(1.5) * norm_d(s, dim);

  rm_ctx c;
  c.m = m;
  c.eqps_old = *eqps;
  c.q = q;
  w->q = q;
  c.thermo = thermo_contribution(m, *temperature);
  c.dt = dt;
  c.slope = 3.0 * m->G;
  const double tolerance = sigma_y_of(m) * 1.e-10;
  dual zero = {0.0, 0.0};
  w->plastic = 0;
  if (delta_fixed || rm_residual(&c, zero).v > tolerance) {
    dual e0 = {c.eqps_old, 0.0};
    const double upper = (q - hardening_evaluate(m, e0).v * c.thermo) / (3.0 * m->G);
    double delta;
    if (delta_fixed) {
      dual df = {*delta_fixed, 0.0};
      delta = *delta_fixed;
      *r_out = rm_residual(&c, df).v;
    } else {
      delta = scalar_solve(&c, 0.0, 0.0, upper, 1.e-10, tolerance, 100, &status);
      if (polish) delta = polish_root(&c, delta, 0.0, upper);
    }
    w->plastic = 1;
    w->delta = delta;
    w->hprime = return_map_slope(&c, delta);
    /* (q == 0 is reached only under delta_fixed = 0, when a point of the oracle tangent's stencil is a pure dilatation:
     * s = 0 there and nothing is returned; the reference yields only with q > 0) */
    for (int i = 0; i < dd; ++i) Np[i] = q > 0.0 ? 1.5 / q * s[i] : 0.0;
    for (int i = 0; i < dd; ++i) s[i] += -2.0 * m->G * delta * Np[i];
    if (accumulate) {
      double inc[9], ex[9], old[9];
      for (int i = 0; i < dd; ++i) inc[i] = -delta * Np[i];
      sym_fun(inc, dim, 1, ex);
      *eqps += delta;
      memcpy(old, Fp_inv, sizeof(double) * dd);
      mat_mul(old, ex, dim, Fp_inv);
    }
  }
  if (!accumulate) {
    double alt[9];
    for (int i = 0; i < dd; ++i) alt[i] = s[i];
    for (int i = 0; i < dim; ++i) M(alt, i, i) += p / w->detF;
    pk1_from_sigma(dim, alt, w);
  }
  return status;
}

/* one dispatcher for the stateful extras; state pointers address ONE quadrature point */
static int other_material_stress_x(const oracle_material* m, int dim, double dt, int accumulate, int polish,
                                   double* mat1, double* mat2, double* eqps, double* temperature, point_work* w,
                                   const double* delta_fixed, double* r_out) {
  w->plastic = 0;
  switch (m->kind) {
  case MAT_STVK: if (!accumulate) stvk_pk1(m, dim, w); return 0;
  case MAT_J2LINEAR: return j2linear_stress(m, dim, accumulate, mat1, mat2, eqps, w);
  case MAT_J2SIMO:
    return j2simo_stress(m, dim, dt, accumulate, polish, mat1, mat2, eqps, temperature, w, delta_fixed, r_out);
  default: return j2log_stress(m, dim, dt, accumulate, polish, mat1, eqps, temperature, w, delta_fixed, r_out);
  }
}

static int other_material_stress(const oracle_material* m, int dim, double dt, int accumulate, int polish,
                                 double* mat1, double* mat2, double* eqps, double* temperature, point_work* w) {
  return other_material_stress_x(m, dim, dt, accumulate, polish, mat1, mat2, eqps, temperature, w, NULL, NULL);
}

/* tangent of those materials for the oracle's TANGENT_EXACT mode (not in the reference): SIXTH-ORDER central difference
 * quotients of P(F) at the POINT (round 3; rounds 1-2: second order with step 1e-6, good to ~1e-9, which capped every
 * comparison of the HIP path's tangents for these materials at 1e-6).  The quotient is always taken of a SMOOTH
 * function, so that the stencil's width (+-3 h, h = 1e-3) costs nothing:
 *   - at a yielding point of J2Simo / J2Log the increment delta is NOT re-solved under the perturbation (with power-law
 *     hardening delta(F) has an unbounded second derivative at first yield); instead
 *     dP = dP|delta + (dP/d delta) d delta,  d delta = -(dr|delta) / (dr/d delta)  with the return-map residual r,
 *     dr/d delta analytic (return_map_slope), the branch forced plastic at the fixed delta;
 *   - at an elastic point of those two the branch is forced too (delta = 0: the trial state), so that a perturbed F
 *     near the yield surface does not change formulas inside the stencil;
 *   - J2Linear's radial return is piecewise smooth in F: its branch is re-decided under the perturbation (a kink within
 *     +-3 h of the point would show; the tests' points are not that close, and its closed form is checked separately).
 * f'(x) = [45 (f1 - f-1) - 9 (f2 - f-2) + (f3 - f-3)] / (60 h) + O(h^6): truncation ~1e-16, rounding ~2e-13 |f|. */
static void stencil6(const double* fp1, const double* fm1, const double* fp2, const double* fm2, const double* fp3,
                     const double* fm3, int n, double h, double* out) {
  for (int i = 0; i < n; ++i)
    out[i] = (45.0 * (fp1[i] - fm1[i]) - 9.0 * (fp2[i] - fm2[i]) + (fp3[i] - fm3[i])) / (60.0 * h);
}

/* f'(x) = [4/5 (f1 - f-1) - 1/5 (f2 - f-2) + 4/105 (f3 - f-3) - 1/280 (f4 - f-4)] / h + O(h^8); f[2k] = f(x + (k+1) h),
 * f[2k+1] = f(x - (k+1) h) */
static void stencil8(double (*f)[9], int n, double h, double* out) {
  for (int i = 0; i < n; ++i)
    out[i] = (4.0 / 5.0 * (f[0][i] - f[1][i]) - 1.0 / 5.0 * (f[2][i] - f[3][i]) + 4.0 / 105.0 * (f[4][i] - f[5][i])
              - 1.0 / 280.0 * (f[6][i] - f[7][i])) / h;
}

static void difference_tangent(const oracle_material* m, int dim, double dt, double* mat1, double* mat2, double* eqps,
                               double* temperature, const point_work* w0, double* A) {
  double h = 1.0e-3;
  const int dd = dim * dim;
  point_work wc = *w0;
  double r_unused = 0;
  /* the expansion point is the increment the reference's ScalarSolve returns (no polishing: with delta frozen under the
   * perturbation nothing needs a root to rounding, and a tangent taken at a polished root differs from one taken at the
   * solver's own by |dA/d delta| x 1e-10 -- up to 1e-9 relative where the hardening curve is steep) */
  other_material_stress_x(m, dim, dt, 0, 0, mat1, mat2, eqps, temperature, &wc, NULL, NULL);
  const int implicit = m->kind == MAT_J2SIMO || m->kind == MAT_J2LOG;   /* delta is the root of a scalar equation */
  const int frozen = implicit && wc.plastic;
  const double delta0 = frozen ? wc.delta : 0.0, slope = wc.hprime;
  const double* forced = implicit ? &delta0 : NULL;
  /* the flow direction s / |s| of a yielding point varies over F on the scale of the trial deviatoric strain e = q / 3G, and
   * the stencil must stay well inside it: yielding points take the EIGHTH-order stencil with h = min(1e-3, e / 28).  (With
   * the sixth-order one at h = 1e-3 the quotient is off by ~ 2 w (h / e)^6, w the share of the trial stress that is
   * returned: under 1e-10 for the slightly yielding points of a cold law, but 1e-5 relative at a melted point -- thermo = 0,
   * it yields at any strain and w = 1 -- with 0.5 % strain, and still 2e-10 at 4 % strain.) */
  const int narrow = frozen;
  if (narrow && wc.q / (3.0 * m->G * 28.0) < h) h = wc.q / (3.0 * m->G * 28.0);
  const int n_s = narrow ? 8 : 6;
  double dP_ddelta[9] = {0};
  if (frozen) {
    const double k = 2.0e-2 * (fabs(delta0) + 1.0e-3);
    double P[6][9];
    for (int s_ = 0; s_ < 6; ++s_) {
      point_work wp = *w0;
      const double d = delta0 + (s_ % 2 ? -1.0 : 1.0) * (s_ / 2 + 1) * k;
      other_material_stress_x(m, dim, dt, 0, 1, mat1, mat2, eqps, temperature, &wp, &d, &r_unused);
      memcpy(P[s_], wp.P, sizeof(double) * dd);
    }
    stencil6(P[0], P[1], P[2], P[3], P[4], P[5], dd, k, dP_ddelta);
  }
  for (int j = 0; j < dim; ++j)
    for (int L = 0; L < dim; ++L) {
      double P[8][9], r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int s_ = 0; s_ < n_s; ++s_) {
        point_work wp = *w0;
        M(wp.F, j, L) += (s_ % 2 ? -1.0 : 1.0) * (s_ / 2 + 1) * h;
        wp.detF = det_d(wp.F, dim);
        inv_d(wp.F, dim, wp.Finv);
        other_material_stress_x(m, dim, dt, 0, 1, mat1, mat2, eqps, temperature, &wp, forced, &r[s_]);
        memcpy(P[s_], wp.P, sizeof(double) * dd);
      }
      double dP[9], dr = 0.0;
      if (narrow) {
        stencil8(P, dd, h, dP);
        double r9[8][9];
        for (int s_ = 0; s_ < 8; ++s_) r9[s_][0] = r[s_];
        stencil8(r9, 1, h, &dr);
      } else {
        stencil6(P[0], P[1], P[2], P[3], P[4], P[5], dd, h, dP);
        stencil6(&r[0], &r[1], &r[2], &r[3], &r[4], &r[5], 1, h, &dr);
      }
      const double ddelta = frozen ? dr / slope : 0.0;
      for (int i = 0; i < dim; ++i)
        for (int Jx = 0; Jx < dim; ++Jx)
          A[((i * dim + Jx) * dim + j) * dim + L] = M(dP, i, Jx) + M(dP_ddelta, i, Jx) * ddelta;
    }
}

/* dP_iJ/dF_jL, exact, stored A[((i*dim+J)*dim+j)*dim+L]  (not in the reference: the
 * reference differentiates numerically, nonlinear_solid.cpp:48-76) */
static void exact_tangent(const oracle_material* m, int dim, const point_work* w, double* A) {
  const double J = w->detF;
  const double* Fi = w->Finv; /* Finv(J,k) ; F^-T(k,J) = Finv(J,k) */
  if (m->kind == MAT_NEOHOOKEAN) {
    const double c1 = m->lambda * J * (J - 1.) - m->mu;
    const double c2 = m->lambda * (2. * J - 1.) * J;
    for (int i = 0; i < dim; ++i)
      for (int Jx = 0; Jx < dim; ++Jx)
        for (int j = 0; j < dim; ++j)
          for (int L = 0; L < dim; ++L) {
            double v = (i == j && Jx == L) ? m->mu : 0.0;
            v += -c1 * M(Fi, L, i) * M(Fi, Jx, j);
            v += c2 * M(Fi, L, j) * M(Fi, Jx, i);
            A[((i * dim + Jx) * dim + j) * dim + L] = v;
          }
    return;
  }
  /* J2: P_iJ = J sigma_ik Finv_Jk ; sigma from small-strain radial return */
  double beta = 1.0, gamma = 0.0;
  if (w->plastic) {
    const double q = w->q, G = m->G;
    beta = 1.0 - 3.0 * G * w->delta / q;
    gamma = 3.0 * G * (1.5 / q) * (1.0 / ((3.0 * G + w->hprime) * q) - w->delta / (q * q));
  }
  const double G2 = 2.0 * m->G;
  for (int i = 0; i < dim; ++i)
    for (int Jx = 0; Jx < dim; ++Jx)
      for (int j = 0; j < dim; ++j)
        for (int L = 0; L < dim; ++L) {
          double v = 0.0;
          for (int k = 0; k < dim; ++k) {
            /* sigma_ik d(J Finv_Jk)/dF_jL */
            v += M(w->sigma, i, k) * J * (M(Fi, L, j) * M(Fi, Jx, k) - M(Fi, Jx, j) * M(Fi, L, k));
            /* J dsigma_ik/dF_jL Finv_Jk */
            double C = (i == k && j == L ? m->K : 0.0);
            C += beta * G2 * (0.5 * ((i == j && k == L ? 1.0 : 0.0) + (i == L && k == j ? 1.0 : 0.0))
                              - (i == k && j == L ? 1.0 / (double)dim : 0.0));
            C -= G2 * gamma * M(w->s_trial, i, k) * M(w->s_trial, j, L);
            v += J * C * M(Fi, Jx, k);
          }
          A[((i * dim + Jx) * dim + j) * dim + L] = v;
        }
}

/* ---- integrator ----------------------------------------------------------- */
/* integrator_utils.cpp:33-40  ComputeF: F = x_e^T dN_dX + I */
static void compute_F(int dim, int n_dof, const double* x_e, const double* dNdX, point_work* w) {
  for (int i = 0; i < dim; ++i)
    for (int J = 0; J < dim; ++J) {
      double s = 0;
      for (int a = 0; a < n_dof; ++a) s += x_e[a + i * n_dof] * dNdX[a + J * n_dof];
      M(w->F, i, J) = s;
    }
  for (int i = 0; i < dim; ++i) M(w->F, i, i) += 1.0;
  w->detF = det_d(w->F, dim);
  inv_d(w->F, dim, w->Finv);
}

static int evaluate_pk1(const oracle_domain* D, int e, int q, point_work* w) {
  if (D->mat.kind == MAT_NEOHOOKEAN) {
    neo_hookean_pk1(&D->mat, D->dim, w);
    return 0;
  }
  const long pt = (long)e * D->n_q + q;
  const int dd = D->dim * D->dim;
  if (D->mat.kind != MAT_J2)
    return other_material_stress(&D->mat, D->dim, D->dt, 0, 0, D->plastic_strain + pt * dd,
                                 D->state2 ? D->state2 + pt * dd : NULL, D->eqps + pt, D->temperature + pt, w);
  return j2_plastic_stress(&D->mat, D->dim, D->dt, 0, D->plastic_strain + pt * D->dim * D->dim,
                           D->eqps + pt, D->temperature + pt, w);
}

static void point_tangent(const oracle_domain* D, long pt, const point_work* w, double* A) {
  const int dd = D->dim * D->dim;
  if (D->mat.kind == MAT_NEOHOOKEAN || D->mat.kind == MAT_J2 || D->mat.kind == MAT_J2LINEAR) {
    exact_tangent(&D->mat, D->dim, w, A);
    return;
  }
  difference_tangent(&D->mat, D->dim, D->dt, D->plastic_strain + pt * dd, D->state2 ? D->state2 + pt * dd : NULL,
                     D->eqps + pt, D->temperature + pt, w, A);
}

/* nonlinear_solid.hpp:65-87  ElementResidual<false>:
 *   R_e = sum_q (w_q det_q) dN_dX_q P(F_q)^T   (AddMult_a_ABt) */
static int element_residual(const oracle_domain* D, int e, const double* x_e, double* R_e) {
  const int dim = D->dim, n_dof = D->n_dof;
  int status = 0;
  memset(R_e, 0, sizeof(double) * n_dof * dim);
  for (int q = 0; q < D->n_q; ++q) {
    const long pt = (long)e * D->n_q + q;
    const double* dNdX = D->dN_dX + pt * n_dof * dim;
    point_work w;
    compute_F(dim, n_dof, x_e, dNdX, &w);
    status |= evaluate_pk1(D, e, q, &w);
    const double a = D->weight[pt] * D->det[pt];
    for (int i = 0; i < dim; ++i)
      for (int J = 0; J < dim; ++J) {
        const double aP = a * M(w.P, i, J);
        for (int n = 0; n < n_dof; ++n) R_e[n + i * n_dof] += dNdX[n + J * n_dof] * aP;
      }
  }
  return status;
}

/* nonlinear_solid.cpp:48-76  ElementResidualAndGrad: forward finite differences,
 * step |u_i|*1e-8 or 1e-10, K_e column i = (R(u+h e_i) - R(u))/h */
static int element_residual_and_grad_fd(const oracle_domain* D, int e, double* x_e, double* R_e,
                                        double* K_e) {
  const int n_tdof = D->n_dof * D->dim;
  double fwd[MAX_TDOF];
  int status = element_residual(D, e, x_e, R_e);
  double* g = K_e;
  for (int i = 0; i < n_tdof; ++i) {
    const double orig = x_e[i];
    const double step = (orig != 0.0) ? fabs(orig) * 1.0e-8 : 1.0e-10;
    const double step_inv = 1. / step;
    x_e[i] = orig + step;
    status |= element_residual(D, e, x_e, fwd);
    for (int j = 0; j < n_tdof; ++j) *g++ = (fwd[j] - R_e[j]) * step_inv;
    x_e[i] = orig;
  }
  return status;
}

/* exact tangent counterpart: K_e[(a,i),(b,j)] = sum_q w det dN_aJ A_iJjL dN_bL */
static int element_residual_and_grad_exact(const oracle_domain* D, int e, const double* x_e,
                                           double* R_e, double* K_e) {
  const int dim = D->dim, n_dof = D->n_dof, n_tdof = n_dof * dim;
  int status = 0;
  memset(R_e, 0, sizeof(double) * n_tdof);
  memset(K_e, 0, sizeof(double) * n_tdof * n_tdof);
  for (int q = 0; q < D->n_q; ++q) {
    const long pt = (long)e * D->n_q + q;
    const double* dNdX = D->dN_dX + pt * n_dof * dim;
    point_work w;
    double A[81];
    compute_F(dim, n_dof, x_e, dNdX, &w);
    status |= evaluate_pk1(D, e, q, &w);
    point_tangent(D, pt, &w, A);
    const double wd = D->weight[pt] * D->det[pt];
    for (int i = 0; i < dim; ++i)
      for (int J = 0; J < dim; ++J) {
        const double aP = wd * M(w.P, i, J);
        for (int n = 0; n < n_dof; ++n) R_e[n + i * n_dof] += dNdX[n + J * n_dof] * aP;
      }
    for (int j = 0; j < dim; ++j)
      for (int b = 0; b < n_dof; ++b) {
        /* t[i][J] = sum_L A_iJjL dN_bL */
        double t[9];
        for (int i = 0; i < dim; ++i)
          for (int J = 0; J < dim; ++J) {
            double s = 0;
            for (int L = 0; L < dim; ++L) s += A[((i * dim + J) * dim + j) * dim + L] * dNdX[b + L * n_dof];
            t[i * dim + J] = s * wd;
          }
        double* col = K_e + (long)(b + j * n_dof) * n_tdof;
        for (int i = 0; i < dim; ++i)
          for (int a = 0; a < n_dof; ++a) {
            double s = 0;
            for (int J = 0; J < dim; ++J) s += dNdX[a + J * n_dof] * t[i * dim + J];
            col[a + i * n_dof] += s;
          }
      }
  }
  return status;
}

/* element-level entry for tests */
int oracle_element_residual_and_grad(const oracle_domain* D, int e, const double* u, int mode,
                                     double* R_e, double* K_e) {
  const int n_tdof = D->n_dof * D->dim;
  double x_e[MAX_TDOF];
  const int* vd = D->v_dofs + (long)e * n_tdof;
  for (int k = 0; k < n_tdof; ++k) x_e[k] = u[vd[k]];
  if (mode == TANGENT_FD) return element_residual_and_grad_fd(D, e, x_e, R_e, K_e);
  return element_residual_and_grad_exact(D, e, x_e, R_e, K_e);
}

/* The reference keeps its per-thread arrays in work_data_ (integrator_utils.hpp:49-50): mfem::Vector::SetSize in
 * nonlinear_solid.cpp:117-121 allocates on the first call only, later calls just zero them.  Same here: grow-only
 * buffers, so that a timed call pays the zeroing and the reduction but not the page faults of a fresh allocation. */
static double* tl_buffer(double** slot, size_t* have, size_t need) {
  if (need > *have) {
    free(*slot);
    *slot = (double*)malloc(sizeof(double) * need);
    *have = *slot ? need : 0;
  }
  return *slot;
}
static double* g_tlr = 0;
static double* g_tlA = 0;
static size_t g_tlr_n = 0, g_tlA_n = 0;
void oracle_release_thread_local(void) {
  free(g_tlr);
  free(g_tlA);
  g_tlr = g_tlA = 0;
  g_tlr_n = g_tlA_n = 0;
}

/* nonlinear_solid.cpp:78-105 ThreadLocalResidual + nonlinear_base.hpp:90-107
 * AddThreadLocalResidual: per-thread full-size vectors, then a chunked reduction */
int oracle_add_domain_residual(const oracle_domain* D, const double* u, double* r, int n_threads) {
  const int n_tdof = D->n_dof * D->dim;
  if (n_threads < 1) n_threads = 1;
  if (n_threads > D->n_el) n_threads = D->n_el;
  double* tl = tl_buffer(&g_tlr, &g_tlr_n, (size_t)n_threads * D->n_vdofs);
  if (!tl) return -1;
  int status = 0;
#pragma omp parallel for num_threads(n_threads) reduction(| : status)
  for (int t = 0; t < n_threads; ++t) {
    long b, en;
    chunk_rule(D->n_el, n_threads, t, &b, &en);
    double* tr = tl + (size_t)t * D->n_vdofs;
    memset(tr, 0, sizeof(double) * D->n_vdofs);
    double x_e[MAX_TDOF], R_e[MAX_TDOF];
    for (long e = b; e < en; ++e) {
      const int* vd = D->v_dofs + e * n_tdof;
      for (int k = 0; k < n_tdof; ++k) x_e[k] = u[vd[k]];
      status |= element_residual(D, (int)e, x_e, R_e);
      for (int k = 0; k < n_tdof; ++k) tr[vd[k]] += R_e[k];
    }
  }
#pragma omp parallel for num_threads(n_threads)
  for (int t = 0; t < n_threads; ++t) {
    long b, en;
    chunk_rule(D->n_vdofs, n_threads, t, &b, &en);
    for (int s = 0; s < n_threads; ++s) {
      const double* tr = tl + (size_t)s * D->n_vdofs;
      for (long j = b; j < en; ++j) r[j] += tr[j];
    }
  }
  return status;
}

/* nonlinear_solid.cpp:107-149 ThreadLocalResidualAndGrad + nonlinear_base.hpp:112-151
 * AddThreadLocalResidualAndGrad: per-thread full-size residual AND nnz-sized value
 * arrays, zeroed every call, A[A_ids[k]] += K_e[k], then
 * A += grad_factor * sum_t A_t in chunks.  mode selects FD (reference) or exact. */
int oracle_add_domain_residual_and_grad(const oracle_domain* D, const double* u, double grad_factor,
                                        double* r, double* A, long nnz, int n_threads, int mode) {
  const int n_tdof = D->n_dof * D->dim;
  if (n_threads < 1) n_threads = 1;
  if (n_threads > D->n_el) n_threads = D->n_el;
  double* tlr = tl_buffer(&g_tlr, &g_tlr_n, (size_t)n_threads * D->n_vdofs);
  double* tlA = tl_buffer(&g_tlA, &g_tlA_n, (size_t)n_threads * nnz);
  if (!tlr || !tlA) return -1;
  int status = 0;
#pragma omp parallel for num_threads(n_threads) reduction(| : status)
  for (int t = 0; t < n_threads; ++t) {
    long b, en;
    chunk_rule(D->n_el, n_threads, t, &b, &en);
    double* tr = tlr + (size_t)t * D->n_vdofs;
    double* tA = tlA + (size_t)t * nnz;
    memset(tr, 0, sizeof(double) * D->n_vdofs);
    memset(tA, 0, sizeof(double) * nnz);
    double x_e[MAX_TDOF], R_e[MAX_TDOF];
    double* K_e = (double*)malloc(sizeof(double) * n_tdof * n_tdof);
    if (mode == TANGENT_NONE) en = b;   /* timing probe: the zeroing and the reduction pass alone */
    for (long e = b; e < en; ++e) {
      const int* vd = D->v_dofs + e * n_tdof;
      for (int k = 0; k < n_tdof; ++k) x_e[k] = u[vd[k]];
      if (mode == TANGENT_FD)
        status |= element_residual_and_grad_fd(D, (int)e, x_e, R_e, K_e);
      else
        status |= element_residual_and_grad_exact(D, (int)e, x_e, R_e, K_e);
      for (int k = 0; k < n_tdof; ++k) tr[vd[k]] += R_e[k];
      const int* ids = D->a_ids + e * (long)n_tdof * n_tdof;
      for (int k = 0; k < n_tdof * n_tdof; ++k) tA[ids[k]] += K_e[k];
    }
    free(K_e);
  }
#pragma omp parallel for num_threads(n_threads)
  for (int t = 0; t < n_threads; ++t) {
    long rb, re, gb, ge;
    chunk_rule(D->n_vdofs, n_threads, t, &rb, &re);
    chunk_rule(nnz, n_threads, t, &gb, &ge);
    for (int s = 0; s < n_threads; ++s) {
      const double* tr = tlr + (size_t)s * D->n_vdofs;
      for (long j = rb; j < re; ++j) r[j] += tr[j];
      const double* tA = tlA + (size_t)s * nnz;
      for (long j = gb; j < ge; ++j) A[j] += grad_factor * tA[j];
    }
  }
  return status;
}

/* nonlinear_solid.cpp:179-199 DomainPostTimeAdvance -> ElementResidual<true> ->
 * J2::Accumulate (materials.hpp:399-402) */
int oracle_domain_post_time_advance(const oracle_domain* D, const double* u, int n_threads) {
  if (D->mat.kind == MAT_NEOHOOKEAN || D->mat.kind == MAT_STVK) return 0;
  const int dim = D->dim, n_dof = D->n_dof, n_tdof = n_dof * dim;
  if (n_threads < 1) n_threads = 1;
  if (n_threads > D->n_el) n_threads = D->n_el;
  int status = 0;
#pragma omp parallel for num_threads(n_threads) reduction(| : status)
  for (int t = 0; t < n_threads; ++t) {
    long b, en;
    chunk_rule(D->n_el, n_threads, t, &b, &en);
    double x_e[MAX_TDOF];
    for (long e = b; e < en; ++e) {
      const int* vd = D->v_dofs + e * n_tdof;
      for (int k = 0; k < n_tdof; ++k) x_e[k] = u[vd[k]];
      for (int q = 0; q < D->n_q; ++q) {
        const long pt = e * D->n_q + q;
        point_work w;
        compute_F(dim, n_dof, x_e, D->dN_dX + pt * n_dof * dim, &w);
        if (D->mat.kind == MAT_J2)
          status |= j2_plastic_stress(&D->mat, dim, D->dt, 1, D->plastic_strain + pt * dim * dim,
                                      D->eqps + pt, D->temperature + pt, &w);
        else
          status |= other_material_stress(&D->mat, dim, D->dt, 1, 0, D->plastic_strain + pt * dim * dim,
                                          D->state2 ? D->state2 + pt * dim * dim : NULL, D->eqps + pt,
                                          D->temperature + pt, &w);
      }
    }
  }
  return status;
}

/* point-level entry for tests: F (column-major dim x dim) -> P and exact dP/dF */
int oracle_point_pk1(const oracle_material* m, int dim, double dt, const double* F,
                     const double* plastic_strain, double eqps, double temperature, double* P,
                     double* A, const double* state2) {
  point_work w;
  memcpy(w.F, F, sizeof(double) * dim * dim);
  w.detF = det_d(w.F, dim);
  inv_d(w.F, dim, w.Finv);
  int status = 0;
  if (m->kind == MAT_NEOHOOKEAN) {
    neo_hookean_pk1(m, dim, &w);
  } else if (m->kind != MAT_J2) {
    double m1[9] = {0}, m2[9] = {0};
    if (plastic_strain) memcpy(m1, plastic_strain, sizeof(double) * dim * dim);
    if (state2) memcpy(m2, state2, sizeof(double) * dim * dim);
    status = other_material_stress(m, dim, dt, 0, 0, m1, m2, &eqps, &temperature, &w);
    memcpy(P, w.P, sizeof(double) * dim * dim);
    if (A && m->kind == MAT_J2LINEAR) exact_tangent(m, dim, &w, A);
    else if (A) difference_tangent(m, dim, dt, m1, m2, &eqps, &temperature, &w, A);
    return status;
  } else {
    double ps[9];
    memcpy(ps, plastic_strain, sizeof(double) * dim * dim);
    status = j2_plastic_stress(m, dim, dt, 0, ps, &eqps, &temperature, &w);
  }
  memcpy(P, w.P, sizeof(double) * dim * dim);
  if (A) exact_tangent(m, dim, &w, A);
  return status;
}

int oracle_max_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}
