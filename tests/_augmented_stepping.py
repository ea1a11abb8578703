"""The augmentation loop of NonlinearSolid.step_time2 around the augmented contact law, restated on the CPU in float64 and
joined from pieces that share no code with mimi_amd: oracle.harness (Operator, line_search_newton, GeneralizedAlpha2's
factors), tests/_cases.balken_oracle (the golden neo-Hookean beam), tests/_augmented_reference.py (the law and its
consistent tangent, long double, rounded to doubles on output).  tests/_friction_stepping.py is for friction what this is for
augmentation.

Scenario: the beam of tests/test_boundary_action_gpu._beam (5 x 1, degree 3, 2 x 2 elements, clamped at x = 0, body force -5,
dt 0.05, Newton 1e-12 / 1e-8 / 10 iterations from zero), the rigid plane PLANE_BELOW = 0.02 heights BELOW its lower edge, so
that the beam falls onto it in the third step (IMPACT_STEP); STEPS = 4 steps, AUGMENTATIONS = 8 per step, gap tolerance 0.
A step is: predict; Newton; then measure the violation max |dlambda_i| / eps, stop when it is zero or after 8 updates, else
lambda <- p and Newton again (from zero, as the beam's Newton is not iterative) -- the loop of step_time2.  Before the impact
every multiplier and every nodal pressure is zero, dlambda = min(-lambda, eps gt) = 0 exactly, and the loop ends at once.

The Jacobian is dense: M + fac0 K_domain from the oracle's CSR values plus fac0 times the reference's consistent contact
tangent, which leaves the CSR pattern; Dirichlet rows and columns are eliminated as Operator does.

Figures (tests/test_augmented_cpu.py asserts: every Newton solve converges, every step that starts with a positive violation
ends at no more than RATIO_BAR of it, the impact step starts positive).  The Uzawa loop contracts like k / (k + eps), k the
effective stiffness under the contact including the inertia term rho / (beta dt^2):
    eps = 1e4, impact step: ratio 1.85e-3 of the bar 1/100;  eps = 2e3: 1.2e-2 of the bar 1/25."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import _augmented_reference as ar
import _face_reference as fr
from oracle import harness as hz

LD = np.longdouble
PLANE_BELOW, STEPS, AUGMENTATIONS, IMPACT_STEP, GAP_TOLERANCE = 0.02, 4, 8, 2, 0.0
RATIO_BAR = {1.0e4: 1.0 / 100.0, 2.0e3: 1.0 / 25.0}


class AugmentedContact:
    """the augmented law on one face of an oracle patch against a plane / sphere dict, with its multipliers"""

    def __init__(self, patch, axis, side, body, penalty, order=-1):
        self.dim = patch.dim
        self.fb = fr.face_basis(tuple(patch.p), patch.knots, axis, side, order)
        self.X = patch.ctrl.astype(LD)
        self.body, self.penalty = body, penalty
        self.lam = np.zeros(len(fr.face_node_ids(self.fb.n_ctrl, axis, side)))

    def evaluate(self, x, fac=1.0, with_tangent=False):
        pts = fr.face_points(self.fb, self.X + np.asarray(x, dtype=LD).reshape(-1, self.dim))
        return ar.augmented_contact(pts, self.body, self.penalty, self.lam, fac, with_tangent)

    def add_boundary_residual(self, x, y):
        y += np.asarray(self.evaluate(x).r, dtype=np.float64)

    def update(self, x, apply):
        """the violation at x; apply: lambda <- p"""
        out = self.evaluate(x)
        if apply:
            self.lam = np.asarray(out.pressure, dtype=np.float64)
        return float(out.violation), out


class AugmentedOperator(hz.Operator):
    """Operator with a dense Jacobian: the contact's consistent tangent reaches past the CSR pattern"""

    def _csr(self, vals):
        return sp.csr_matrix(vals) if np.ndim(vals) == 2 else super()._csr(vals)

    def residual_and_grad(self, a):
        contact, self.contact = self.contact, None
        try:
            y, jac = super().residual_and_grad(a)                     # (everything but the contact)
        finally:
            self.contact = contact
        out = contact.evaluate(self.x + self.fac0 * a, self.fac0, with_tangent=True)
        keep = np.ones(self.n)
        keep[self.dirichlet] = 0.0
        y = y + keep * np.asarray(out.r, dtype=np.float64)
        J = super()._csr(jac).toarray() + keep[:, None] * np.asarray(out.K, dtype=np.float64) * keep[None, :]
        return y, J


def system(penalty):
    from _cases import balken_oracle
    P, D, op0, ode, dt = balken_oracle("neohook")
    y0, height = P.ctrl[:, 1].min(), P.ctrl[:, 1].max() - P.ctrl[:, 1].min()
    body = dict(kind="plane", point=[0.0, float(y0 - PLANE_BELOW * height)], normal=[0.0, 1.0])
    contact = AugmentedContact(P, 1, 0, body, penalty)
    # (op0 eliminated its copies; the mass values and the right-hand side are rebuilt from the same routines)
    mass = hz.assemble_mass(P, D.tables, 1.0, D.rowptr, D.col)
    rhs = hz.assemble_body_force(P, D.tables, [0.0, -5.0])
    op = AugmentedOperator(D, D.rowptr, D.col, mass, rhs, op0.dirichlet, contact=contact)
    ode = hz.GeneralizedAlpha2(op, 0.5, dict(ode.newton_opts))
    return types.SimpleNamespace(P=P, op=op, ode=ode, contact=contact, dt=dt, body=body)


def step(S, x, v, n_aug=AUGMENTATIONS, tol=GAP_TOLERANCE):
    """GeneralizedAlpha2.step with the augmentation loop between the solve and the commit"""
    ode, op, dt = S.ode, S.op, S.dt
    op.dt = dt
    if ode.nstate == 0:
        op.v0 = v
        ode.a = op.explicit_accel(x)
        ode.nstate = 1
        ode.aa = np.zeros_like(x)
    a = ode.a
    xa = x + (v + ode.fac0 * dt * a) * (ode.fac1 * dt)
    va = v + ode.fac2 * dt * a
    f3, f4 = ode.fac3 * dt * dt, ode.fac4 * dt
    op.set_parameters(f3, f4, xa, va)
    newton, violations, applied = [], [], 0
    ode.aa, info = hz.line_search_newton(op, ode.aa, **ode.newton_opts)
    newton.append(info)
    while True:
        violations.append(S.contact.update(xa + f3 * ode.aa, apply=False)[0])
        if violations[-1] <= tol or applied >= n_aug:
            break
        S.contact.update(xa + f3 * ode.aa, apply=True)
        applied += 1
        ode.aa, info = hz.line_search_newton(op, ode.aa, **ode.newton_opts)
        newton.append(info)
    xa, va = xa + f3 * ode.aa, va + f4 * ode.aa
    prev = 1.0 - 1.0 / ode.fac1
    x[:] = x * prev + xa / ode.fac1
    v[:] = v * prev + va / ode.fac1
    ode.a = a * prev + ode.aa / ode.fac5
    op.post_time_advance(x)
    return types.SimpleNamespace(newton=newton, violations=violations, x=x.copy(), lam=S.contact.lam.copy())


@functools.lru_cache(maxsize=None)
def run(penalty, n_aug=AUGMENTATIONS):
    S = system(penalty)
    x, v = np.zeros(S.P.n_vdofs), np.zeros(S.P.n_vdofs)
    steps = [step(S, x, v, n_aug) for _ in range(STEPS)]
    return types.SimpleNamespace(steps=steps, x=x, body=S.body)
