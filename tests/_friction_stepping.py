"""The time-stepping routes around the friction kernels, restated on the CPU from the model of DESIGN 4.6a and joined from
pieces that share no code with mimi_amd: oracle.harness (Operator, line_search_newton, GeneralizedAlpha2),
tests/_explicit_reference.py (Stepper), tests/_face_reference.py (mortar_contact, long double), tests/_friction_reference.py
(evaluate, long double) and tests/_spline_bodies.py (circle, whose analytic twin is a sphere).

RoughContact is the `contact` of oracle.harness.Operator: the normal part fr.mortar_contact, the friction part fq.evaluate
against the object's OWN committed state (xi, xbar, c) and its d, summed in long double and rounded to float64 on output,
the dense tangent scattered onto the oracle pattern's CSR values.  An evaluation never touches the committed state;
post_time_advance(x) evaluates at x and replaces it by the trial state.  `body` and `d` are plain attributes.  Every
evaluation is logged with the two margins the exact comparisons rest on:
    gate   the smallest |g| / extent over the face's points, g the signed distance to the body.  (A node's mortar gap g_A =
           sum_q N_A da min(g_q, 0) is EXACTLY zero while no point it sees penetrates, so the nodal value has no margin to
           measure; it, the nodal pressure and with them the gate p_N > 0 of every point change status exactly when some
           g_q changes sign, and that is the distance recorded.)
    kink   the smallest |eps_T |s| / (mu p_N) - 1| over the points that carry a traction.
RoughOperator commits the contact with the domain; ConstantVelocityAlpha2 is the generalized-alpha step with
constant-velocity dofs: before the solve aa = 0, va = vbar, xa = x + vbar dt on them, after the extrapolation x = the saved
xa, v = vbar, a = 0.

Scenarios (tests/test_friction_stepping_cpu.py asserts what each gives: stick and slip, points entering and leaving contact,
gate and kink margins >= 1e-9 at every evaluation resp. every compared sample):
  slide     the block of tests/test_friction_solid_gpu.py (4 x 2 elements, degree 2, on the plane y = 0, mu 0.3, penalty
            1e2), its top driven down for 3 steps and sideways for 6.  Values used: the block starts PRESS = 1e-3 inside the
            plane (a rigid translation set through the solution view: at rest on y = 0 every g is exactly 0 at the first
            evaluation, which has no gate margin), travel per step 0.003 down and 0.03 sideways (at that test's 0.01 / 0.004
            no step has sticking and slipping points together; here the first sideways step has 2 and 14).
            NO POINT LEAVES CONTACT in this scenario, at any drive amplitude tried (down 1e-4 .. 1e-2, sideways 0.03 .. 0.2,
            press 1e-4 .. 1e-3): p_N = -sum N_A p_A of a point vanishes only when no point of the three elements its nodes
            see penetrates, the edge has four elements, and the top edge is held level.  The CPU test asserts that (left ==
            0) for this scenario and "at least one leaves" for the other three.
  punch     a 6 x 3 block, degree 2, bottom clamped, under the NURBS circle sb.circle(L, "up") lifted by PUNCH_LIFT = 0.16
            (0.01 above the top edge), which descends 0.02 per step for 3 steps and slides 0.1 per step for 5; mu 0.3,
            penalty 1e2, eps_T = PUNCH_EPS_T = 10.  The contact patch is narrower than an element and crosses from one
            element into the next, so the points of the first element leave.
  e_run     the 200-step contact run of tests/_explicit_cases.py with friction 0.3 on its plane (ec.e_reference("friction")).
  e_short   twelve explicit steps on cube_p2 from a displacement pressed 2 E_GAP into that plane; initial velocity at the top
            SHORT_V = (0.4, 0.2) along the plane and +-0.5 into / out of it at x = 0 / x = max.  The face rubs (stick, then
            slip) for eight steps and leaves; x, v and the state are compared after 6 steps (in contact) and after 12.

Bars.  Lock-step (implicit routes): the restatement solves nothing; per step it is evaluated at the product's own alpha-level
vectors and acceleration, and
    |op.mult(aa_product)|_2 <= max(rel_tol |op.mult(aa_start)|_2, abs_tol) + slack,
    slack = sum over the terms T in (inertia M aa, domain, contact, friction) of bar_T sqrt(n) max|T|,
with the Newton tolerances the test configures (1e-10, 1e-9), the restatement's own initial residual, bar = RESIDUAL_BAR =
1e-12 for inertia and domain, fc.TOL["contact_r"] = 1e-12 for contact and friction: each entry of a term the device formed
may be off by its bar relative to the term's largest entry, and sqrt(n) takes n such entries into the 2-norm.  For the
spline punch the contact term's bar is the one tests/test_contact_spline_gpu.py holds this circle to against its analytic
twin, sb.bound(sb.MEASURED_TWIN["6x3-p2-circle-seam-up"]) = 1e-13 (relative to the largest entry, so the penalty scales it).
The predictor is held to 16 x 2^-53 max|.|.  Explicit short run: spread / MARGIN between the restatement and the restatement
whose domain residual is moved by its bar and whose contact + friction residual by fc.TOL["contact_r"] max|r_c + r_f|, random
signs (ec.bars' method)."""
import functools
import types

import numpy as np

import _explicit_cases as ec
import _explicit_reference as er
import _face_cases as fc
import _face_reference as fr
import _friction_reference as fq
import _spline_bodies as sb
from oracle import harness as hz

LD = np.longdouble
MU, PENALTY, DT, RHO_INF = 0.3, 1.0e2, 0.05, 0.25
NEWTON = dict(rel_tol=1e-10, abs_tol=1e-9, max_iter=40, iterative_mode=False)
RESIDUAL_BAR = ec.RESIDUAL_BAR
PREDICTOR_BAR = 16 * 2.0 ** -53
MARGIN_MIN = 1e-9
# fx.XI_TOL is relative to the largest entry of xi and was sized on slips of 0.25 fc.U_SCALE = 5e-3 extents (tests/_friction_cases.py:
# "x_q - xbar at increments of 5e-3 of the extent costs about 1e-13"); the error is the rounding of the coordinates, whatever the
# slip, so a step that only presses (slips of 1e-4 extents and less) is held to the same absolute accuracy: the scale of the
# comparison is max(max|xi|, XI_FLOOR extents)
XI_FLOOR = 0.25 * fc.U_SCALE
# slide
SLIDE_N_EL, SLIDE_LENGTHS, PRESS = (4, 2), (4.0, 2.0), 1.0e-3
SLIDE_DOWN, SLIDE_SIDE = (3, 0.003), (6, 0.03)
# punch
PUNCH_N_EL, PUNCH_LIFT, PUNCH_DOWN, PUNCH_SIDE, PUNCH_EPS_T = (6, 3), 0.16, (3, 0.02), (5, 0.1), 10.0
PUNCH_TWIN_BAR = sb.bound(sb.MEASURED_TWIN["6x3-p2-circle-seam-up"])
# e_short
SHORT_STEPS, SHORT_SHOTS, SHORT_V = 12, (6, 12), (0.4, 0.2, 0.5)   # v0 at the top: x, y, and z = +-SHORT_V[2] at x = 0 / max


class RoughContact:
    """mortar contact with Coulomb friction on one face of an oracle patch against dict(kind="plane" | "sphere", ...)"""

    def __init__(self, patch, axis, side, body, penalty, mu, eps_t, order=-1):
        self.dim = patch.dim
        self.fb = fr.face_basis(tuple(patch.p), patch.knots, axis, side, order)
        self.X = patch.ctrl.astype(LD)
        self.body, self.penalty, self.mu, self.eps_t, self.d = body, penalty, mu, eps_t, None
        self.rowptr, self.col = patch.sparsity()
        self.rows = np.repeat(np.arange(len(self.rowptr) - 1), np.diff(self.rowptr))
        self.state = fq.initial_state(len(self.fb.w), self.dim)
        p0 = fr.face_points(self.fb, self.X)
        centroid = (p0.da[:, None] * p0.x).sum(axis=0) / p0.da.sum()
        self.extent = float(np.linalg.norm((p0.x - centroid).astype(np.float64), axis=1).max())
        self.log = []
        self.entered = self.left = 0
        self.n_stick = self.n_slip = 0
        self.friction_force, self.friction_traction = np.zeros(self.dim), 0.0
        self.r_contact = self.r_friction = None

    def evaluate(self, x, fac=1.0, with_tangent=False):
        """(contact, friction evaluation or None) at the displacement x; the history attributes are those of this call"""
        pts = fr.face_points(self.fb, self.X + np.asarray(x, dtype=LD).reshape(-1, self.dim))
        con = fr.mortar_contact(pts, self.body, self.penalty, fac, with_tangent)
        ev = None
        entry = dict(gate=float(np.abs(con.g).min()) / self.extent, kink=np.inf, n_stick=0, n_slip=0)
        self.r_contact, self.r_friction = np.asarray(con.r, dtype=np.float64), np.zeros(con.r.size)
        self.n_stick = self.n_slip = 0
        self.friction_force, self.friction_traction = np.zeros(self.dim), 0.0
        if self.mu > 0.0:
            ev = fq.evaluate(pts, con, self.state, self.mu, self.eps_t, d=self.d, grad_factor=fac, with_tangent=with_tangent)
            if ev.tr.on.any():
                entry["kink"] = float(np.abs(ev.tr.ratio[ev.tr.on] - 1).min())
            entry["n_stick"], entry["n_slip"] = self.n_stick, self.n_slip = ev.n_stick, ev.n_slip
            self.r_friction = np.asarray(ev.r, dtype=np.float64)
            self.friction_force, self.friction_traction = ev.force.astype(np.float64), float(ev.traction)
        self.log.append(entry)
        self.pts = pts
        return con, ev

    def add_boundary_residual(self, x, y):
        con, ev = self.evaluate(x)
        y += np.asarray(con.r + (ev.r if ev is not None else 0), dtype=np.float64)

    def dense_tangent(self, x, fac):
        con, ev = self.evaluate(x, fac, with_tangent=True)
        return con, ev, con.K + (ev.K if ev is not None else 0)

    def add_boundary_residual_and_grad(self, x, fac, y, jac_vals, mode=0):
        con, ev, K = self.dense_tangent(x, fac)
        y += np.asarray(con.r + (ev.r if ev is not None else 0), dtype=np.float64)
        K = np.asarray(K, dtype=np.float64)
        inside = np.zeros(K.shape, dtype=bool)
        inside[self.rows, self.col] = True
        assert not np.any(K[~inside]), "the face tangent has an entry outside the pattern"
        jac_vals += K[self.rows, self.col]

    def post_time_advance(self, x):
        con, ev = self.evaluate(x)
        if ev is None:
            return
        new = ev.trial
        self.entered += int((new.c & ~self.state.c).sum())
        self.left += int((~new.c & self.state.c).sum())
        self.state = types.SimpleNamespace(xi=new.xi.copy(), xbar=new.xbar.copy(), c=new.c.copy())
        self.log[-1]["commit"] = True


class RoughOperator(hz.Operator):
    def post_time_advance(self, x):
        super().post_time_advance(x)
        self.contact.post_time_advance(x)


def predictor(ode, x, v, a, dt, cv_dofs, vbar):
    """(xa, va, saved x) at the start of a generalized-alpha step, the constant-velocity dofs applied"""
    xa = x + (v + ode.fac0 * dt * a) * (ode.fac1 * dt)
    va = v + ode.fac2 * dt * a
    va[cv_dofs] = vbar
    xa[cv_dofs] = x[cv_dofs] + vbar * dt
    return xa, va, xa[cv_dofs].copy()


class ConstantVelocityAlpha2(hz.GeneralizedAlpha2):
    """GeneralizedAlpha2 with prescribed-velocity dofs (they are among the operator's Dirichlet dofs): `cv_dofs` move with
    `vbar` (an array the caller may change between steps)"""

    def __init__(self, op, rho_inf, newton_opts, cv_dofs, vbar):
        super().__init__(op, rho_inf, newton_opts)
        self.cv_dofs, self.vbar = np.asarray(cv_dofs, dtype=np.int64), np.asarray(vbar, dtype=np.float64).copy()

    def step(self, x, v, t, dt):
        op = self.op
        op.dt = dt
        if self.nstate == 0:
            op.v0 = v
            self.a = op.explicit_accel(x)
            self.nstate = 1
            self.aa = np.zeros_like(x)
        a = self.a
        xa, va, saved = predictor(self, x, v, a, dt, self.cv_dofs, self.vbar)
        self.aa[self.cv_dofs] = 0.0
        fac3dtdt, fac4dt = self.fac3 * dt * dt, self.fac4 * dt
        op.set_parameters(fac3dtdt, fac4dt, xa, va)
        self.aa, info = hz.line_search_newton(op, self.aa, **self.newton_opts)
        self.history.append(info)
        xa = xa + fac3dtdt * self.aa
        va = va + fac4dt * self.aa
        prev = 1.0 - 1.0 / self.fac1
        x[:] = x * prev + xa / self.fac1
        v[:] = v * prev + va / self.fac1
        self.a = a * prev + self.aa / self.fac5
        x[self.cv_dofs], v[self.cv_dofs], self.a[self.cv_dofs] = saved, self.vbar, 0.0
        op.post_time_advance(x)
        return t + dt


# ---- the implicit scenarios -----------------------------------------------------------------------------------------------
def _face_dofs(P, axis, side):
    nodes = P.boundary_nodes(axis, side)
    return np.sort(np.concatenate([nodes * P.dim + c for c in range(P.dim)]))


def implicit_system(name, patch=None):
    """the restated operator, its ode and the start vectors of the scenario "slide" or "punch"; patch: the oracle patch made of
    the product's own arrays (its knots differ from iga.Patch.block's by a rounding of k / m), None: the block"""
    from oracle import iga, ref_path as rp
    if name == "slide":
        P = iga.Patch.block(SLIDE_N_EL, 2, list(SLIDE_LENGTHS)) if patch is None else patch
        body = dict(kind="plane", point=[0.0, 0.0], normal=[0.0, 1.0])
        contact = RoughContact(P, 1, 0, body, PENALTY, MU, PENALTY)
        cv = _face_dofs(P, 1, 1)
        dirichlet = cv
        vbar = np.where(cv % 2 == 0, 0.0, -SLIDE_DOWN[1] / DT)
        x0 = np.zeros(P.n_vdofs)
        x0[1::2] = -PRESS
    else:
        P = iga.Patch.block(PUNCH_N_EL, 2) if patch is None else patch
        contact = RoughContact(P, 1, 1, punch_twin(0), PENALTY, MU, PUNCH_EPS_T)
        cv, vbar = np.zeros(0, dtype=np.int64), np.zeros(0)
        dirichlet = _face_dofs(P, 1, 0)
        x0 = np.zeros(P.n_vdofs)
    D = rp.DomainOracle(P, ec.material_pair("neohook")[0])
    mass = hz.assemble_mass(P, D.tables, ec.RHO, D.rowptr, D.col)
    op = RoughOperator(D, D.rowptr, D.col, mass, np.zeros(P.n_vdofs), dirichlet, contact=contact)
    op.tangent_mode = rp.TANGENT_EXACT
    ode = ConstantVelocityAlpha2(op, RHO_INF, dict(NEWTON), cv, vbar)
    return types.SimpleNamespace(P=P, D=D, op=op, ode=ode, contact=contact, x0=x0, cv=cv, dirichlet=dirichlet)


def slide_drive(k):
    """(vx, vy) of the top edge during step k of the scenario "slide" """
    return (0.0, -SLIDE_DOWN[1] / DT) if k < SLIDE_DOWN[0] else (SLIDE_SIDE[1] / DT, 0.0)


SLIDE_STEPS = SLIDE_DOWN[0] + SLIDE_SIDE[0]


def punch_shift(k):
    return np.array([0.0, -PUNCH_DOWN[1]]) if k < PUNCH_DOWN[0] else np.array([PUNCH_SIDE[1], 0.0])


PUNCH_STEPS = PUNCH_DOWN[0] + PUNCH_SIDE[0]


@functools.lru_cache(maxsize=None)
def punch_circle():
    """the body dict of the lifted NURBS circle (never modified) -- its `twin` is the sphere"""
    from oracle import iga
    L = iga.Patch.block(PUNCH_N_EL, 2).ctrl.max(axis=0)
    body = sb.circle(L, "up")
    lift = np.array([0.0, PUNCH_LIFT])
    twin = dict(body["twin"], center=list(np.asarray(body["twin"]["center"]) + lift))
    body = dict(body, control_points=body["control_points"] + lift, twin=twin)
    body["control_points"].setflags(write=False)
    return body


def punch_twin(n_steps):
    """the analytic sphere after the shifts of the first n_steps steps, accumulated as the control points are"""
    c = np.array(punch_circle()["twin"]["center"], dtype=np.float64)
    for k in range(n_steps):
        c = c + punch_shift(k)
    return dict(kind="sphere", center=list(c), radius=punch_circle()["twin"]["radius"])


@functools.lru_cache(maxsize=None)
def implicit_run(name, with_d=True):
    """the scenario solved by the restatement alone: per step Newton's info, the evaluation log and the committed state"""
    S = implicit_system(name)
    x, v = S.x0.copy(), np.zeros_like(S.x0)
    steps, t = [], 0.0
    for k in range(SLIDE_STEPS if name == "slide" else PUNCH_STEPS):
        if name == "slide":
            vx, vy = slide_drive(k)
            S.ode.vbar[:] = np.where(S.cv % 2 == 0, vx, vy)
        else:
            S.contact.body = punch_twin(k + 1)
            S.contact.d = punch_shift(k) if with_d else None
        first = len(S.contact.log)
        t = S.ode.step(x, v, t, DT)
        steps.append(types.SimpleNamespace(info=S.ode.history[-1], log=S.contact.log[first:], x=x.copy(),
                                           n_stick=S.contact.n_stick, n_slip=S.contact.n_slip, state=S.contact.state))
    return types.SimpleNamespace(steps=steps, contact=S.contact, x=x, v=v)


# ---- the explicit short run -------------------------------------------------------------------------------------------------
def short_start(P):
    """(x0, v0) of "e_short": the top pressed 2 E_GAP into the plane of ec.e_plane (linear in height, the bottom at rest),
    a tangential velocity growing with the height and a tilt that pulls the side x = max away from the plane"""
    z = P.ctrl[:, 2] / P.ctrl[:, 2].max()
    x0, v0 = np.zeros((P.n_nodes, 3)), np.zeros((P.n_nodes, 3))
    x0[:, 2] = 3.0 * ec.E_GAP * z
    v0[:, 0], v0[:, 1] = SHORT_V[0] * z, SHORT_V[1] * z
    v0[:, 2] = SHORT_V[2] * z * (1.0 - 2.0 * P.ctrl[:, 0] / P.ctrl[:, 0].max())
    return x0.reshape(-1), v0.reshape(-1)


def short_run(mu=MU, perturb=False):
    from oracle import ref_path as rp
    P = ec.oracle_patch(ec.E_CASE)
    D = rp.DomainOracle(P, ec.material_pair("neohook")[0])
    D.set_dt(ec.E_DT)
    contact = RoughContact(P, P.dim - 1, 1, ec.e_plane(P), ec.E_PENALTY, mu, ec.E_PENALTY)
    rng = np.random.default_rng(77)

    def force(x):
        r = np.zeros(P.n_vdofs)
        D.add_domain_residual(x, r)
        if perturb:
            r = r + ec._residual_perturbation(P, D, "neohook", r, x, rng)
        rc = np.zeros(P.n_vdofs)
        contact.add_boundary_residual(x, rc)
        if perturb:
            rc = rc + fc.TOL["contact_r"] * np.abs(rc).max() * rng.choice([-1.0, 1.0], rc.size)
        return r + rc

    def commit(x):
        D.domain_post_time_advance(x)
        contact.post_time_advance(x)

    x0, v0 = short_start(P)
    s = er.Stepper(ec.lumped_mass(P, D), ec.clamped_bottom(P)).start(x0, v0, None, force, commit=commit)
    samples, shots = [], []
    for k in range(1, SHORT_STEPS + 1):
        s.step(ec.E_DT)
        samples.append((contact.n_stick, contact.n_slip, contact.log[-1]["kink"]))
        if k in SHORT_SHOTS:
            shots.append(types.SimpleNamespace(x=s.x.copy(), v=s.v.copy(), state=contact.state, n_stick=contact.n_stick,
                                               n_slip=contact.n_slip, kink=contact.log[-1]["kink"]))
    return types.SimpleNamespace(shots=shots, contact=contact, samples=samples)


@functools.lru_cache(maxsize=None)
def short_reference():
    """(the run, the frictionless run, per shot the absolute bars of x, v and xi)"""
    base, moved, plain = short_run(), short_run(perturb=True), short_run(mu=0.0)
    spread = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) / ec.MARGIN
    bars = [(spread(a.x, b.x), spread(a.v, b.v), spread(a.state.xi, b.state.xi)) for a, b in zip(base.shots, moved.shots)]
    return base, plain, bars
