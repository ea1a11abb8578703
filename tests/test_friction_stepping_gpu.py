"""The routes around the friction kernels -- step_time2, fixed_point_solve2 + advance_time2, a moving spline punch with
step_displacement, explicit_steps -- against the restatement of tests/_friction_stepping.py (its docstring has the scenarios,
the formula of the lock-step bar and where every bar comes from; tests/test_friction_stepping_cpu.py asserts what the
scenarios are relied on for).

Lock-step, after every step of the product: (1) its alpha-level vectors _xa, _va against the restated predictor applied to the
previous (x, v, a), and x, v, a after the step against the restated extrapolation, to 16 x 2^-53 max|.|; (2) the restated
operator, set to the product's _xa, _va, _fac0, _fac1, at the product's acceleration:
|op.mult(aa)|_2 <= max(1e-10 |op.mult(0)|_2, 1e-9) + slack; (3) the restatement commits at the product's x and the product's
FrictionState is its state: c exact, xi to fx.XI_TOL, xbar to fc.TOL["surface_x"], stick / slip counts exact, the friction
force and sum da |t| to fc.TOL["contact_force"], with the kink and gate margins of that evaluation asserted >= 1e-9.  A
product that commits at the alpha level, inside Newton or its line search, evaluates friction at another level or with
another d, or loses the friction tangent (Newton then misses its goal) fails one of these.

Scales of (3), where tests/test_friction_gpu.py's "relative to the largest reference entry" would be ill-conditioned: xi
relative to max(max|xi|, fs.XI_FLOOR extents) (a step that only presses has slips of 1e-5 .. 1e-4 extents, and the error is
the rounding of the coordinates whatever the slip: relative to the largest entry alone the device, correct to 7.5e-16
absolute, shows 2.7e-12 there); the friction force relative to sum da |t| (while the block only spreads under the press the
tractions cancel in the sum; relative to the force's own largest entry the same device figures read 4.6e-8).  In the first
step the previous acceleration is the restatement's own M^-1 (f - r) at rest, which the device's differs from by its
residual's bar: that step's vectors are held to RESIDUAL_BAR = 1e-12, all later ones to 16 x 2^-53.

Measured on an MI355X (worst over the steps; bars in brackets):
  slide, step_time2:   predictor 3.5e-16 (1.8e-15), first step 2.8e-16 (1e-12), residual 1.8e-10 .. 6.6e-10 against goals of
                       1.0e-09 .. 5.0e-09 + slack 1.3e-11 .. 1.8e-10, xi 7.8e-14 (1e-12), xbar 2.3e-16 (1e-14), force 7.0e-13,
                       sum da |t| 5.0e-13 (1e-11), gate margin 3.1e-4, kink margin 6.8e-2; 16 points rub from the second step on
  slide, fixed point:  the same figures, to the digits shown
  punch:               predictor 2.4e-16, first step 4.3e-14, residual 1.3e-11 .. 1.7e-10 against 1.0e-09 + slack 1.3e-12 ..
                       1.5e-11, xi 7.7e-14, xbar 3.0e-16, force 3.7e-12, sum da |t| 2.6e-12, gate margin 7.8e-4, kink margin
                       5.3e-2; 24 points rub, 20 after the contact patch has crossed into the next element
  translated punch:    sum da |t| 1.0e-14 (bound 5.1e-12), 24 points stick
  e_short:             after 6 steps x 5.0e-17 (bar 1.1e-13) v 7.3e-15 (bar 2.9e-11) xi 5.9e-17 (bar 9.4e-15); after 12 steps
                       x 5.7e-17 (bar 2.9e-13) v 6.3e-15 (bar 2.7e-11) xi 0 (bar 0); friction moves x by 3.7e-4 / 1.2e-3
Mutants (not committed): CommitFriction moved before the step in explicit_steps fails the e_short test (x off by 2.2e-4);
_post_time_advance committing at _xa fails both lock-step tests (xbar off by 4.8e-4 / 2.3e-6)."""
import types

import numpy as np
import pytest

import _explicit_cases as ec
import _face_cases as fc
import _face_reference as fr
import _friction_cases as fx
import _friction_stepping as fs

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    if scale == 0.0:
        return 0.0 if not np.any(a) else np.inf
    return float(np.abs(np.asarray(a) - b).max() / scale)


# ---- the products ------------------------------------------------------------------------------------------------------------
def slide_product():
    import test_friction_solid_gpu as tf
    nl, plane = tf.block(fs.MU, fs.PENALTY)
    nl.solution_view("displacement", "x")[1::2] = -fs.PRESS
    return nl


def slide_before_step(nl, k):
    import test_friction_solid_gpu as tf
    tf.drive(nl, *fs.slide_drive(k))


def punch_product():
    """(facade, scene, spline): the 6 x 3 block under the lifted NURBS circle, handed over as examples/nl_contact.py does"""
    import mimi_amd as mimi
    from mimi_amd.integrators import NearestDistanceToSplines
    B = mimi.BSplinePatch.block(fs.PUNCH_N_EL, 2)
    probe = ec.facade("sq_p2", "neohook", setup=False)
    bottom = [a - 1 for a, f in probe._faces.items() if f == (1, 0)][0]
    top = [a - 1 for a, f in probe._faces.items() if f == (1, 1)][0]
    body = fs.punch_circle()
    spline = types.SimpleNamespace(degrees=body["degrees"], knot_vectors=body["knots"],
                                   control_points=np.array(body["control_points"], dtype=float), weights=body["weights"])
    scene = NearestDistanceToSplines()
    scene.add_spline(spline)
    scene.plant_kd_tree(body["resolution"], 1)
    scene.coefficient = fs.PENALTY
    scene.friction = fs.MU
    scene.tangential_coefficient = fs.PUNCH_EPS_T

    def configure(bc):
        bc.initial.dirichlet(bottom, 0)
        bc.initial.dirichlet(bottom, 1)
        bc.current.contact(top, scene)
    nl = ec.facade("sq_p2", "neohook", flags=(), configure=configure, setup=False)
    nl.patch = lambda: B
    nl.time_step_size = fs.DT
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", fs.NEWTON["rel_tol"], fs.NEWTON["abs_tol"], fs.NEWTON["max_iter"], False)
    return nl, scene, spline


def move_punch(scene, spline, shift, with_d=True):
    spline.control_points += shift
    scene.plant_kd_tree(fs.punch_circle()["resolution"], 1)
    if with_d:
        scene.step_displacement = shift


# ---- the lock-step ------------------------------------------------------------------------------------------------------------
class LockStep:
    """the restated system of a scenario beside a product: before(), the product's step, after()"""

    def __init__(self, name, nl, contact_bar):
        from oracle import iga
        B = nl.patch()
        self.S = S = fs.implicit_system(name, iga.Patch(list(B.degrees), [np.asarray(k, dtype=np.float64) for k in B.knots],
                                                        np.asarray(B.control_points, dtype=np.float64)))
        self.nl, self.contact_bar = nl, contact_bar
        block = fs.implicit_system(name).P
        assert np.array_equal(S.P.ctrl, block.ctrl) and all(np.allclose(a, b, rtol=0, atol=1e-15) for a, b in zip(S.P.knots, block.knots))
        assert np.array_equal(np.sort(nl.dirichlet_), S.dirichlet) and np.array_equal(np.sort(nl.constant_velocity_dofs_), S.cv)
        assert np.array_equal(nl.x, S.x0)
        S.op.dt = fs.DT
        self.worst = dict(predictor=0.0, first_step=0.0, traction=0.0, residual=0.0, goal_lo=np.inf, goal_hi=0.0, slack=0.0, xi=0.0, xbar=0.0, force=0.0,
                          gate=np.inf, kink=np.inf)
        self.rubbed, self.first = [], True

    def before(self):
        nl, S = self.nl, self.S
        self.prev = (nl.x.copy(), nl.x_dot.copy(), nl._a.cpu().numpy() if nl._nstate else S.op.explicit_accel(nl.x.copy()))
        self.vbar = nl.constant_velocity_values_[np.argsort(nl.constant_velocity_dofs_)].copy()

    def after(self):
        nl, S, w = self.nl, self.S, self.worst
        ode, op, C = S.ode, S.op, S.contact
        x0, v0, a0 = self.prev
        n = len(x0)
        xa, va, aa = (t.cpu().numpy() for t in (nl._xa, nl._va, nl._aa))
        # 1: the predictor and the extrapolation
        xa_r, va_r, saved = fs.predictor(ode, x0, v0, a0, fs.DT, S.cv, self.vbar)
        prev = 1.0 - 1.0 / ode.fac1
        x_r = x0 * prev + (xa_r + nl._fac0 * aa) / ode.fac1
        v_r = v0 * prev + (va_r + nl._fac1 * aa) / ode.fac1
        a_r = a0 * prev + aa / ode.fac5
        x_r[S.cv], v_r[S.cv], a_r[S.cv] = saved, self.vbar, 0.0
        assert nl._fac0 == ode.fac3 * fs.DT * fs.DT and nl._fac1 == ode.fac4 * fs.DT
        # (in the first step the previous a is not the product's but the restatement's own M^-1 (f - r) at rest, which the
        # device's differs from by its residual's bar, not by rounding; from x = v = 0 the alpha levels are that a alone)
        bar, key = (fs.RESIDUAL_BAR, "first_step") if self.first else (fs.PREDICTOR_BAR, "predictor")
        self.first = False
        for got, want in ((xa, xa_r), (va, va_r), (nl.x, x_r), (nl.x_dot, v_r), (nl._a.cpu().numpy(), a_r)):
            scale = max(np.abs(want).max(), np.abs(got).max())
            err = np.abs(got - want).max() / scale if scale > 0 else 0.0
            w[key] = max(w[key], err)
            assert err <= bar, (key, err)
        # 2: the product's acceleration solves the restated step
        op.set_parameters(nl._fac0, nl._fac1, xa, va)
        start = np.linalg.norm(op.mult(np.zeros(n)))
        r = op.mult(aa)
        inertia = op._csr(op.mass) @ aa
        domain = np.zeros(n)
        S.D.add_domain_residual(xa + nl._fac0 * aa, domain)
        slack = np.sqrt(n) * (fs.RESIDUAL_BAR * (np.abs(inertia).max() + np.abs(domain).max())
                              + self.contact_bar * np.abs(C.r_contact).max() + fc.TOL["contact_r"] * np.abs(C.r_friction).max())
        goal = max(fs.NEWTON["rel_tol"] * start, fs.NEWTON["abs_tol"])
        norm = float(np.linalg.norm(r))
        w["residual"], w["slack"] = max(w["residual"], norm), max(w["slack"], slack)
        w["goal_lo"], w["goal_hi"] = min(w["goal_lo"], goal), max(w["goal_hi"], goal)
        assert nl.newton_history[-1]["converged"]
        assert norm <= goal + slack, (norm, goal, slack)
        # 3: the commit at the end-of-step displacement
        op.post_time_advance(nl.x)
        entry = C.log[-1]
        w["gate"], w["kink"] = min(w["gate"], entry["gate"]), min(w["kink"], entry["kink"])
        assert entry["gate"] >= fs.MARGIN_MIN and entry["kink"] >= fs.MARGIN_MIN
        G = nl.contacts_[0]
        xi, xbar, c = G.FrictionState()
        dim = S.P.dim
        perm, _ = fr.match_points(C.state.xbar, xbar.reshape(-1, dim))
        assert np.array_equal(c.reshape(-1)[perm].astype(bool), C.state.c)
        xi_scale = max(float(np.abs(C.state.xi).max()), fs.XI_FLOOR * C.extent)
        xi_err = float(np.abs(xi.reshape(-1, dim)[perm] - C.state.xi.astype(np.float64)).max()) / xi_scale
        w["xi"] = max(w["xi"], xi_err)
        w["xbar"] = max(w["xbar"], rel(xbar.reshape(-1, dim)[perm], C.state.xbar))
        assert (G.n_stick_, G.n_slip_) == (C.n_stick, C.n_slip)
        # (the force is a sum of da t whose terms cancel while the block only presses and spreads: held relative to sum da |t|)
        if C.friction_traction > 0.0:
            w["force"] = max(w["force"], float(np.abs(G.last_friction_force_ - C.friction_force).max()) / C.friction_traction)
            w["traction"] = max(w["traction"], abs(G.last_friction_traction_ - C.friction_traction) / C.friction_traction)
        else:
            assert not np.any(G.last_friction_force_) and G.last_friction_traction_ == 0.0
        self.rubbed.append(C.n_stick + C.n_slip)
        print(f"   step {len(self.rubbed) - 1}: residual {norm:.2e} goal {goal:.2e} slack {slack:.2e} stick {C.n_stick} slip {C.n_slip} "
              f"xi {xi_err:.2e} of {xi_scale:.2e} (largest entry {float(np.abs(C.state.xi).max()):.2e}) gate {entry['gate']:.2e} "
              f"kink {entry['kink']:.2e}")
        assert w["xi"] <= fx.XI_TOL and w["xbar"] <= fc.TOL["surface_x"] and w["force"] <= fc.TOL["contact_force"]
        assert w["traction"] <= fc.TOL["contact_force"]

    def report(self, what):
        print(f"figures friction stepping {what}: " + " ".join(f"{k}={v:.2e}" for k, v in self.worst.items()) + f" rubbing points {self.rubbed}")


# ---- 2. the implicit route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["step_time2", "fixed_point"])
def test_implicit_route_in_lock_step(route):
    """step_time2 on every step; "fixed_point": the last two sideways steps by fixed_point_solve2 x 2 + advance_time2"""
    nl = slide_product()
    lock = LockStep("slide", nl, fc.TOL["contact_r"])
    for k in range(fs.SLIDE_STEPS):
        slide_before_step(nl, k)
        lock.before()
        if route == "fixed_point" and k >= fs.SLIDE_STEPS - 2:
            nl.fixed_point_solve2()
            nl.fixed_point_solve2()
            nl.advance_time2()
        else:
            nl.step_time2()
        lock.after()
    lock.report(f"slide {route}")
    assert sum(lock.rubbed) > 0


# ---- 3. the moving spline punch ---------------------------------------------------------------------------------------------------
def state_bytes(nl):
    return tuple(a.tobytes() for a in nl.contacts_[0].FrictionState())


def test_moving_spline_punch_in_lock_step():
    nl, scene, spline = punch_product()
    lock = LockStep("punch", nl, fs.PUNCH_TWIN_BAR)
    other, other_scene, other_spline = punch_product()               # the same, step_displacement left at None
    for k in range(fs.PUNCH_STEPS):
        shift = fs.punch_shift(k)
        move_punch(scene, spline, shift)
        lock.S.contact.body, lock.S.contact.d = fs.punch_twin(k + 1), shift
        lock.before()
        nl.step_time2()
        lock.after()
        move_punch(other_scene, other_spline, shift, with_d=False)
        other.step_time2()
        if k == 0:
            assert state_bytes(other) == state_bytes(nl)             # contact is new in this step: d is not read yet
    lock.report("punch")
    assert sum(lock.rubbed[fs.PUNCH_DOWN[0]:]) > 0                   # friction acted in the slide phase
    assert other_scene.step_displacement is None and state_bytes(other) != state_bytes(nl)
    assert np.abs(other.x - nl.x).max() > 1e-6 * np.abs(nl.x).max()


def test_block_translated_with_the_punch_has_no_traction():
    """the closed form of test_closed_forms_on_a_flat_face through the facade: after the step in which contact is new (xi = 0,
    c = 1 committed at x), the block -- every node, through the solution view -- and the punch are translated by the same
    vector, step_displacement says so, and a step of 1e-9 time units (the block's own motion over it, a dt^2 of 1e-18, is
    far below the rounding of the coordinates) evaluates and commits there: x_q - xbar - d cancels to the rounding of the
    coordinates, a few units of it, times eps_T, over the area -- the bound of that test"""
    nl, scene, spline = punch_product()
    move_punch(scene, spline, fs.punch_shift(0))
    nl.step_time2()
    G = nl.contacts_[0]
    xi, _, c = G.FrictionState()
    assert c.all() and not np.any(xi) and abs(G.last_pressure_) > 0.0
    shift = np.array([0.037, 0.011])
    x = nl.solution_view("displacement", "x")
    x[:] = (x.reshape(-1, 2) + shift).reshape(-1)
    nl.solution_view("displacement", "x_dot")[:] = 0.0
    move_punch(scene, spline, shift)
    nl.time_step_size = 1e-9
    nl.step_time2()
    assert nl.newton_history[-1]["converged"]
    B = nl.patch()
    area = float(fr.face_points(fr.face_basis(B.degrees, B.knots, 1, 1), B.control_points).da.sum())
    bound = 64 * EPS * float(np.abs(B.control_points).max()) * fs.PUNCH_EPS_T * area
    print(f"figures friction stepping punch translated: sum da |t| {G.last_friction_traction_:.2e} bound {bound:.2e} "
          f"pressure {G.last_pressure_:.3e} stick {G.n_stick_} slip {G.n_slip_}")
    assert abs(G.last_pressure_) > 0.0 and G.n_stick_ + G.n_slip_ == c.size
    assert G.last_friction_traction_ <= bound
    # the same step without step_displacement rubs
    scene.step_displacement = None
    x[:] = (x.reshape(-1, 2) + shift).reshape(-1)
    spline.control_points += shift
    scene.plant_kd_tree(fs.punch_circle()["resolution"], 1)
    nl.step_time2()
    assert G.last_friction_traction_ > 1e6 * bound


# ---- 4b. the explicit route, twelve steps -------------------------------------------------------------------------------------------
def test_explicit_short_run_against_the_restatement():
    import test_friction_solid_gpu as tf
    base, plain, bars = fs.short_reference()
    nl = tf.rough(fs.MU)
    x0, v0 = fs.short_start(ec.oracle_patch(ec.E_CASE))
    nl.solution_view("displacement", "x")[:] = x0
    nl.solution_view("displacement", "x_dot")[:] = v0
    G = nl.contacts_[0]
    done = 0
    for at, shot, other, (bx, bv, bxi) in zip(fs.SHORT_SHOTS, base.shots, plain.shots, bars):
        nl.explicit_steps(at - done)
        done = at
        xi, xbar, c = G.FrictionState()
        perm, _ = fr.match_points(shot.state.xbar, xbar.reshape(-1, 3))
        ex, ev = np.abs(nl.x - shot.x).max(), np.abs(nl.x_dot - shot.v).max()
        exi = np.abs(xi.reshape(-1, 3)[perm] - shot.state.xi.astype(np.float64)).max()
        effect = np.abs(shot.x - other.x).max()
        print(f"figures friction stepping e_short after {at} steps: x {ex:.2e} (bar {bx:.2e}) v {ev:.2e} (bar {bv:.2e}) xi {exi:.2e} "
              f"(bar {bxi:.2e}); friction moves x by {effect:.2e}; stick {G.n_stick_} slip {G.n_slip_}")
        assert effect > 100 * bx
        assert ex <= bx and ev <= bv and exi <= bxi
        assert np.array_equal(c.reshape(-1)[perm].astype(bool), shot.state.c)
        assert (G.n_stick_, G.n_slip_) == (shot.n_stick, shot.n_slip) and shot.kink >= fs.MARGIN_MIN
