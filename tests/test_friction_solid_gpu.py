"""Friction through NonlinearSolid: a 2-D block of 4 x 2 elements (degree 2) on a RigidPlane(friction=0.3), its top edge
driven down and then sideways by constant_velocity (implicit route), and the contact run of tests/test_explicit_gpu.py
with friction on the plane (explicit route).  The state is committed by _post_time_advance on step_time2 / advance_time2,
never by fixed_point_solve2, and by the null form of the commit inside explicit_steps.  The explicit run is held to the float64
restatement of tests/_explicit_cases.py (run "friction": domain + RoughContact of tests/_friction_stepping.py, committed after
every step).  Measured on an MI355X: KE, W_int at the end equal to the restatement's in all 13 digits printed (bar 1e-6 of
the scale 5.96), the stick / slip counts at the ten samples the restatement's, (4, 60) ... (12, 52) ... (0, 0)."""
import numpy as np
import pytest

import _explicit_cases as ec

pytestmark = pytest.mark.gpu
MU, PENALTY = 0.3, 1.0e2       # (the frozen-pressure tangent makes Newton a fixed-point iteration in the pressure: it
#                                contracts while the penalty is small beside the block's stiffness, E / height = 1050)
DOWN, SIDE = (3, 0.01), (6, 0.004)      # (steps, travel per step) of the two phases
DT = 0.05


def block(friction=None, penalty=PENALTY):
    """the facade of the block: bottom edge on the plane y = 0, top edge prescribed in both components"""
    import mimi_amd as mimi
    from mimi_amd.integrators import RigidPlane
    B = mimi.BSplinePatch.block((4, 2), 2, lengths=(4.0, 2.0))
    probe = ec.facade("sq_p2", "neohook", setup=False)
    bottom = [a - 1 for a, f in probe._faces.items() if f == (1, 0)][0]
    top = [a - 1 for a, f in probe._faces.items() if f == (1, 1)][0]
    kw = {} if friction is None else dict(friction=friction)
    plane = RigidPlane([0.0, 0.0], [0.0, 1.0], penalty, **kw)

    def configure(bc):
        bc.initial.constant_velocity(top, 0, 0.0)
        bc.initial.constant_velocity(top, 1, -DOWN[1] / DT)
        bc.current.contact(bottom, plane)
    nl = ec.facade("sq_p2", "neohook", flags=(), configure=configure, setup=False)
    nl.patch = lambda: B
    nl.time_step_size = DT
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-10, 1e-9, 40, False)
    return nl, plane


def drive(nl, vx, vy):
    """the prescribed velocity of the top edge from the next step on"""
    import torch
    comp = nl.constant_velocity_dofs_ % 2
    nl.constant_velocity_values_[:] = np.where(comp == 0, vx, vy)
    nl.d_cv_values_.copy_(torch.from_numpy(nl.constant_velocity_values_))


def slide(nl, plane, log=None):
    c = nl.contacts_[0]
    for phase, (steps, travel) in enumerate((DOWN, SIDE)):
        if phase == 1:
            drive(nl, travel / DT, 0.0)
        for _ in range(steps):
            nl.step_time2()
            h = nl.newton_history[-1]
            if log is not None:
                log.append((phase, h, c.last_pressure_, c.last_friction_traction_, c.last_friction_force_.copy(), c.n_stick_, c.n_slip_))
    return nl.x.copy()


def test_implicit_slide():
    nl, plane = block(MU)
    log = []
    slide(nl, plane, log)
    slipped = 0
    for phase, h, pressure, traction, force, n_stick, n_slip in log:
        print(f"phase {phase}: Newton {h['converged']} in {h['iterations']}, |r| {h['norm']:.2e} of {h['norm0']:.2e}; pressure "
              f"{pressure:.6e} sum da|t| {traction:.6e} force {force} stick {n_stick} slip {n_slip}")
        assert h["converged"]
        assert traction <= MU * abs(pressure) * (1 + 1e-12)
        if phase == 1:
            assert n_stick + n_slip > 0 and force[0] > 0.0        # the block slides towards +x: the force on it opposes that
        if phase == 1 and n_stick == 0 and n_slip > 0:
            slipped += 1
            assert abs(traction - MU * abs(pressure)) <= 1e-10 * MU * abs(pressure)
    assert abs(log[DOWN[0] - 1][2]) > 0.0                         # the plane was reached before the slide began
    assert slipped > 0                                            # full slip was reached


def test_zero_friction_is_a_body_without_the_attribute():
    runs = []
    for friction in (None, 0.0):
        nl, plane = block(friction)
        runs.append(slide(nl, plane))
        assert nl.contacts_[0].friction_ == 0.0
    assert np.abs(runs[0]).max() > 0 and runs[0].tobytes() == runs[1].tobytes()


def test_fixed_point_solve_leaves_the_friction_state_alone():
    a, plane_a = block(MU)
    b, plane_b = block(MU)
    for _ in range(DOWN[0]):
        a.step_time2()
        b.step_time2()
    for nl in (a, b):
        drive(nl, SIDE[1] / DT, 0.0)
    a.step_time2()
    b.step_time2()
    state = lambda nl: tuple(s.tobytes() for s in nl.contacts_[0].FrictionState())
    before = state(a)
    assert before == state(b)
    a.fixed_point_solve2()
    first = a._aa.cpu().numpy().tobytes()
    assert state(a) == before
    a.fixed_point_solve2()
    assert a._aa.cpu().numpy().tobytes() == first and state(a) == before
    a.advance_time2()
    b.step_time2()
    assert state(a) != before
    assert a.x.tobytes() == b.x.tobytes() and state(a) == state(b)


def rough(mu):
    def configure(bc):
        from mimi_amd.integrators import RigidPlane
        for c in range(3):
            bc.initial.dirichlet(0, c)
        p = ec.e_plane(ec.oracle_patch(ec.E_CASE))
        bc.current.contact(1, RigidPlane(p["point"], p["normal"], ec.E_PENALTY, **({} if mu is None else dict(friction=mu))))
    nl = ec.facade(ec.E_CASE, "neohook", configure=configure)
    nl.time_step_size = ec.E_DT
    nl.solution_view("displacement", "x_dot")[:] = ec.e_initial_velocity(ec.oracle_patch(ec.E_CASE), "contact")
    return nl


def test_explicit_route():
    """E* is conserved by the scheme whatever the force law: the bar is the one tests/test_explicit_gpu.py holds its
    contact run to, 8 x the drift of the float64 restatement of that run"""
    bar = 8.0 * ec.e_reference("contact").drift
    ref = ec.e_reference("friction")
    nl = rough(MU)
    c = nl.contacts_[0]
    series, rubbed, touched, counts = [nl.explicit_energies()], 0, False, []
    for _ in range(ec.E_STEPS // ec.E_EVERY):
        nl.explicit_steps(ec.E_EVERY)
        series.append(nl.explicit_energies())
        rubbed += c.n_stick_ + c.n_slip_
        counts.append((c.n_stick_, c.n_slip_))
        touched = touched or np.abs(c.last_force_).max() > 0.0
    star = np.array([e["E_star"] for e in series])
    drift = np.abs(star - star[0]).max()
    print(f"explicit with friction: E* drift {drift:.2e} (bar {bar:.2e}); points with a traction at the samples: {rubbed}")
    assert touched and rubbed > 0                                 # the plane was reached, and it rubbed
    assert drift <= bar
    # the run is the one the restatement made (E* holds whatever the force law; the works and the branches do not): the
    # line tests/test_explicit_gpu.py has for its contact run, against domain + RoughContact committed after every step,
    # and the restatement's stick / slip counts at the sampled steps (their kink margins: tests/test_friction_stepping_cpu.py)
    last = series[-1]
    print("   at the end: " + " ".join(f"{k} {last[k]:.12e} (restated {float(ref.last[k]):.12e})" for k in ("KE", "W_int", "W_ext"))
          + f"; scale {ref.scale:.3e}; stick / slip at the samples {counts}")
    for k in ("KE", "W_int", "W_ext"):
        assert abs(last[k] - float(ref.last[k])) <= 1e-6 * ref.scale, k
    assert all(kink >= 1e-9 for _, _, kink in ref.counts)
    assert counts == [(a, b) for a, b, _ in ref.counts]
    # the same run without friction copies as often to the host, and differs
    plain = rough(None)
    plain.explicit_steps(ec.E_STEPS)
    assert plain.explicit_d2h_copies_ > 0
    again = rough(MU)
    again.explicit_steps(ec.E_STEPS)
    assert again.explicit_d2h_copies_ == plain.explicit_d2h_copies_
    assert again.x.tobytes() != plain.x.tobytes()
    # n steps and n more are 2 n steps
    assert again.x.tobytes() == nl.x.tobytes() and again.x_dot.tobytes() == nl.x_dot.tobytes()
    assert tuple(s.tobytes() for s in again.contacts_[0].FrictionState()) == tuple(s.tobytes() for s in c.FrictionState())
