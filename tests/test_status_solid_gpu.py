"""The facade's share of the status word (tests/test_status_gpu.py has the integrator's): mimi_amd.NonlinearSolid hands its
integrators device tensors, so their calls only enqueue and a failed return map waits in the handle's status word until
somebody reads it.  The reference throws out of StepTime2; so must the facade, and before it commits.

The solid: sq_p2 of tests/_explicit_cases.py (square-nurbs.mesh, degree 2, 2 x 2 elements, the bottom clamped, tensor_small) with
the small-strain J2 law under the softening Voce law of tests/_status_cases.py, where every yielding point fails, and under
the hardening Voce law as the control.  Implicit routes: a body force (BODY_FORCE along x, one step of STEP) from rest, so the
evaluation at the start is quiet and points yield inside the first Newton solve -- on the CPU the oracle's own
GeneralizedAlpha2 step throws under the softening law and leaves 22 % of the points plastic (eqps up to 0.011) under the control
(tests/test_status_cases_cpu.py::test_the_oracle_step_throws).  Explicit route: a sheared start displacement (the failure is
in the start evaluation: raised by explicit_restart before a step is taken), and a shear velocity from rest (the failure
comes inside the step loop, which by design reads the words once per explicit_steps call: raised at the end of the call).

Asserted: step_time2() raises RuntimeError "root not bracketed" on the direct-solve, the iterative and the matrix_free +
matrix_free_jacobi routes, fixed_point_solve2() the same, explicit_steps(n) the same; the step raises before it commits --
the committed accumulated plastic strain, current_time and the host displacement are those from before the step (for the
failure inside the explicit loop: the state only; the time has moved on by the n steps of the call, see above); the words
are clean afterwards; the control steps without error on every route and yields."""
import numpy as np
import pytest

import _explicit_cases as ec
import _status_cases as sc

pytestmark = pytest.mark.gpu

CASE, BODY_FORCE, STEP = sc.SOLID_CASE, sc.SOLID_BODY_FORCE, sc.SOLID_STEP
SHEAR = 0.15                                      # start displacement gamma Y e_x: trial q = sqrt(3) G gamma = 3 x the yield stress
SHEAR_RATE, EXPLICIT_STEPS = 100.0, 20            # start velocity V Y e_x: gamma = V n dt = 0.2 after the call's 20 steps of 1e-4
ROUTES = {"direct": (), "iterative": (("use_iterative_solver", 1),),
          "matrix_free_jacobi": (("use_iterative_solver", 1), ("matrix_free", 1), ("matrix_free_jacobi", 1))}
EXPLICIT = (("explicit_dynamics", 1),)


def solid(law, flags, body_force=True):
    def configure(bc):
        for c in range(2):
            bc.initial.dirichlet(0, c)
        if body_force:
            bc.initial.body_force(0, BODY_FORCE)

    nl = ec.facade(CASE, "j2", flags=flags, configure=configure, material=sc.product_material("j2", law))
    assert nl.domain_.path_ == 1
    if flags != EXPLICIT:
        nl.configure_newton("nonlinear_solid", 1e-12, 1e-8, 10, False)
        nl.time_step_size = STEP
    return nl


def snapshot(nl):
    return nl.domain_.State("accumulated_plastic_strain").copy(), nl.current_time, nl.x.copy(), nl.x_dot.copy()


def unchanged(nl, before, time=True):
    eqps, t, x, v = before
    assert np.array_equal(nl.domain_.State("accumulated_plastic_strain"), eqps)
    if time:
        assert nl.current_time == t and np.array_equal(nl.x, x) and np.array_equal(nl.x_dot, v)
    for integ in nl.integrators_:                 # reported once: the words are clean
        integ.Synchronize()


def sheared(nl, gamma):
    ref = nl.solution_view("displacement", "x_ref").reshape(-1, 2)
    u = np.zeros_like(ref)
    u[:, 0] = gamma * ref[:, 1]
    return u.ravel()


@pytest.mark.parametrize("route", ROUTES)
def test_step_time2_raises_before_it_commits(route):
    nl = solid(sc.MAIN_LAW, ROUTES[route])
    assert (nl.use_iterative_solver_, nl.matrix_free_) == (route != "direct", route == "matrix_free_jacobi")
    before = snapshot(nl)
    with pytest.raises(RuntimeError, match=sc.MESSAGE):
        nl.step_time2()
    assert nl.domain_.LastKernelFamily() == "tensor_small"
    unchanged(nl, before)


def test_fixed_point_solve2_raises_before_it_commits():
    nl = solid(sc.MAIN_LAW, ())
    before = snapshot(nl)
    with pytest.raises(RuntimeError, match=sc.MESSAGE):
        nl.fixed_point_solve2()
    unchanged(nl, before)
    with pytest.raises(RuntimeError, match=sc.MESSAGE):            # the open step is solved again, and fails again
        nl.fixed_point_solve2()
    unchanged(nl, before)


def test_explicit_start_evaluation_raises_before_a_step_is_taken():
    nl = solid(sc.MAIN_LAW, EXPLICIT, body_force=False)
    nl.solution_view("displacement", "x")[:] = sheared(nl, SHEAR)
    before = snapshot(nl)
    with pytest.raises(RuntimeError, match=sc.MESSAGE):
        nl.explicit_steps(EXPLICIT_STEPS)
    unchanged(nl, before)


def test_explicit_steps_raise_at_the_end_of_the_call():
    nl = solid(sc.MAIN_LAW, EXPLICIT, body_force=False)
    nl.solution_view("displacement", "x_dot")[:] = sheared(nl, SHEAR_RATE)
    before = snapshot(nl)
    nl.explicit_restart()                                           # the start is quiet
    with pytest.raises(RuntimeError, match=sc.MESSAGE):
        nl.explicit_steps(EXPLICIT_STEPS)
    # a failed return map takes no plastic step, so the committed state is still the one from before the call; the time is
    # not: the loop commits every step on the device and reads the words once, after the last
    unchanged(nl, before, time=False)
    assert nl.current_time == pytest.approx(EXPLICIT_STEPS * ec.DT)


@pytest.mark.parametrize("route", list(ROUTES) + ["fixed_point", "explicit"])
def test_the_hardening_control_steps_without_error(route):
    if route == "explicit":
        nl = solid(sc.CONTROL_LAW, EXPLICIT, body_force=False)
        nl.solution_view("displacement", "x_dot")[:] = sheared(nl, SHEAR_RATE)
        nl.explicit_steps(EXPLICIT_STEPS)
    elif route == "fixed_point":
        nl = solid(sc.CONTROL_LAW, ())
        nl.fixed_point_solve2()
        nl.advance_time2()
    else:
        nl = solid(sc.CONTROL_LAW, ROUTES[route])
        nl.step_time2()
    assert nl.current_time > 0.0
    eqps = nl.domain_.State("accumulated_plastic_strain")
    assert eqps.max() > 1e-3                       # points yield within the first step
