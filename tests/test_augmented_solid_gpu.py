"""The facade's augmented-Lagrangian contact (rc.set_int("contact_augmented_lagrange", 1), "contact_augmentations",
update_contact_lagrange / fill_contact_lagrange) against the float64 restatement of tests/_augmented_stepping.py: the beam of
tests/test_boundary_action_gpu._beam, the rigid plane 0.02 heights below it, four steps, eight augmentations per step.

Route: matrix_free + matrix_free_boundary + contact_consistent_tangent (GMRES with the Kronecker preconditioner), penalty
PENALTY = 1e4 -- the device GMRES and Newton converge there in every solve of this scenario (the existing facade test at that
penalty, whose plane starts inside the beam, asserts nothing but finite values).
(1) every Newton and GMRES solve converges; x after each step is np.allclose to the restatement's; the violation sequences
    agree within 10 x _augmented_cases.VIOLATION_DEVIATION; every step that starts with a positive violation ends at no more
    than the restatement's bar (1/100) of it; a penalty-only run of the same flags keeps a penetration of the order of the
    first violation;
(2) fixed_point_solve2 / update_contact_lagrange / advance_time2 by hand give the bytes of the automatic step_time2;
(3) the assembled direct route at penalty 1e2 with two augmentations converges and lowers the violation (no ratio asserted:
    at a penalty far below the beam's stiffness the loop contracts by a few per cent per update);
(4) the refusals of the facade.

Measured on an MI355X (5 tests, 4 s): (1) Newton 2 to 4 iterations per solve, every GMRES solve converged; the impact step's
violations 3.248e-3 4.866e-4 1.065e-4 4.178e-5 2.446e-5 1.657e-5 1.170e-5 8.366e-6 6.003e-6 (ratio 1.85e-3, bar 1e-2), the
restatement's to 3.7e-11 of the first; the fourth step 3.944e-3 then 0 (the beam rebounds and every node releases); penalty
alone keeps 3.124e-3; (3) 2.332e-2 2.172e-2 2.023e-2 and 4.191e-2 3.903e-2 3.635e-2."""
import functools
import types

import numpy as np
import pytest

import _augmented_cases as ac
import _augmented_stepping as st

pytestmark = pytest.mark.gpu
PENALTY = 1.0e4
CONSISTENT = [("contact_consistent_tangent", 1)]
AUGMENTED = [("contact_augmented_lagrange", 1)]


def build(flags, penalty, augmentations=0):
    from mimi_amd.integrators import RigidPlane
    from test_boundary_action_gpu import _beam

    def mark(nl):
        x = nl.patch().control_points
        y0, height = x[:, 1].min(), x[:, 1].max() - x[:, 1].min()
        lower = [a - 1 for a, f in nl._faces.items() if f == (1, 0)][0]
        nl.boundary_condition.current.contact(lower, RigidPlane([0.0, y0 - st.PLANE_BELOW * height], [0.0, 1.0], penalty))

    nl = _beam(flags + ([("contact_augmentations", augmentations)] if augmentations else []), mark)
    if nl.use_iterative_solver_:
        mult = nl.linear_.Mult

        def checked(A, *args):
            out = mult(A, *args)
            assert nl.linear_.converged_, "a GMRES solve did not converge"
            return out
        nl.linear_.Mult = checked
    return nl


def matrix_free():
    from test_boundary_action_gpu import MATRIX_FREE
    return list(MATRIX_FREE)


@functools.lru_cache(maxsize=None)
def automatic_run():
    nl = build(matrix_free() + CONSISTENT + AUGMENTED, PENALTY, st.AUGMENTATIONS)
    assert nl.route_.augmented_contact and nl.contacts_[0].augmented_ and nl.contacts_[0].consistent_tangent_
    u = nl.solution_view("displacement", "x").ravel()
    steps = []
    for _ in range(st.STEPS):
        first = len(nl.newton_history)
        nl.step_time2()
        loop = nl.augmentation_loops[-1]
        steps.append(types.SimpleNamespace(x=u.copy(), newton=nl.newton_history[first:], violations=list(loop["violations"]),
                                           loop=loop, lam=nl.contacts_[0].Lagrange()))
    assert nl.contacts_[0].HoldsAugmentedRecord() and nl.contacts_[0].HoldsConsistentRecord()
    return steps


def test_automatic_loop_against_the_restatement():
    ref = st.run(PENALTY)
    steps = automatic_run()
    deviation = 0.0
    for k, (s, r) in enumerate(zip(steps, ref.steps)):
        print(f"figures augmented facade step {k + 1}: Newton iterations {[h['iterations'] for h in s.newton]}, violations "
              + " ".join(f"{v:.3e}" for v in s.violations))
        assert all(h["converged"] for h in s.newton), (k, s.newton)
        assert len(s.newton) == len(r.newton) and len(s.violations) == len(r.violations)
        assert np.allclose(s.x, r.x)
        assert np.allclose(s.lam, r.lam, rtol=1e-5, atol=1e-8 * PENALTY)
        assert (s.violations[0] > 0) == (r.violations[0] > 0)
        if r.violations[0] > 0:
            deviation = max(deviation, max(abs(a - b) for a, b in zip(s.violations, r.violations)) / r.violations[0])
            assert s.violations[-1] <= st.RATIO_BAR[PENALTY] * s.violations[0]
        assert s.loop["augmentations"] == len(s.violations) - 1 and s.loop["converged"] == (s.violations[-1] <= 0.0)
    print(f"figures augmented facade: violation sequences deviate {deviation:.2e} of the step's first violation "
          f"(recorded {ac.VIOLATION_DEVIATION})")
    assert steps[st.IMPACT_STEP].violations[0] > 0 and len(steps[st.IMPACT_STEP].violations) == st.AUGMENTATIONS + 1
    assert deviation <= 10 * ac.VIOLATION_DEVIATION


def test_penalty_only_keeps_the_violation():
    """the same flags without the mode: after the impact step the beam sits in the plane by about the first violation of
    the augmented run, which that run has brought below 1/100 of it"""
    steps = automatic_run()
    nl = build(matrix_free() + CONSISTENT, PENALTY)
    assert not nl.route_.augmented_contact
    with pytest.raises(RuntimeError, match="contact_augmented_lagrange"):
        nl.update_contact_lagrange()
    for _ in range(st.IMPACT_STEP + 1):
        nl.step_time2()
        assert nl.newton_history[-1]["converged"]
    c = nl.contacts_[0]
    c.BoundaryPostTimeAdvance(nl.x)
    kept = float(np.abs(c.AveragePressure()).max()) / PENALTY
    first, last = steps[st.IMPACT_STEP].violations[0], steps[st.IMPACT_STEP].violations[-1]
    print(f"figures augmented facade: penalty-only penetration {kept:.3e}, augmented {first:.3e} -> {last:.3e}")
    assert kept >= 0.5 * first and last <= st.RATIO_BAR[PENALTY] * kept


def test_hand_written_loop_gives_the_bytes_of_the_automatic_one():
    steps = automatic_run()
    nl = build(matrix_free() + CONSISTENT + AUGMENTED, PENALTY)
    u = nl.solution_view("displacement", "x").ravel()
    for s in steps:
        nl.fixed_point_solve2()
        applied = 0
        while True:
            violation = nl.update_contact_lagrange(apply=False)
            if violation <= 0.0 or applied >= st.AUGMENTATIONS:
                break
            assert nl.update_contact_lagrange() == violation
            applied += 1
            nl.fixed_point_solve2()
        nl.advance_time2()
        assert u.tobytes() == s.x.tobytes() and nl.contacts_[0].Lagrange().tobytes() == s.lam.tobytes()
        assert applied == s.loop["augmentations"]
    assert not nl.augmentation_loops and len(nl.augmentation_history) > st.AUGMENTATIONS
    nl.fill_contact_lagrange()
    assert not np.any(nl.contacts_[0].Lagrange())


def test_assembled_route_at_a_soft_penalty():
    nl = build(AUGMENTED, 1.0e2, 2)
    assert not nl.use_iterative_solver_ and nl.contacts_[0].augmented_
    lowered = 0
    for k in range(st.STEPS):
        first = len(nl.newton_history)
        nl.step_time2()
        assert all(h["converged"] for h in nl.newton_history[first:]), (k, nl.newton_history[first:])
        v = nl.augmentation_loops[-1]["violations"]
        print(f"figures augmented facade assembled 1e2 step {k + 1}: violations " + " ".join(f"{x:.3e}" for x in v))
        if v[0] > 0:
            assert v[-1] < v[0] and len(v) == 3
            lowered += 1
    assert lowered > 0 and nl.contacts_[0].HoldsTangentBlocks()


def test_facade_refusals():
    from test_nonlinear_solid import beam
    nl = beam("neohook", runtime=[("explicit_dynamics", 1)] + AUGMENTED, finish=False)
    with pytest.raises(RuntimeError, match="contact_augmented_lagrange cannot be combined with explicit_dynamics"):
        nl.setup(1)
    nl = build(AUGMENTED, 1.0e2)
    with pytest.raises(RuntimeError, match="before any solve"):
        nl.update_contact_lagrange()
