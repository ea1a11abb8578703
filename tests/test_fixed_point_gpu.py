"""Fixed-point time stepping of the facade (NonlinearSolid.fixed_point_solve2 / fixed_point_advance2 / advance_time2,
restating solvers/ode.cpp:81-186 and py/py_solid.cpp:443-511) and the accessors a partitioned coupling reads
(linear_form_view2, boundary_dof_ids, zero_dof_ids, newton_final_norms)."""
import os

import numpy as np
import pytest

from test_nonlinear_solid import BEAM, GOLDEN_CASES, beam
from test_periodic_gpu import facade

pytestmark = pytest.mark.gpu


def fixed_point_step(nl):
    nl.fixed_point_solve2()
    nl.advance_time2()


@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_golden_series_through_fixed_point_steps_is_bitwise_step_time2(golden_dir, case):
    from oracle import harness as hz
    nl, twin = beam(case), beam(case)
    u, u_twin = nl.solution_view("displacement", "x"), twin.solution_view("displacement", "x")
    for i in range(10):
        fixed_point_step(nl)
        twin.step_time2()
        ref = hz.golden_to_lexicographic(np.genfromtxt(os.path.join(golden_dir, "ref", GOLDEN_CASES[case]["refdir"],
                                                                    f"x_{i}.txt")))
        assert np.allclose(u, ref)                     # the reference's criterion
        assert np.abs(u - ref).max() < 1e-8, (i, np.abs(u - ref).max())
        assert u.tobytes() == u_twin.tobytes() and nl.x_dot.tobytes() == twin.x_dot.tobytes(), i
    assert nl.current_time == twin.current_time
    if GOLDEN_CASES[case]["hardening"]:
        s, s_twin = nl.domain_.State("accumulated_plastic_strain"), twin.domain_.State("accumulated_plastic_strain")
        assert s.max() > 0.05 and s.tobytes() == s_twin.tobytes()


@pytest.mark.parametrize("pairs,cv", [({}, [(1, 1, 0.3)]), ({3: 4}, None)], ids=["constant_velocity", "periodic"])
def test_bitwise_twin_with_constant_velocity_and_periodic(pairs, cv):
    nl, x = facade("square-nurbs.mesh", "neohook", pairs, steps=0, cv=cv)
    twin, x_twin = facade("square-nurbs.mesh", "neohook", pairs, steps=0, cv=cv)
    assert (nl.fold_ is not None) == bool(pairs) and (len(nl.constant_velocity_dofs_) > 0) == bool(cv)
    for _ in range(4):
        fixed_point_step(nl)
        twin.step_time2()
        assert x.tobytes() == x_twin.tobytes() and nl.x_dot.tobytes() == twin.x_dot.tobytes()
    assert np.abs(x).max() > 1e-4
    if cv:
        top = nl.boundary_dof_ids("displacement", 1, 1)
        assert np.all(nl.x_dot[top] == 0.3)


def test_repeated_solves_commit_nothing():
    nl, twin = beam("j2"), beam("j2")                # iterative_mode False (BEAM["newton"])
    assert BEAM["newton"][4] is False
    # the first step that flows plastically (the twin tells), reached by step_time2
    for _ in range(10):
        before = twin.domain_.State("accumulated_plastic_strain")
        twin.step_time2()
        if not np.array_equal(twin.domain_.State("accumulated_plastic_strain"), before):
            break
        nl.step_time2()
    x0, v0 = nl.x.copy(), nl.x_dot.copy()
    s0 = nl.domain_.State("accumulated_plastic_strain").copy()
    t0 = nl.current_time
    nl.fixed_point_solve2()
    xa, va = nl.fixed_point_advance2()
    assert xa.shape == (len(nl.x) // 2, 2) and va.shape == xa.shape
    first = (xa.tobytes(), va.tobytes())
    for _ in range(2):
        nl.fixed_point_solve2()
        xb, vb = nl.fixed_point_advance2()
        assert xb is xa and vb is va
        assert (xa.tobytes(), va.tobytes()) == first
    views = nl.fixed_point_advanced_vector_views()
    assert views[0] is xa and views[1] is va
    assert np.array_equal(nl.x, x0) and np.array_equal(nl.x_dot, v0) and nl.current_time == t0
    assert np.array_equal(nl.domain_.State("accumulated_plastic_strain"), s0)
    h = nl.newton_history[-1]
    rel, final = nl.newton_final_norms("nonlinear_solid")
    assert final == h["norm"] and rel == h["norm"] / h["norm0"] and h["norm0"] > 0
    nl.advance_time2()
    assert nl.x.tobytes() == xa.reshape(-1).tobytes() and nl.x_dot.tobytes() == va.reshape(-1).tobytes()
    assert not np.array_equal(nl.x, x0)
    assert not np.array_equal(nl.domain_.State("accumulated_plastic_strain"), s0)
    assert nl.domain_.State("accumulated_plastic_strain").tobytes() == twin.domain_.State("accumulated_plastic_strain").tobytes()
    assert nl.x.tobytes() == twin.x.tobytes()
    assert nl.current_time == t0 + nl.time_step_size


def test_refusals():
    nl = beam("neohook")
    with pytest.raises(RuntimeError, match=r"FixedPointAdvance2\(\) should be called after FixedPointSolve2\(\)"):
        nl.fixed_point_advance2()
    with pytest.raises(RuntimeError, match="fixed_point_solve2"):
        nl.advance_time2()
    nl.fixed_point_solve2()
    with pytest.raises(RuntimeError, match="fixed-point step is open"):
        nl.step_time2()
    nl.advance_time2()
    with pytest.raises(RuntimeError, match="FixedPointAdvance2"):     # the predictor is re-armed
        nl.fixed_point_advance2()
    nl.step_time2()
    with pytest.raises(KeyError):
        nl.linear_form_view2("lhs")
    # no body force, no traction: the reference makes no "rhs" linear form
    bare = beam("neohook", finish=False)
    bare.boundary_condition.initial.body_force_.clear()
    bare.setup(1)
    with pytest.raises(KeyError, match="rhs"):
        bare.linear_form_view2("rhs")


def beam_with_body_force(value):
    nl = beam("neohook", finish=False)
    bf = nl.boundary_condition.initial.body_force_
    bf[GOLDEN_CASES["neohook"]["body_force"][0]] = value
    nl.setup(1)
    nl.configure_newton(*BEAM["newton"])
    nl.time_step_size = GOLDEN_CASES["neohook"]["dt"]
    return nl


def test_rhs_view_scaled_is_the_doubled_body_force(tmp_path):
    comp, value = GOLDEN_CASES["neohook"]["body_force"]
    a = beam("neohook")
    view = a.linear_form_view2("rhs")
    assert view is a.linear_form_view2("rhs") and np.abs(view).max() > 0
    view *= 2.0
    b = beam_with_body_force(2 * value)
    for _ in range(3):
        a.step_time2()
        b.step_time2()
        assert np.abs(a.x - b.x).max() <= 1e-12 * np.abs(b.x).max()
    # the same through the fixed-point entries
    c = beam("neohook")
    c.linear_form_view2("rhs")[:] *= 2.0
    for _ in range(3):
        fixed_point_step(c)
    assert np.abs(c.x - b.x).max() <= 1e-12 * np.abs(b.x).max()
    # advance_time2 writes the .npz series step_time2 writes
    paths = []
    for stepper in ("fixed_point", "step_time2"):
        nl = beam("neohook")
        rc = nl.runtime_communication
        path = str(tmp_path / f"{stepper}.npz")
        rc.set_fname(path)
        rc.append_should_save("x", 1)
        rc.append_should_save("v", 2)
        for _ in range(4):
            fixed_point_step(nl) if stepper == "fixed_point" else nl.step_time2()
        paths.append(path)
    fa, fb = np.load(paths[0]), np.load(paths[1])
    assert sorted(fa.files) == sorted(fb.files) and len(fa.files) == 4 + 2
    for k in fa.files:
        assert fa[k].tobytes() == fb[k].tobytes(), k


def test_dof_ids():
    nl = beam("neohook")
    zero = nl.zero_dof_ids("displacement")
    union = np.unique(np.concatenate([nl.boundary_dof_ids("displacement", bid, c) for bid, c in BEAM["clamped"]]))
    assert np.array_equal(zero, union) and len(zero) > 0
    x_ref = nl.solution_view("displacement", "x_ref").reshape(-1, 2)
    lo, hi = x_ref.min(axis=0), x_ref.max(axis=0)
    tol = 1e-12 * np.abs(x_ref).max()
    for bid in range(4):
        for comp in range(2):
            ids = nl.boundary_dof_ids("displacement", bid, comp)
            assert len(ids) == 5 and np.all(np.diff(ids) > 0) and np.all(ids % 2 == comp)
            X = x_ref[ids // 2]
            # the face's nodes lie on one side of the 5 x 1 beam: one coordinate constant, at the extreme of the patch
            assert any(np.ptp(X[:, d]) <= tol and min(abs(X[0, d] - lo[d]), abs(X[0, d] - hi[d])) <= tol for d in range(2)), X
    # constant velocity implies dirichlet
    cv, _ = facade("square-nurbs.mesh", "neohook", {}, steps=0, cv=[(1, 1, 0.3)])
    assert np.array_equal(cv.zero_dof_ids("displacement"),
                          np.unique(np.concatenate([cv.boundary_dof_ids("displacement", 0, c) for c in range(2)]
                                                   + [cv.boundary_dof_ids("displacement", 1, 1)])))
    # periodic: the joined faces' ids are folded onto the same dofs
    per, x = facade("square-nurbs.mesh", "neohook", {3: 4}, steps=0)
    for comp in range(2):
        a, b = per.boundary_dof_ids("displacement", 2, comp), per.boundary_dof_ids("displacement", 3, comp)
        assert np.array_equal(a, b) and a.max() < len(x)
    # the Dirichlet marker of facade(): every component of bid 0, folded like every other id
    union = np.unique(np.concatenate([per.boundary_dof_ids("displacement", 0, c) for c in range(2)]))
    assert np.array_equal(per.zero_dof_ids("displacement"), union) and union.max() < len(x)
