"""What tests/test_friction_stepping_gpu.py and the friction run of tests/test_friction_solid_gpu.py rely on, asserted on the
restatement of tests/_friction_stepping.py alone, without a GPU -- conditions, not measurements:
  - in every scenario sticking and slipping points occur and at least one point enters contact; at least one leaves in
    "punch", "e_run" and "e_short" (in "slide" none can: tests/_friction_stepping.py says why, and this asserts it);
  - gate margin: at every evaluation of every scenario no point of the face has |g| < 1e-9 extents;
  - kink margin: at every evaluation whose stick / slip counts a GPU test compares exactly no point has
    |eps_T |s| / (mu p_N) - 1| < 1e-9 -- every compared sample, none skipped;
  - the restated Newton converged in every implicit step, and the prescribed dofs moved as prescribed;
  - the CSR scatter of RoughContact's tangent: CSR times a vector is the dense reference K v to rounding.
Values used for the scenarios: tests/_friction_stepping.py (SLIDE_*, PRESS, PUNCH_*, SHORT_*).  Measured here: gate margins
slide 1.4e-4, punch 7.5e-4, e_run 4.3e-7, e_short 2.3e-5; kink margins at the compared samples slide 6.8e-2, punch 5.3e-2, e_run
1.8e-5, e_short 1.7 (over ALL evaluations: 3.6e-3, 3.9e-2, 1.8e-5, 1.7e-3); the test prints them."""
import numpy as np
import pytest

import _explicit_cases as ec
import _friction_stepping as fs

SCENARIOS = ("slide", "punch", "e_run", "e_short")


def scenario(name):
    """(evaluation log, kink margins of the compared samples, contact)"""
    if name in ("slide", "punch"):
        run = fs.implicit_run(name)
        assert all(s.info["converged"] for s in run.steps)
        return run.contact.log, [s.log[-1]["kink"] for s in run.steps], run.contact
    if name == "e_run":
        ref = ec.e_reference("friction")
        return ref.rough.log, [c[2] for c in ref.counts], ref.rough
    base = fs.short_reference()[0]
    return base.contact.log, [s.kink for s in base.shots], base.contact


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenarios_hold_what_the_gpu_tests_rely_on(name):
    log, compared, contact = scenario(name)
    gate = min(e["gate"] for e in log)
    kink = min(compared)
    stick, slip = sum(e["n_stick"] for e in log), sum(e["n_slip"] for e in log)
    print(f"figures friction stepping {name}: evaluations {len(log)} gate {gate:.2e} kink at the {len(compared)} compared samples "
          f"{kink:.2e} (all evaluations {min(e['kink'] for e in log):.2e}) stick {stick} slip {slip} entered {contact.entered} "
          f"left {contact.left}")
    assert stick > 0 and slip > 0
    assert contact.entered > 0
    if name == "slide":
        assert contact.left == 0
    else:
        assert contact.left > 0
    assert gate >= fs.MARGIN_MIN
    assert len(compared) > 0 and kink >= fs.MARGIN_MIN


def test_a_step_has_sticking_and_slipping_points_together():
    for name in ("slide", "punch"):
        assert any(s.n_stick > 0 and s.n_slip > 0 for s in fs.implicit_run(name).steps), name
    assert any(a > 0 and b > 0 for a, b, _ in fs.short_reference()[0].samples)


def test_prescribed_dofs_move_as_prescribed():
    S = fs.implicit_system("slide")
    run = fs.implicit_run("slide")
    want = S.x0[S.cv].copy()
    for k in range(fs.SLIDE_STEPS):
        vx, vy = fs.slide_drive(k)
        want = want + np.where(S.cv % 2 == 0, vx, vy) * fs.DT
    assert np.array_equal(run.x[S.cv], want)
    assert np.array_equal(run.v[S.cv], np.where(S.cv % 2 == 0, fs.SLIDE_SIDE[1] / fs.DT, 0.0))


def test_step_displacement_matters_to_the_restatement():
    with_d, without = fs.implicit_run("punch"), fs.implicit_run("punch", with_d=False)
    assert np.abs(with_d.contact.state.xi - without.contact.state.xi).max() > 1e-3 * np.abs(with_d.contact.state.xi).max()


def test_the_short_run_bars_are_small_beside_friction():
    base, plain, bars = fs.short_reference()
    for shot, other, (bx, bv, bxi) in zip(base.shots, plain.shots, bars):
        effect = float(np.abs(shot.x - other.x).max())
        print(f"figures friction stepping e_short: bar x {bx:.2e} v {bv:.2e} xi {bxi:.2e}; friction moves x by {effect:.2e}")
        assert 0 < bx and effect > 100 * bx
    assert base.shots[0].state.c.all() and np.abs(base.shots[0].state.xi).max() > 0          # in contact, with an elastic slip
    assert not base.shots[1].state.c.any()                                                   # and gone at the end


@pytest.mark.parametrize("name", ["slide", "punch"])
def test_csr_tangent_times_a_vector_is_the_dense_reference(name):
    """the scatter of RoughContact: after a commit and a further move (stick and slip, a non-zero elastic slip), the CSR
    values it adds, times a vector, against the long-double dense K times that vector"""
    import scipy.sparse as sp
    S = fs.implicit_system(name)
    run = fs.implicit_run(name)
    C = S.contact
    k = next(i for i, s in enumerate(run.steps) if s.n_stick > 0 and s.n_slip > 0)
    if name == "punch":
        C.body, C.d = fs.punch_twin(k + 1), fs.punch_shift(k)
    C.state = run.steps[k - 1].state
    x = run.steps[k].x
    n = len(x)
    r, vals = np.zeros(n), np.zeros(len(C.col))
    C.add_boundary_residual_and_grad(x, 0.6, r, vals)
    assert (C.n_stick, C.n_slip) == (run.steps[k].n_stick, run.steps[k].n_slip)
    K = C.dense_tangent(x, 0.6)[2]
    v = np.random.default_rng(3).standard_normal(n)
    got = sp.csr_matrix((vals, C.col, C.rowptr), shape=(n, n)) @ v
    want = K @ v.astype(np.longdouble)
    bound = 4 * 2.0 ** -53 * float((np.abs(K) @ np.abs(v).astype(np.longdouble)).max())     # one rounding per entry, one per sum
    err = float(np.abs(got - want).max())
    print(f"figures friction stepping csr {name}: |K v| {float(np.abs(want).max()):.3e} error {err:.2e} bound {bound:.2e}")
    assert np.abs(want).max() > 0 and np.abs(K - K.T).max() > 0
    assert err <= bound
