"""Coulomb friction of MortarContact (csrc/kernels_face_friction.hpp) on the device against the long-double reference of
tests/_friction_reference.py, on the faces, bodies and staged history of tests/_friction_cases.py (tests/test_friction_cpu.py
asserts what those cases give).  Per case, kind of body and face, the stages of one handle:
  1  friction set, nothing committed: the bytes of a frictionless handle
  2  commit at u0: c the reference's, xi = 0, xbar the reference's points
  3  at u1: two runs bit-equal, residual-only = the residual of the grad call, only the face's rows and columns change,
     r and K against the reference, stick / slip counts exact, force and sum da |t| against the reference
  4  an evaluation at u2 and again at u1: the bytes of stage 3 (evaluations do not touch the committed state)
  5  commit by the null form after the evaluation at u1, and by BoundaryPostTimeAdvance(u1) on a second handle: states
     bit-equal, xi against the reference
  6  at u2 with the body increment d: r and K against the reference
  7  ResetFriction: the bytes of stage 1
  9  every refusal raises and the handle works afterwards
and (8) the closed forms of tests/test_friction_cpu.py through the device.  Points are matched between the reference (no
face numbering) and the device (face-major) by position.

Bars: fc.TOL["contact_r"], ["contact_K"], ["contact_force"], ["surface_x"] and fx.XI_TOL, relative to the largest reference
entry -- those of the frictionless kernels on these faces.  Measured on an MI355X, worst over the cases: r 1.9e-14, K 1.7e-14,
xi 1.2e-13, xbar 7.0e-16, friction force 2.0e-13, sum da |t| 2.2e-14; the stick / slip counts are exact."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _face_cases as fc
import _face_reference as fr
import _friction_cases as fx

pytestmark = pytest.mark.gpu
T = fc.TOL


def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def pattern_of(case):
    from mimi_amd.integrators import CSRPattern
    rowptr, col = fc.oracle_patch(case).sparsity()
    return CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), rowptr[-1]), np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def dense(case, values):
    pattern, _ = pattern_of(case)
    n = len(pattern.rowptr) - 1
    return sp.csr_matrix((values, pattern.col, pattern.rowptr), shape=(n, n)).toarray()


@functools.lru_cache(maxsize=None)
def prefill(case):
    pattern, _ = pattern_of(case)
    n = len(pattern.rowptr) - 1
    r0, A0 = np.random.default_rng(5).standard_normal(n), np.random.default_rng(6).standard_normal(pattern.nnz)
    r0.setflags(write=False)
    A0.setflags(write=False)
    return r0, A0


def assert_only_the_face_changed(case, nodes, r, A):
    pattern, entry_row = pattern_of(case)
    r0, A0 = prefill(case)
    dim = fc.product_patch(case).dim
    vd = (np.asarray(nodes)[:, None] * dim + np.arange(dim)).ravel()
    off = np.ones(len(r0), bool)
    off[vd] = False
    assert np.array_equal(r[off], r0[off])
    outside = off[entry_row] | off[pattern.col]
    assert np.array_equal(A[outside], A0[outside])


def handle(case, axis, side, order, kind, **friction):
    from mimi_amd.integrators import MortarContact
    body = fx.product_body(fc.body(case, axis, side, order, kind), **friction)
    return MortarContact(body, "contact", pattern_of(case)[0], fc.product_patch(case), axis, side, quadrature_order=order).Prepare()


def assemble(G, case, u, grad=True):
    """(r, A, history) of one call on the pre-filled vectors; the history without a commit"""
    r0, A0 = prefill(case)
    r, A = r0.copy(), A0.copy()
    if grad:
        G.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
    else:
        G.AddBoundaryResidual(u, r)
    G._history()
    hist = (G.last_area_, G.last_pressure_, G.last_force_.tobytes(), G.last_friction_force_.tobytes(), G.last_friction_traction_,
            G.n_stick_, G.n_slip_)
    return r, A, hist


def state_bytes(G):
    return tuple(a.tobytes() for a in G.FrictionState())


@pytest.mark.parametrize("kind", fx.KINDS)
@pytest.mark.parametrize("case,order", fx.CASES, ids=lambda c: str(c))
def test_friction_stages(case, order, kind):
    dim = fc.product_patch(case).dim
    u0, u1, u2 = fx.displacements(case)
    r0, A0 = prefill(case)
    worst = dict(xbar=0.0, r1=0.0, K1=0.0, force=0.0, traction=0.0, xi=0.0, r2=0.0, K2=0.0)
    for axis, side in fc.faces(case):
        ref = fx.reference(case, axis, side, order, kind)
        G = handle(case, axis, side, order, kind, friction=fx.MU, tangential_coefficient=ref.eps_t)
        body = G.nearest_distance_coeff_
        # 1
        plain = assemble(handle(case, axis, side, order, kind), case, u0)
        first = assemble(G, case, u0)
        assert np.array_equal(first[0], plain[0]) and np.array_equal(first[1], plain[1]) and first[2][:3] == plain[2][:3]
        assert first[2][5:] == (0, 0)
        # 2
        G.BoundaryPostTimeAdvance(u0)
        xi, xbar, c = G.FrictionState()
        perm, _ = fr.match_points(ref.pts[0].x, xbar.reshape(-1, dim))
        assert np.array_equal(c.reshape(-1)[perm].astype(bool), ref.ev0.trial.c) and not np.any(xi)
        worst["xbar"] = max(worst["xbar"], rel(xbar.reshape(-1, dim)[perm], ref.pts[0].x))
        # 3
        r, A, hist = assemble(G, case, u1)
        again = assemble(G, case, u1)
        assert np.array_equal(again[0], r) and np.array_equal(again[1], A) and again[2] == hist
        only_r = assemble(G, case, u1, grad=False)
        assert np.array_equal(only_r[0], r) and only_r[2] == hist
        assert_only_the_face_changed(case, ref.nodes, r, A)
        worst["r1"] = max(worst["r1"], rel(r - r0, ref.contact[1].r + ref.ev1.r))
        worst["K1"] = max(worst["K1"], rel(dense(case, A - A0), ref.contact[1].K + ref.ev1.K))
        assert (G.n_stick_, G.n_slip_) == (ref.ev1.n_stick, ref.ev1.n_slip) and G.n_stick_ > 0 and G.n_slip_ > 0
        worst["force"] = max(worst["force"], rel(G.last_friction_force_, ref.ev1.force))
        worst["traction"] = max(worst["traction"], rel(G.last_friction_traction_, ref.ev1.traction))
        # 4
        assemble(G, case, u2)
        back = assemble(G, case, u1)
        assert np.array_equal(back[0], r) and np.array_equal(back[1], A) and back[2] == hist
        # 5
        G.CommitFriction()
        G2 = handle(case, axis, side, order, kind, friction=fx.MU, tangential_coefficient=ref.eps_t)
        G2.BoundaryPostTimeAdvance(u0)
        G2.BoundaryPostTimeAdvance(u1)
        assert state_bytes(G) == state_bytes(G2)
        assert (G2.n_stick_, G2.n_slip_) == (ref.ev1.n_stick, ref.ev1.n_slip)
        xi, xbar, c = G.FrictionState()
        assert np.array_equal(c.reshape(-1)[perm].astype(bool), ref.ev1.trial.c)
        worst["xi"] = max(worst["xi"], rel(xi.reshape(-1, dim)[perm], ref.ev1.trial.xi))
        # 6
        body.step_displacement = ref.d
        r, A, _ = assemble(G, case, u2)
        worst["r2"] = max(worst["r2"], rel(r - r0, ref.contact[2].r + ref.ev2.r))
        worst["K2"] = max(worst["K2"], rel(dense(case, A - A0), ref.contact[2].K + ref.ev2.K))
        assert (G.n_stick_, G.n_slip_) == (ref.ev2.n_stick, ref.ev2.n_slip)
        # 7
        G.ResetFriction()
        body.step_displacement = None
        fresh = assemble(G, case, u0)
        assert np.array_equal(fresh[0], first[0]) and np.array_equal(fresh[1], first[1]) and fresh[2] == first[2]
        assert not any(np.any(a) for a in G.FrictionState())
    print(f"figures friction {case} order {order} {kind}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["xbar"] <= T["surface_x"]
    assert worst["r1"] <= T["contact_r"] and worst["r2"] <= T["contact_r"]
    assert worst["K1"] <= T["contact_K"] and worst["K2"] <= T["contact_K"]
    assert worst["force"] <= T["contact_force"] and worst["traction"] <= T["contact_force"]
    assert worst["xi"] <= fx.XI_TOL


def test_refusals_raise_and_leave_the_handle_working():
    from mimi_amd.integrators import TANGENT_REFERENCE_FD
    from mimi_amd.parallel import ShardedContact
    case, order, kind = "rep2d_p3", -1, "plane"
    axis, side = fc.faces(case)[0]
    ref = fx.reference(case, axis, side, order, kind)
    u0, u1, _ = fx.displacements(case)
    G = handle(case, axis, side, order, kind, friction=fx.MU, tangential_coefficient=ref.eps_t)
    G.BoundaryPostTimeAdvance(u0)
    expected = assemble(G, case, u1)
    y = np.zeros_like(u0)
    for refused in (lambda: G.SetTangentMode(TANGENT_REFERENCE_FD), lambda: G.Linearize(u0), lambda: G.ApplyTangent(u0, y)):
        with pytest.raises(RuntimeError, match="friction"):
            refused()
        again = assemble(G, case, u1)
        assert np.array_equal(again[0], expected[0]) and np.array_equal(again[1], expected[1]) and again[2] == expected[2]
    with pytest.raises(RuntimeError, match="friction"):
        ShardedContact(None, G.nearest_distance_coeff_, None, axis, side)
    # the C entries refuse on their own: friction on a handle in the reference-FD mode, and a commit without an evaluation
    F = handle(case, axis, side, order, kind)
    F.SetTangentMode(TANGENT_REFERENCE_FD)
    with pytest.raises(RuntimeError, match="reference-FD"):
        F.SetFriction(fx.MU, ref.eps_t)
    plain = assemble(handle(case, axis, side, order, kind), case, u0)
    F.SetTangentMode(0)
    assert np.array_equal(assemble(F, case, u0)[0], plain[0])
    H = handle(case, axis, side, order, kind, friction=fx.MU)
    with pytest.raises(RuntimeError, match="no evaluation"):
        H.CommitFriction()
    # friction = 0 on the body switches it off again: the frictionless bytes, whatever was committed
    G.nearest_distance_coeff_.friction = 0.0
    off = assemble(G, case, u0)
    assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
    G.Linearize(u0)


@pytest.mark.parametrize("delta,branch", [(1.0e-4, "stick"), (5.0e-3, "slip")])
def test_closed_forms_on_a_flat_face(delta, branch):
    """the face xi_1 = 0 of the block pushed 1e-3 into a plane, committed, then translated by delta along it: the total
    friction force is eps_T delta area (stick) or mu eps depth area (slip), along the translation, and it dissipates"""
    from mimi_amd.integrators import MortarContact, RigidPlane
    case = "block2d_p4"
    depth, eps, eps_t, mu = 1.0e-3, 1.0e4, 2.0e4, 0.3
    B = fc.product_patch(case)
    area = float(fr.face_points(fr.face_basis(B.degrees, B.knots, 1, 0), B.control_points).da.sum())
    body = RigidPlane([0.0, depth], [0.0, 1.0], eps, friction=mu, tangential_coefficient=eps_t)
    G = MortarContact(body, "contact", pattern_of(case)[0], B, 1, 0).Prepare()
    u0 = np.zeros(B.n_vdofs)
    u1 = u0.copy()
    u1[0::2] = delta
    G.BoundaryPostTimeAdvance(u0)
    r = np.zeros_like(u0)
    G.AddBoundaryResidual(u1, r)
    G._history()
    n_points = G.n_marked_boundaries_ * G.n_q_
    expected = eps_t * delta * area if branch == "stick" else mu * eps * depth * area
    assert (G.n_stick_, G.n_slip_) == ((n_points, 0) if branch == "stick" else (0, n_points))
    # internal force on the block: along +x, opposing the slip; the normal part has no x component on a flat face
    assert abs(r[0::2].sum() - expected) <= 1e-12 * expected
    assert abs(G.last_friction_force_[0] - expected) <= 1e-12 * expected and abs(G.last_friction_force_[1]) <= 1e-12 * expected
    assert abs(G.last_friction_traction_ - expected) <= 1e-12 * expected
    assert G.last_friction_traction_ <= mu * abs(G.last_pressure_) * (1 + 1e-12)
    assert r[0::2].sum() * delta >= 0.0
    # the body moving along with the block: no traction
    body.step_displacement = [delta, 0.0]
    r2 = np.zeros_like(u0)
    G.AddBoundaryResidual(u1, r2)
    G._history()
    # (x_q - xbar - d cancels to the rounding of the coordinates: a few units of it, times eps_T, over the area)
    assert abs(r2[0::2].sum()) <= 64 * np.finfo(np.float64).eps * float(np.abs(B.control_points).max()) * eps_t * area
