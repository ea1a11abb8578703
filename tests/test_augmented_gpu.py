"""Augmented-Lagrangian mortar contact on the device (csrc/kernels_face_augmented.hpp, the AUG variants in csrc/contact.hip
and csrc/kernels_face_consistent.hpp) through MortarContact.SetAugmented / SetLagrange / UpdateLagrange, against the
long-double reference of tests/_augmented_reference.py on the faces, bodies and multipliers of tests/_augmented_cases.py.

(1) every case, plane and sphere, every face: residual, nodal pressure / area / unclamped gap, force, pressure integral and
    the assembled (frozen) tangent at _face_cases.TOL's contact bars; the frozen and the consistent action against the
    reference's products with the two vectors of the face (contact_K on the scale without cancellation);
(2) the consistent action is the derivative of the device's own residual: central quotient at h = 1e-6 on FD_CASES within
    10 x the float64 figure of tests/_contact_consistent_cases.py;
(3) UpdateLagrange: the four numbers and the multipliers afterwards against the reference, apply=False keeps the bytes, a
    released node holds exactly 0.0, two identical sequences give identical bytes, the history scalars are left alone,
    SetLagrange projects;
(4) nothing changes when off: on and off again gives the bytes of a handle never switched; on with lambda = 0 and every
    point penetrating equals the penalty law to 1e-15 of the largest entry;
(5) a rigid spline body equals its analytic twin at tests/test_contact_spline_gpu.py's bound;
(6) friction reads the augmented nodal pressure: residual and trial state against tests/_friction_reference.py;
(7) the refusals.

Every test here fails on a tree without the feature (no SetAugmented).

Worst figures measured on an MI355X (34 tests, 5 s): (1) r 1.5e-14, pressure 1.5e-14, area 5.6e-16, gap 6.1e-15, K 1.5e-14, force
1.5e-14 (all mix2d_31 order 41, sphere), frozen action 7.5e-15, consistent action 8.3e-16; (2) 1.7e-10 of the bar 9.5e-10, the
frozen action at least 4.4e-2 away; (3) 1.5e-14; (5) residual, tangent and multipliers 4.2e-14 of the bound 1e-13 (the points
far outside the circle, which the penalty law never asks for, cost the closest-point search that much), the consistent
action 1.1e-12 on the scale without cancellation; (6) r 2.1e-15, K 2.7e-16, xi 2.5e-14, friction force 1.3e-14."""
import types

import numpy as np
import pytest

import _augmented_cases as ac
import _augmented_reference as ar
import _face_cases as fc
import _face_reference as fr
from test_boundary_action_cpu import vectors

pytestmark = pytest.mark.gpu
T = fc.TOL


def faces_gpu():
    import test_faces_gpu
    return test_faces_gpu


def handle(case, axis, side, order, kind, lam=None, on=True):
    G = faces_gpu().contact_handle(case, axis, side, order, kind)
    if on:
        G.SetAugmented(True)
    if lam is not None:
        G.SetLagrange(np.array(lam))
    return G


def close(a, b, tol):
    """max |a - b| <= tol max |b|; a reference that is exactly zero asks for exact zeros"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    return float(np.abs(a - b).max() / scale) if scale > 0 else (0.0 if not np.any(a) else np.inf)


def action(G, v, factor=1.0):
    y0 = np.random.default_rng(11).standard_normal(len(v))
    y = y0.copy()
    G.ApplyTangent(np.array(v), y, factor)
    return y - y0


def on_scale(got, want, scale):
    s = float(np.max(scale))
    return float(np.abs(got - want).max() / s) if s > 0 else (0.0 if not np.any(got) else np.inf)


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("case,order", ac.CASES, ids=lambda c: str(c))
def test_residual_and_tangents_against_the_reference(case, order, kind):
    tf = faces_gpu()
    u = fc.displacement(case)
    r0, A0 = tf.prefill(case)
    worst = dict(r=0.0, pressure=0.0, area=0.0, gap=0.0, K=0.0, force=0.0, last_pressure=0.0, frozen=0.0, consistent=0.0)
    for axis, side in fc.faces(case):
        R = ac.reference(case, axis, side, order, kind)
        G = handle(case, axis, side, order, kind, R.lam64)
        assert np.array_equal(G.MarkedNodes(), R.nodes)
        r, A = r0.copy(), A0.copy()
        G.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
        G.BoundaryPostTimeAdvance(u)
        tf.assert_only_the_face_changed(case, R.nodes, r, A)
        p = G.AveragePressure()
        assert np.array_equal(p == 0.0, np.asarray(R.pressure == 0)) and np.all(p <= 0.0)      # (no node near its switch)
        area, gap = np.zeros(len(R.nodes)), np.zeros(len(R.nodes))
        G.GetNodal(area, gap)
        figures = dict(r=close(r - r0, R.r, 1), pressure=close(p, R.pressure, 1), area=close(area, R.area, 1),
                       gap=close(gap, R.gap, 1), K=close(tf.dense(case, A - A0), R.K_frozen64, 1),
                       force=close(G.last_force_, R.last_force, 1), last_pressure=close(G.last_pressure_, R.last_pressure, 1))
        assert close(G.last_area_, R.last_area, 1) <= T["contact_area"]
        for consistent, key, Kv, scale in ((False, "frozen", R.Kv_frozen, R.scale_frozen), (True, "consistent", R.Kv, R.scale)):
            G.SetConsistentTangent(consistent)
            G.Linearize(u)
            assert G.HoldsAugmentedRecord() and G.HoldsConsistentRecord() == consistent
            figures[key] = max(on_scale(action(G, v, fc.GRAD_FACTOR), Kv[k], scale[k]) for k, v in enumerate(vectors(case, axis, side)))
        assert not np.array_equal(R.Kv, R.Kv_frozen) or R.n_active == 0
        for k, v in figures.items():
            worst[k] = max(worst[k], v)
    print(f"figures augmented contact {case} order {order} {kind}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["r"] <= T["contact_r"] and worst["pressure"] <= T["contact_pressure"] and worst["gap"] <= T["contact_pressure"]
    assert worst["area"] <= T["contact_area"] and worst["K"] <= T["contact_K"]
    assert worst["force"] <= T["contact_force"] and worst["last_pressure"] <= T["contact_force"]
    assert worst["frozen"] <= T["contact_K"] and worst["consistent"] <= T["contact_K"]


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("case", ac.FD_CASES)
def test_consistent_action_is_the_derivative_of_the_device_residual(case, kind):
    u = np.array(fc.displacement(case))
    h, worst, frozen = ac.FD_STEP, 0.0, np.inf
    for axis, side in fc.faces(case):
        R = ac.reference(case, axis, side, -1, kind)
        G = handle(case, axis, side, -1, kind, R.lam64)
        for k, v in enumerate(vectors(case, axis, side)):
            rp, rm = np.zeros(len(u)), np.zeros(len(u))
            G.AddBoundaryResidual(u + h * v, rp)
            G.AddBoundaryResidual(u - h * v, rm)
            q = (rp - rm) / (2 * h)
            scale = R.scale[k].max() / fc.GRAD_FACTOR
            for consistent in (True, False):
                G.SetConsistentTangent(consistent)
                G.Linearize(u)
                dev = float(np.abs(action(G, v) - q).max() / scale)
                if consistent:
                    worst = max(worst, dev)
                else:
                    frozen = min(frozen, dev)
    bar = 10 * ac.F64_WORST
    print(f"figures augmented device quotient {case} {kind}: consistent {worst:.2e} (bar {bar:.2e}), frozen at least {frozen:.2e}")
    assert worst <= bar
    assert frozen > 1.0e3 * bar


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("case,order", ac.CASES, ids=lambda c: str(c))
def test_update_lagrange(case, order, kind):
    u = fc.displacement(case)
    worst = 0.0
    for axis, side in fc.faces(case):
        R = ac.reference(case, axis, side, order, kind)
        runs = []
        for _ in range(2):
            G = handle(case, axis, side, order, kind, R.lam64)
            before = G.Lagrange()
            assert np.array_equal(before, R.lam64)
            measured = G.UpdateLagrange(u, apply=False)
            assert G.Lagrange().tobytes() == before.tobytes()
            applied = G.UpdateLagrange(u)
            runs.append((measured, applied, G.Lagrange()))
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][2].tobytes() == runs[1][2].tobytes()
        measured, applied, lam = runs[0]
        assert measured["n_active"] == applied["n_active"] == R.n_active
        for key in ("violation", "norm"):
            assert measured[key] == applied[key]
        assert np.all(lam[np.asarray(R.pressure == 0)] == 0.0) and not np.any(np.signbit(lam[lam == 0.0])) and np.all(lam <= 0.0)
        figures = (close(measured["violation"], R.violation, 1), close(measured["norm"], R.norm, 1),
                   close(measured["max_lagrange"], R.max_lagrange_kept, 1), close(applied["max_lagrange"], R.max_lagrange_applied, 1),
                   close(lam, R.pressure, 1))
        worst = max(worst, *figures)
    print(f"figures augmented update {case} order {order} {kind}: {worst:.2e}")
    assert worst <= T["contact_pressure"]


def test_update_leaves_the_history_alone_and_set_projects():
    import torch
    case, axis, side = "rep3d_p1", 2, 1
    R = ac.reference(case, axis, side, -1, "plane")
    G = handle(case, axis, side, -1, "plane", R.lam64)
    u = np.array(fc.displacement(case))
    G.AddBoundaryResidual(u, np.zeros(len(u)))
    G.BoundaryPostTimeAdvance(u)
    hist = (G.last_area_, G.last_pressure_, G.last_force_.tobytes())
    out = G.UpdateLagrange(1.3 * u, apply=False)
    G.BoundaryPostTimeAdvance(u)
    assert (G.last_area_, G.last_pressure_, G.last_force_.tobytes()) == hist and G.last_area_ > 0
    # device arguments: u and the multipliers
    dev = torch.device("cuda", 0)
    assert G.UpdateLagrange(torch.from_numpy(1.3 * u).to(dev), apply=False) == out
    mixed = np.where(np.arange(len(R.nodes)) % 2 == 0, 1.0, -1.0) * np.abs(R.lam64 - 1.0)
    G.SetLagrange(torch.from_numpy(mixed).to(dev))
    assert np.array_equal(G.Lagrange(), np.minimum(mixed, 0.0))
    G.SetLagrange(mixed)
    assert np.array_equal(G.Lagrange(), np.minimum(mixed, 0.0))
    G.FillLagrange(-2.5)
    assert np.all(G.Lagrange() == -2.5)
    G.FillLagrange()
    assert not np.any(G.Lagrange())
    with pytest.raises(ValueError, match="multipliers"):
        G.SetLagrange(np.zeros(len(R.nodes) + 1))
    # off and on again: the multipliers start at zero
    G.SetLagrange(R.lam64)
    G.SetAugmented(True)
    assert np.array_equal(G.Lagrange(), R.lam64)
    G.SetAugmented(False)
    G.SetAugmented(True)
    assert not np.any(G.Lagrange())


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
def evaluate(G, case, u, v):
    """(r, A, frozen action, consistent action, pressure bytes) of a handle on the pre-filled vectors"""
    r0, A0 = faces_gpu().prefill(case)
    r, A = r0.copy(), A0.copy()
    G.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
    out = [r, A]
    for consistent in (False, True):
        G.SetConsistentTangent(consistent)
        G.Linearize(u)
        out.append(action(G, v, 0.7))
    G.SetConsistentTangent(False)
    return out + [G.AveragePressure()]


@pytest.mark.parametrize("case,axis,side", [("rep3d_p1", 2, 1), ("rep2d_p2", 1, 0)])
def test_nothing_changes_when_off(case, axis, side):
    from mimi_amd.integrators import MortarContact, RigidPlane
    u, v = np.array(fc.displacement(case)), np.array(vectors(case, axis, side)[0])
    R = ac.reference(case, axis, side, -1, "plane")
    never = evaluate(handle(case, axis, side, -1, "plane", on=False), case, u, v)
    G = handle(case, axis, side, -1, "plane", R.lam64)
    on = evaluate(G, case, u, v)
    assert G.HoldsAugmentedRecord() and not np.array_equal(on[0], never[0]) and not np.array_equal(on[3], never[3])
    G.SetAugmented(False)
    assert G.HoldsAugmentedRecord() and not G.augmented_               # (the record is a snapshot)
    off = evaluate(G, case, u, v)
    assert not G.HoldsAugmentedRecord()
    for a, b in zip(off, never):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(RuntimeError, match="not in the augmented mode"):
        G.UpdateLagrange(u)
    # the mode on with lambda = 0 and every point penetrating: the penalty law
    pts = fc.points(case, axis, side)
    b = fc.body(case, axis, side, -1, "plane")
    normal = np.asarray(b["normal"])
    depth = float(((pts.x.astype(np.float64) - np.asarray(b["point"])) @ normal).max())
    deep = list(np.asarray(b["point"]) + (depth + 0.05) * normal)
    pair = []
    for mode in (False, True):
        H = MortarContact(RigidPlane(deep, b["normal"], fc.PENALTY), "contact", faces_gpu().pattern_of(case)[0],
                          fc.product_patch(case), axis, side).Prepare()
        H.SetAugmented(mode)
        pair.append(evaluate(H, case, u, v))
    r0, A0 = faces_gpu().prefill(case)
    assert np.all(pair[0][4] < 0)
    for k, (a, b_) in enumerate(zip(pair[1], pair[0])):
        base = (r0, A0, 0.0, 0.0, 0.0)[k]
        assert np.abs(a - b_).max() <= 1e-15 * np.abs(b_ - base).max(), k


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
def test_spline_body_equals_its_analytic_twin():
    import _spline_bodies as sb
    from test_contact_spline_gpu import TWINS, device_contact, product_body
    case, cid = [t for t in TWINS if t[1] == "6x3-p2-circle-seam-down"][0]
    (n_el, p, axis), name = case
    P, patch, tables, u, body = sb.setup((n_el, p, axis), name)
    out, lam = [], None
    for b in (body["twin"], body):
        G, rowptr = device_contact(P, n_el, p, axis, 1, product_body(b))
        if lam is None:                                                # sized on the twin's penalty pressure
            G.AddBoundaryResidual(u, np.zeros(P.n_vdofs))
            pmax = float(np.abs(G.AveragePressure()).max())
            rng = np.random.default_rng(ac.SEED)
            n = len(G.MarkedNodes())
            mask = rng.random(n) < 0.5
            lam = np.where(mask, -pmax * rng.random(n), 0.0)
            assert pmax > 0 and np.any(lam < 0)
        G.SetAugmented(True)
        G.SetLagrange(lam)
        r, A = np.zeros(P.n_vdofs), np.zeros(rowptr[-1])
        G.AddBoundaryResidualAndGrad(u, 0.6, r, A)
        G.SetConsistentTangent(True)
        G.Linearize(u)
        v = np.random.default_rng(21).standard_normal(P.n_vdofs)
        out.append((r, A, action(G, v), G.UpdateLagrange(u)["violation"], G.Lagrange()))
    assert np.abs(out[0][0]).max() > 0 and np.any(out[0][4] == 0.0) and np.any(out[0][4] < 0)
    errs = [sb.rel(out[1][k], out[0][k]) for k in (0, 1, 4)] + [abs(out[1][3] - out[0][3]) / out[0][3]]
    # the consistent action cancels (eps dG - gt dA): its two sides are compared on the scale without cancellation of
    # tests/test_contact_consistent_gpu.py's spline test, max_i (K_abs |v|)_i, at the actions' bar
    import _contact_consistent_reference as ccr
    x = patch.control_points.astype(np.longdouble) + np.asarray(u, dtype=np.longdouble).reshape(-1, patch.dim)
    K_abs = np.asarray(ccr.consistent_contact(fr.face_points(fr.face_basis(patch.degrees, patch.knots, axis, 1), x), body["twin"],
                                              1.0e4).K_abs, dtype=np.float64)
    err_action = float(np.abs(out[1][2] - out[0][2]).max() / (K_abs @ np.abs(v)).max())
    print(cid, "augmented: residual, tangent, multipliers, violation against the analytic body:", errs, "bound",
          sb.bound(sb.MEASURED_TWIN[cid]), "consistent action", err_action)
    assert max(errs) < sb.bound(sb.MEASURED_TWIN[cid])
    assert np.abs(out[0][2]).max() > 0 and err_action <= T["contact_K"]


# ---- (6) ---------------------------------------------------------------------------------------------------------------------
def test_friction_reads_the_augmented_pressure():
    import _friction_cases as fx
    import _friction_reference as fq
    from mimi_amd.integrators import MortarContact
    case, axis, side, order, kind = "rep2d_p3", 1, 0, -1, "plane"
    dim = fc.product_patch(case).dim
    lam = ac.multipliers(case, axis, side, order, kind)[0]
    u0, u1, _ = fx.displacements(case)
    p = [fx.points(case, axis, side, order, k) for k in range(2)]
    body = fc.body(case, axis, side, order, kind)
    con = [ar.augmented_contact(p[k], body, fc.PENALTY, lam, fc.GRAD_FACTOR) for k in range(2)]
    # the tangential penalty: the cut between stick and slip in the widest gap of |s| / p_N, as tests/_friction_cases.py sizes it
    c0 = fq.point_pressure(p[0], con[0]) < 0
    probe = fq.tractions(p[1], fq.point_pressure(p[1], con[1]), types.SimpleNamespace(xi=np.zeros_like(p[0].x), xbar=p[0].x, c=c0),
                         fx.MU, 1.0)
    cut, margin = fx._cut((probe.sn[probe.on] / probe.pn[probe.on]).astype(np.float64))
    eps_t = float(fx.MU / cut)
    ev0 = fq.evaluate(p[0], con[0], fq.initial_state(len(p[0].x), dim), fx.MU, eps_t, with_tangent=False)
    ev1 = fq.evaluate(p[1], con[1], ev0.trial, fx.MU, eps_t, grad_factor=fc.GRAD_FACTOR)
    assert ev1.n_stick > 0 and ev1.n_slip > 0 and margin > 1e-6
    assert not np.array_equal(np.asarray(con[1].pressure == 0), np.asarray(fx.contact(case, axis, side, order, kind, 1).pressure == 0))
    tf = faces_gpu()
    G = MortarContact(fx.product_body(body, friction=fx.MU, tangential_coefficient=eps_t), "contact", tf.pattern_of(case)[0],
                      fc.product_patch(case), axis, side, quadrature_order=order).Prepare()
    G.SetAugmented(True)
    G.SetLagrange(np.array(lam))
    G.BoundaryPostTimeAdvance(u0)
    r0, A0 = tf.prefill(case)
    r, A = r0.copy(), A0.copy()
    G.AddBoundaryResidualAndGrad(u1, fc.GRAD_FACTOR, r, A)
    G._history()
    assert (G.n_stick_, G.n_slip_) == (ev1.n_stick, ev1.n_slip)
    G.CommitFriction()
    xi, xbar, c = G.FrictionState()
    perm, _ = fr.match_points(p[1].x, xbar.reshape(-1, dim))
    assert np.array_equal(c.reshape(-1)[perm].astype(bool), ev1.trial.c)
    figures = dict(r=close(r - r0, con[1].r + ev1.r, 1), K=close(tf.dense(case, A - A0), con[1].K_frozen + ev1.K, 1),
                   xi=close(xi.reshape(-1, dim)[perm], ev1.trial.xi, 1), force=close(G.last_friction_force_, ev1.force, 1))
    print("figures augmented friction: " + " ".join(f"{k}={v:.2e}" for k, v in figures.items()))
    assert figures["r"] <= T["contact_r"] and figures["K"] <= T["contact_K"] and figures["xi"] <= fx.XI_TOL
    assert figures["force"] <= T["contact_force"]


# ---- (7) ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mimi_amd import _capi
    from mimi_amd.integrators import TANGENT_REFERENCE_FD
    case, axis, side = "rep2d_p2", 1, 0
    G = handle(case, axis, side, -1, "plane", on=False)
    with pytest.raises(RuntimeError, match="never set to the augmented mode"):
        G.Lagrange()
    G.sharded_ = True
    with pytest.raises(RuntimeError, match="ShardedContact"):
        G.SetAugmented(True)
    G.SetAugmented(False)
    G.sharded_ = False
    G.SetTangentMode(TANGENT_REFERENCE_FD)
    with pytest.raises(RuntimeError, match="reference-FD"):
        G.SetAugmented(True)
    assert not G.augmented_
    G.SetTangentMode(0)
    G.SetAugmented(True)
    with pytest.raises(RuntimeError, match="reference-FD"):
        G.SetTangentMode(TANGENT_REFERENCE_FD)
    with pytest.raises(RuntimeError, match="null"):
        _capi.check(_capi.lib().mimi_hip_contact_update_lagrange(G._handle(), None, 1, None))
    u = np.array(fc.displacement(case))
    assert G.UpdateLagrange(u)["n_active"] >= 0                        # (the handle works afterwards)
