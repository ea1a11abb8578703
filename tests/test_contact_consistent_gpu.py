"""The consistent mortar-contact tangent as a matrix-free action (csrc/kernels_face_consistent.hpp) through the C ABI:
MortarContact.SetConsistentTangent / Linearize / ApplyTangent, the Krylov solvers' boundary term and the facade's
"contact_consistent_tangent" flag.

(1) the action on every face of every case and order of tests/test_boundary_action_gpu.py, plane and sphere, two vectors per
    face, against the long-double reference of tests/_contact_consistent_reference.py: the deviation from K v on the scale
    max_i (K_abs |v|)_i within _face_cases.TOL["contact_K"] (1e-11), the bar of the assembled contact tangent;
(2) the action is the derivative of the device's own residual: (r(u + h v) - r(u - h v)) / 2 h from AddBoundaryResidual,
    h = 1e-6, within 10 x the figure the CPU test records for the same quotient of the reference in float64
    (_contact_consistent_cases.F64_WORST); with the mode off the same comparison misses that bar by more than WIDE;
(3) semantics: the mode off and a mode switched on and off again leave the bytes of an untouched handle; equal bytes,
    accumulation, host and device arguments, the snapshot, the bytes of record, an inactive handle, the refusal with friction;
(4) GMRES with the Kronecker preconditioner on rho M + fac0 K plus the consistent contact action against the
    extended-precision solve of the assembled Jacobian plus the reference's dense new part;
(5) the facade: the beam on a plane, frozen against consistent.

Worst figures measured on an MI355X: (1) 1.9e-15 (block2d_p5, plane) of the bar 1e-11; (2) plane and sphere 1.6e-10 of the bar
9.5e-10, the frozen action at least 8.2e-2 away; the spline bodies within the bar too (on the scale of the handle's ASSEMBLED
frozen tangent, which lacks the new part and is 9 x smaller on the circle, the circle measured 1.02e-9); (4) 44 iterations
against 49 with the frozen term, x 9.7e-9 from the dense solve (bar 5.6e-7), the two systems' solutions 1.4 apart; (5) penalty
1e2: 3 Newton iterations per step in place of 9 (9 against 27, GMRES 141 against 399); penalty 1e4: not converged -- |r| 4.3e2 of
6.2e3 after 10 iterations, then 8.1e4 of 2.1e4 after 6 and 7.5e4 of 9.6e4 after 10."""
import numpy as np
import pytest
import scipy.sparse as sp

import _contact_consistent_cases as cc
import _contact_consistent_reference as ccr
import _face_cases as fc
import _face_reference as fr
import _kronecker_cases as kc
import _kronecker_reference as ref
import _spline_bodies as sb
from _cases import product_material
from test_boundary_action_cpu import vectors

pytestmark = pytest.mark.gpu
T = fc.TOL
WIDE = 1.0e3      # (2): the frozen action misses the bar of the consistent one by more than this factor


def pattern_of(case):
    from test_faces_gpu import pattern_of as cached
    return cached(case)[0]


def contact_handle(case, axis, side, order, kind, **kw):
    from test_faces_gpu import contact_handle as make
    return make(case, axis, side, order, kind, **kw)


def action(G, v, factor=1.0):
    """the increment of ApplyTangent in accumulate form on a random y0"""
    y0 = np.random.default_rng(11).standard_normal(len(v))
    y = y0.copy()
    G.ApplyTangent(np.array(v), y, factor)
    return y - y0


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("case,order", cc.ALL, ids=lambda c: str(c))
def test_consistent_action_against_the_reference(case, order, kind):
    u = fc.displacement(case)
    worst = 0.0
    for axis, side in fc.faces(case):
        P = cc.products(case, axis, side, order, kind)                 # (its K carries GRAD_FACTOR)
        G = contact_handle(case, axis, side, order, kind)
        G.SetConsistentTangent(True)
        G.Linearize(u)
        assert G.HoldsConsistentRecord()
        for k, v in enumerate(vectors(case, axis, side)):
            worst = max(worst, float(np.abs(action(G, v, fc.GRAD_FACTOR) - P.Kv[k]).max() / P.scale[k].max()))
        assert not G.HoldsTangentBlocks()
    print(f"figures consistent contact action {case} order {order} {kind}: K={worst:.2e}")
    assert worst <= T["contact_K"]


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
def device_quotient(G, u, v, h=cc.FD_STEP):
    n = len(u)
    rp, rm = np.zeros(n), np.zeros(n)
    G.AddBoundaryResidual(np.asarray(u) + h * v, rp)
    G.AddBoundaryResidual(np.asarray(u) - h * v, rm)
    return (rp - rm) / (2 * h)


def quotient_deviations(G, u, vs, scales):
    """worst deviation of the action from the device's difference quotient, mode on and mode off"""
    out = {}
    quotients = [device_quotient(G, u, np.array(v)) for v in vs]
    for mode in (True, False):
        G.SetConsistentTangent(mode)
        G.Linearize(np.array(u))
        assert G.HoldsConsistentRecord() == mode
        out[mode] = max(float(np.abs(action(G, v) - q).max() / s) for v, q, s in zip(vs, quotients, scales))
    return out[True], out[False]


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("case", cc.FD_CASES)
def test_action_is_the_derivative_of_the_device_residual(case, kind):
    u = fc.displacement(case)
    on, off = 0.0, np.inf
    for axis, side in fc.faces(case):
        P = cc.products(case, axis, side, -1, kind)
        G = contact_handle(case, axis, side, -1, kind)
        a, b = quotient_deviations(G, u, vectors(case, axis, side), P.scale.max(axis=1) / fc.GRAD_FACTOR)
        on, off = max(on, a), min(off, b)
    bar = 10 * cc.F64_WORST
    print(f"figures device quotient {case} {kind}: consistent {on:.2e} (bar {bar:.2e}), frozen at least {off:.2e}")
    assert on <= bar
    assert off > WIDE * bar


@pytest.mark.parametrize("block,name", [(sb.BLOCKS_2D[0], "circle-seam-down"), (sb.BLOCKS_3D[0], "dome")])
def test_action_is_the_derivative_with_a_rigid_spline_body(block, name):
    """The scale is the bar's own, max_i (K_abs |v|)_i, with the gap and the body's normal at the reference's points from the
    long-double closest point of tests/_closest_point.py (_contact_consistent_reference.spline_body_gap)."""
    from test_contact_spline_gpu import device_contact, product_body
    n_el, p, axis = block
    P, patch, tables, u, body = sb.setup(block, name)
    G, rowptr = device_contact(P, n_el, p, axis, 1, product_body(body))
    x = patch.control_points.astype(np.longdouble) + np.asarray(u, dtype=np.longdouble).reshape(-1, patch.dim)
    pts = fr.face_points(fr.face_basis(patch.degrees, patch.knots, axis, 1), x)
    K_abs = np.asarray(ccr.consistent_contact(pts, body, 1.0e4).K_abs, dtype=np.float64)
    vs = np.random.default_rng(21).standard_normal((2, P.n_vdofs))
    on, off = quotient_deviations(G, u, vs, [float((K_abs @ np.abs(v)).max()) for v in vs])
    bar = 10 * cc.F64_WORST
    print(f"figures device quotient spline body {name}: consistent {on:.2e} (bar {bar:.2e}), frozen {off:.2e}")
    assert on <= bar
    assert off > WIDE * bar


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
SEMANTICS = [("rep3d_p2", 2, 1), ("rep2d_p3", 1, 0)]


@pytest.mark.parametrize("case,axis,side", SEMANTICS)
def test_semantics_of_the_consistent_action(case, axis, side):
    import torch
    from mimi_amd import _capi
    from mimi_amd.integrators import MortarContact, RigidPlane
    B, u = fc.product_patch(case), np.array(fc.displacement(case))
    v = np.array(vectors(case, axis, side)[0])
    y0 = np.random.default_rng(3).standard_normal(len(v))
    n_q = fc.face_basis(case, axis, side).n_q_face

    def apply(G):
        y = y0.copy()
        G.ApplyTangent(v, y, 0.7)
        return y

    # the mode off, and on and off again: the bytes of a handle that never saw the entry
    untouched = contact_handle(case, axis, side, -1, "plane")
    untouched.Linearize(u)
    frozen = apply(untouched)
    off = contact_handle(case, axis, side, -1, "plane")
    off.SetConsistentTangent(False)
    off.Linearize(u)
    G = contact_handle(case, axis, side, -1, "plane")
    assert not G.consistent_tangent_ and not G.HoldsConsistentRecord()
    G.SetConsistentTangent(True)
    assert G.consistent_tangent_ and not G.HoldsConsistentRecord() and G.LinearizationBytes() == 0
    with pytest.raises(RuntimeError, match="before any mimi_hip_contact_linearize"):
        G.ApplyTangent(v, np.zeros_like(v))
    G.Linearize(u)
    runs = [apply(G), apply(G)]
    G.SetConsistentTangent(False)
    assert G.HoldsConsistentRecord()                                   # (the record is not touched)
    G.Linearize(u)
    assert not G.HoldsConsistentRecord()
    for other in (off, G):
        assert np.array_equal(apply(other), frozen) and other.LinearizationBytes() == untouched.LinearizationBytes()
    n_faces = G.n_marked_boundaries_
    assert untouched.LinearizationBytes() == n_faces * n_q * (1 + (B.dim - 1) * B.dim) * 8 + n_faces
    # two runs give equal bytes, and they are not the frozen action's
    assert np.array_equal(runs[0], runs[1]) and np.abs(runs[0] - y0).max() > 0 and not np.array_equal(runs[0], frozen)
    # accumulation: what a zero y gets is the increment (one addition per entry, off the face none)
    G.SetConsistentTangent(True)
    G.Linearize(u)
    assert np.array_equal(apply(G), runs[0])
    z = np.zeros_like(v)
    G.ApplyTangent(v, z, 0.7)
    assert np.array_equal(y0 + z, runs[0]) and np.any(z == 0)
    # device arguments
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y0.copy()).to(dev)
    G.ApplyTangent(torch.from_numpy(v).to(dev), yd, 0.7)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), runs[0])
    G.Linearize(torch.from_numpy(u).to(dev))
    assert np.array_equal(apply(G), runs[0])
    # the bytes of record
    n_marked = len(G.MarkedNodes())
    expect = n_faces * n_q * (2 + B.dim + (B.dim - 1) * B.dim) * 8 + 16 * n_marked + n_faces
    assert G.LinearizationBytes() == expect and G.HoldsConsistentRecord() and not G.HoldsTangentBlocks()
    # the snapshot survives whatever else the handle does
    other = 1.7 * u
    G.UpdateBody(penalty=3.0 * fc.PENALTY)
    G.GapNorm(other)
    G.AddBoundaryResidual(other, np.zeros_like(v))
    G.SetConsistentTangent(False)
    assert np.array_equal(apply(G), runs[0]) and G.HoldsConsistentRecord() and G.LinearizationBytes() == expect
    # ... and a new linearisation reads the handle as it is now: the mode off, then on with the new penalty
    G.Linearize(u)
    now_frozen = apply(G)
    assert not G.HoldsConsistentRecord() and not np.array_equal(now_frozen, runs[0]) and not np.array_equal(now_frozen, frozen)
    G.SetConsistentTangent(True)
    G.Linearize(u)
    now = apply(G)
    assert G.HoldsConsistentRecord() and not np.array_equal(now, runs[0]) and not np.array_equal(now, now_frozen)
    # a far-away body: y keeps its bits
    pts = fc.points(case, axis, side).x.astype(np.float64)
    normal = np.zeros(B.dim)
    normal[0] = 1.0
    far = MortarContact(RigidPlane(list(pts.min(axis=0) - 100.0), list(normal), fc.PENALTY), "contact", pattern_of(case), B,
                        axis, side).Prepare()
    far.SetConsistentTangent(True)
    far.Linearize(u)
    assert far.HoldsConsistentRecord() and np.array_equal(apply(far), y0)
    # friction: refused by the front end and by the C entry, each naming it
    rough = contact_handle(case, axis, side, -1, "plane")
    rough.SetFriction(0.3, 1.0e3)
    with pytest.raises(RuntimeError, match="friction"):
        rough.SetConsistentTangent(True)
    with pytest.raises(RuntimeError, match="friction"):
        _capi.check(_capi.lib().mimi_hip_contact_set_consistent_tangent(rough._handle(), 1))
    assert not rough.consistent_tangent_


def test_a_sharded_contact_is_refused():
    G = contact_handle("rep2d_p3", 1, 0, -1, "plane")
    G.sharded_ = True
    with pytest.raises(RuntimeError, match="ShardedContact"):
        G.SetConsistentTangent(True)
    G.SetConsistentTangent(False)


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
def _contact_system(name, fac0):
    """test_boundary_action_gpu.py::_boundary_system with the contact face alone (axis 2, side 1, a plane through the deformed
    face's mean height): (domain, contact, solver, J, patch, ess, u, b, the plane as the reference's dict)"""
    from mimi_amd.integrators import CSRPattern, MortarContact, NonlinearSolid, RigidPlane
    from test_kronecker_gpu import _kronecker_solver
    P, B = kc.solve_patch(name)
    ess, u, b = kc.solve_inputs(name)
    u = np.array(u)
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    x = B.control_points + u.reshape(-1, P.dim)
    top = x[:, 2] >= x[:, 2].max() - 0.35 * (x[:, 2].max() - x[:, 2].min())
    body = dict(kind="plane", point=[0.0, 0.0, float(x[top, 2].mean())], normal=[0.0, 0.0, -1.0])
    contact = MortarContact(RigidPlane(body["point"], body["normal"], 1e4), "contact", pattern, B, 2, 1).Prepare()
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    G.AddDomainResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    before = vals.copy()
    contact.AddBoundaryResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    contact.BoundaryPostTimeAdvance(u)
    nodal = contact.AveragePressure()
    assert contact.last_area_ > 0 and np.abs(vals - before).max() > 0 and np.any(nodal == 0.0) and np.any(nodal != 0.0)
    S = _kronecker_solver(pattern, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))
    S.Eliminate(None, vals)
    J = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs))
    return G, contact, S, J, P, B, ess, u, b, body


def test_gmres_with_the_consistent_contact_term():
    name, fac0 = "p2_6x4x2", 1e-2
    G, contact, S, J, P, B, ess, u, b, body = _contact_system(name, fac0)
    # the dense system: the assembled Jacobian plus the reference's new part, its essential rows and columns removed
    x = B.control_points.astype(np.longdouble) + u.reshape(-1, P.dim).astype(np.longdouble)
    pts = fr.face_points(fr.face_basis(B.degrees, B.knots, 2, 1), x)
    K_new = np.asarray(ccr.consistent_contact(pts, body, 1e4, fac0).K_new, dtype=np.float64)
    assert np.abs(K_new).max() > 0
    keep = np.ones(P.n_vdofs)
    keep[np.asarray(list(ess), dtype=np.int64)] = 0.0
    J_new = J.toarray() + keep[:, None] * K_new * keep[None, :]
    x_ref = np.array([float(v) for v in ref.solve_extended(J_new, b)])
    x_frozen_ref = np.array([float(v) for v in ref.solve_extended(J, b)])
    S.max_iter = 3000
    S.preconditioner = "kronecker"
    nan = lambda: np.full(len(b), np.nan)
    G.Linearize(u)
    got = {}
    for mode in (False, True):
        contact.SetConsistentTangent(mode)
        contact.Linearize(u)
        S.SetOperator(G, kc.RHO, fac0, 0.0)
        S.AddBoundaryOperator(contact, fac0)
        got[mode] = (S.Mult(None, b, nan()), S.final_iter_, S.converged_)
    scale = np.abs(x_ref).max()
    dev = np.abs(got[True][0] - x_ref).max() / scale
    dev_frozen = np.abs(got[False][0] - x_frozen_ref).max() / np.abs(x_frozen_ref).max()
    apart = np.abs(x_frozen_ref - x_ref).max() / scale
    print(f"\n{name} fac0 {fac0:g} with the consistent contact term: iterations {got[True][1]} (frozen operator "
          f"{got[False][1]}), x deviates {dev:.3g} (bar {kc.BAR * kc.DEV_SOLVE:.3g}; frozen operator against its own system "
          f"{dev_frozen:.3g}); the two systems' solutions are {apart:.3g} apart")
    assert got[True][2] and np.isfinite(got[True][0]).all()
    assert dev <= kc.BAR * kc.DEV_SOLVE
    assert apart > 1e3 * kc.BAR * kc.DEV_SOLVE       # the new part is in the system: the frozen solution is not its solution


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
def test_facade_consistent_against_frozen():
    from test_boundary_action_gpu import FACADE_PENALTY, MATRIX_FREE, _beam, _mark_contact, _three_steps
    routes = {}
    for route, flags in (("frozen", MATRIX_FREE), ("consistent", MATRIX_FREE + [("contact_consistent_tangent", 1)])):
        nl = _beam(flags, _mark_contact)
        assert len(nl.contacts_) == 1 and nl.matrix_free_
        c = nl.contacts_[0]
        assert c.consistent_tangent_ == (route == "consistent")
        xs, newton, gmres = _three_steps(nl)                            # (asserts that every step converges)
        assert c.HoldsConsistentRecord() == (route == "consistent") and not c.HoldsTangentBlocks()
        c.BoundaryPostTimeAdvance(nl.x)
        assert c.last_area_ > 0.0, "no contact: the comparison is void"
        routes[route] = (xs, newton, gmres)
        print(f"\ncontact penalty {FACADE_PENALTY:g} {route}: Newton iterations {newton}, GMRES iterations {gmres}")
    for x_c, x_f in zip(routes["consistent"][0], routes["frozen"][0]):
        assert np.abs(x_f).max() > 0
        assert np.allclose(x_c, x_f)
    assert routes["consistent"][1] < routes["frozen"][1]


def test_facade_consistent_at_the_default_penalty():
    """RigidPlane's own penalty 1e4, where the frozen tangent does not converge in the beam's 10 iterations: what the
    consistent one does is printed, and nothing but finite values is asserted"""
    from mimi_amd.integrators import RigidPlane
    from test_boundary_action_gpu import MATRIX_FREE, _beam

    def mark(nl):
        x = nl.patch().control_points
        y0, height = x[:, 1].min(), x[:, 1].max() - x[:, 1].min()
        lower = [a - 1 for a, f in nl._faces.items() if f == (1, 0)][0]
        nl.boundary_condition.current.contact(lower, RigidPlane([0.0, y0 + 0.01 * height], [0.0, 1.0]))

    nl = _beam(MATRIX_FREE + [("contact_consistent_tangent", 1)], mark)
    u = nl.solution_view("displacement", "x").ravel()
    for step in range(3):
        nl.step_time2()
        h = nl.newton_history[-1]
        print(f"  penalty 1e4 consistent step {step + 1}: Newton converged {h['converged']} after {h['iterations']} iterations, "
              f"|r| {h['norm']:.3e} of {h['norm0']:.3e}")
        assert np.isfinite(u).all() and np.isfinite(h["norm"])
