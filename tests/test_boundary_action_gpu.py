"""The matrix-free action of the contact and follower-pressure tangents (csrc/kernels_face_action.hpp) through the C ABI:
MortarContact / FollowerPressure .Linearize / .ApplyTangent, LinearSolver.AddBoundaryOperator and the facade's
"matrix_free_boundary" flag.

(1) the action on every face of the cases of tests/test_faces_gpu.py (two vectors per face) against the long-double
    reference's K v, within the bar the assembled blocks are held to (_face_cases.TOL pressure_K 1e-12, contact_K 1e-11) on
    the scale without cancellation, max_i (|K| |v|)_i;
(2) against the handle's own assembled tangent, within the same bars: the cases of (1) at the default order, the rigid spline
    bodies of tests/test_contact_spline_gpu.py and element slabs of a 3-D face across repeated knots;
(3) semantics: equal bytes, accumulation, host and device arguments, the refusal, the snapshot, an inactive handle, the bytes
    of record;
(4) GMRES with the Kronecker preconditioner on rho M + fac0 K plus a contact and a pressure term: the iteration count of the
    restated GMRES on the device-assembled matrix, the solution of the extended-precision solve; the rules of the seam;
(5) the facade: a beam pressed onto a rigid plane and a beam under follower pressure, matrix-free against assembled.

Worst figures measured on an MI355X: (1) pressure 3.5e-15, contact 4.8e-14 (one point per face, where the nodal pressure's own
error shows, as in tests/test_faces_gpu.py); (2) 6.6e-16, spline bodies 1.6e-16, slabs 5.8e-16; (4) 48 iterations, the
restatement's, x 1.4e-8 from the extended-precision solve (bar 5.6e-7), 2.1 away without the two terms; (5) pressure: 7 Newton
and 107 GMRES iterations on both routes; contact: 27 Newton and 399 GMRES iterations on both routes."""
import numpy as np
import pytest
import scipy.sparse as sp

import _face_cases as fc
import _kronecker_cases as kc
import _kronecker_reference as ref
import _patches
import _spline_bodies as sb
from _cases import product_material
from test_boundary_action_cpu import ALL, CONTACT_KINDS, PRESSURE_KINDS, reference_products, vectors

pytestmark = pytest.mark.gpu
T = fc.TOL


def pattern_of(case):
    from test_faces_gpu import pattern_of as cached
    return cached(case)[0]


def dense(pattern, values):
    n = len(pattern.rowptr) - 1
    return sp.csr_matrix((values, pattern.col, pattern.rowptr), shape=(n, n))


def pressure_handle(case, axis, side, order, pressure, **kw):
    from mimi_amd.integrators import FollowerPressure
    fp = FollowerPressure("pressure", pattern_of(case), fc.product_patch(case), axis, side, quadrature_order=order, **kw).Prepare()
    fp.SetPressure(pressure)
    return fp


def contact_handle(case, axis, side, order, kind, **kw):
    from test_faces_gpu import contact_handle as make
    return make(case, axis, side, order, kind, **kw)


def action(G, v, factor=1.0):
    """the increment of ApplyTangent in accumulate form on a random y0"""
    y0 = np.random.default_rng(11).standard_normal(len(v))
    y = y0.copy()
    G.ApplyTangent(np.array(v), y, factor)
    return y - y0


def deviation(got, Kv, scale):
    """max |got - K v| over max_i (|K| |v|)_i"""
    return float(np.abs(got - Kv).max() / scale.max())


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,order", ALL, ids=lambda c: str(c))
def test_pressure_action_against_the_reference(case, order):
    u = fc.displacement(case)
    worst = 0.0
    for axis, side in fc.faces(case):
        for kind in PRESSURE_KINDS:
            r = fc.pressure_reference(case, axis, side, order, kind)
            fp = pressure_handle(case, axis, side, order, r.pressure)
            fp.Linearize(u)
            Kv, scale = reference_products(r.K, vectors(case, axis, side))
            for k, v in enumerate(vectors(case, axis, side)):
                worst = max(worst, deviation(action(fp, v), Kv[k], scale[k]))
            assert not fp.HoldsTangentBlocks()
    print(f"figures pressure action {case} order {order}: K={worst:.2e}")
    assert worst <= T["pressure_K"]


@pytest.mark.parametrize("kind", CONTACT_KINDS)
@pytest.mark.parametrize("case,order", ALL + fc.ORDERS_CONTACT, ids=lambda c: str(c))
def test_contact_action_against_the_reference(case, order, kind):
    u = fc.displacement(case)
    worst = 0.0
    for axis, side in fc.faces(case):
        r = fc.contact_reference(case, axis, side, order, kind)          # (its K carries GRAD_FACTOR)
        G = contact_handle(case, axis, side, order, kind)
        G.Linearize(u)
        Kv, scale = reference_products(r.K, vectors(case, axis, side))
        for k, v in enumerate(vectors(case, axis, side)):
            worst = max(worst, deviation(action(G, v, fc.GRAD_FACTOR), Kv[k], scale[k]))
        assert not G.HoldsTangentBlocks()
    print(f"figures contact action {case} order {order} {kind}: K={worst:.2e}")
    assert worst <= T["contact_K"]


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
def against_assembly(G, pattern, u, vs, factor):
    """worst deviation of the action from (the handle's own assembled tangent) v, on the scale |K| |v|"""
    n = len(pattern.rowptr) - 1
    A = np.zeros(pattern.nnz)
    G.AddBoundaryResidualAndGrad(np.array(u), factor, np.zeros(n), A)
    K = dense(pattern, A)
    assert np.abs(A).max() > 0
    G.Linearize(np.array(u))
    worst = 0.0
    for v in vs:
        worst = max(worst, deviation(action(G, v, factor), K @ v, abs(K) @ np.abs(v)))
    return worst


@pytest.mark.parametrize("case", list(_patches.CASES) + fc.BLOCKS)
def test_actions_against_the_assembled_tangents(case):
    u = fc.displacement(case)
    worst = dict(pressure=0.0, contact=0.0)
    for axis, side in fc.faces(case):
        vs = vectors(case, axis, side)
        fp = pressure_handle(case, axis, side, -1, fc.pressure_reference(case, axis, side, -1, "nodal").pressure)
        worst["pressure"] = max(worst["pressure"], against_assembly(fp, pattern_of(case), u, vs, 1.0))
        G = contact_handle(case, axis, side, -1, "sphere")
        worst["contact"] = max(worst["contact"], against_assembly(G, pattern_of(case), u, vs, fc.GRAD_FACTOR))
    print(f"figures action against assembly {case}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["pressure"] <= T["pressure_K"] and worst["contact"] <= T["contact_K"]


@pytest.mark.parametrize("block,name", [(sb.BLOCKS_2D[0], "circle-seam-down"), (sb.BLOCKS_3D[0], "dome")])
def test_contact_action_with_a_rigid_spline_body(block, name):
    from mimi_amd.integrators import CSRPattern
    from test_contact_spline_gpu import device_contact, product_body
    n_el, p, axis = block
    P, patch, tables, u, body = sb.setup(block, name)
    G, rowptr = device_contact(P, n_el, p, axis, 1, product_body(body))
    _, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), rowptr[-1])
    vs = np.random.default_rng(21).standard_normal((2, P.n_vdofs))
    worst = against_assembly(G, pattern, u, vs, 0.6)
    print(f"figures contact action spline body {name}: K={worst:.2e}")
    assert worst <= T["contact_K"]


def test_actions_of_3d_slabs_across_repeated_knots():
    from test_faces_gpu import slab_boxes
    case, axis, cut_axis = "rep3d_p2", 2, 0
    B, u = fc.product_patch(case), fc.displacement(case)
    vs = vectors(case, axis, 1)
    r = fc.pressure_reference(case, axis, 1, -1, "nodal")
    total = np.zeros(vs.shape)
    worst = dict(pressure=0.0, contact=0.0)
    for box in slab_boxes(B, cut_axis):
        part = pressure_handle(case, axis, 1, -1, 1.0, element_box=box)
        part.SetPressure(r.pressure[np.searchsorted(r.nodes, part.FaceNodes())])
        worst["pressure"] = max(worst["pressure"], against_assembly(part, pattern_of(case), u, vs, 1.0))
        total += np.array([action(part, v) for v in vs])
        G = contact_handle(case, axis, 1, -1, "sphere", element_box=box)
        worst["contact"] = max(worst["contact"], against_assembly(G, pattern_of(case), u, vs, fc.GRAD_FACTOR))
    Kv, scale = reference_products(r.K, vs)
    whole = max(deviation(total[k], Kv[k], scale[k]) for k in range(len(vs)))
    print(f"figures slab actions {case}: against assembly pressure {worst['pressure']:.2e} contact {worst['contact']:.2e}, "
          f"pressure slabs summed against the reference {whole:.2e}")
    assert worst["pressure"] <= T["pressure_K"] and worst["contact"] <= T["contact_K"] and whole <= T["pressure_K"]


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
SEMANTICS = [("rep3d_p2", 2, 1), ("rep2d_p3", 1, 0)]


@pytest.mark.parametrize("case,axis,side", SEMANTICS)
@pytest.mark.parametrize("which", ["pressure", "contact"])
def test_semantics_of_the_action(which, case, axis, side):
    import torch
    from mimi_amd.integrators import RigidPlane
    B, u = fc.product_patch(case), np.array(fc.displacement(case))
    v = np.array(vectors(case, axis, side)[0])
    if which == "pressure":
        r = fc.pressure_reference(case, axis, side, -1, "nodal")
        G = pressure_handle(case, axis, side, -1, r.pressure)
        n_faces = G.n_faces_
    else:
        G = contact_handle(case, axis, side, -1, "plane")
        n_faces = G.n_marked_boundaries_
    n_q = fc.face_basis(case, axis, side).n_q_face
    assert G.LinearizationBytes() == 0
    with pytest.raises(RuntimeError, match="before any mimi_hip_(contact|follower)_linearize"):
        G.ApplyTangent(v, np.zeros_like(v))
    G.Linearize(u)
    y0 = np.random.default_rng(3).standard_normal(len(v))
    runs = []
    for _ in range(2):
        y = y0.copy()
        G.ApplyTangent(v, y, 0.7)
        runs.append(y)
    assert np.array_equal(runs[0], runs[1]) and np.abs(runs[0] - y0).max() > 0
    # accumulation: what a zero y gets is the increment (one addition per entry, off the face none)
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
    y = y0.copy()
    G.ApplyTangent(v, y, 0.7)
    assert np.array_equal(y, runs[0])
    # the snapshot survives whatever else the handle does
    other = 1.7 * u
    G.AddBoundaryResidual(other, np.zeros_like(v))
    if which == "pressure":
        G.SetPressure(-2.0)
        G.AddBoundaryResidual(other, np.zeros_like(v))
    else:
        G.UpdateBody(penalty=3.0 * fc.PENALTY)
        G.GapNorm(other)
        G.AddBoundaryResidual(other, np.zeros_like(v))
    y = y0.copy()
    G.ApplyTangent(v, y, 0.7)
    assert np.array_equal(y, runs[0])
    # ... and a new linearisation reads the handle as it is now
    G.Linearize(u)
    y = y0.copy()
    G.ApplyTangent(v, y, 0.7)
    assert not np.array_equal(y, runs[0])
    expect = n_faces * n_q * (1 + (B.dim - 1) * B.dim) * 8 + n_faces
    assert G.LinearizationBytes() == expect and not G.HoldsTangentBlocks()
    # nothing active: y keeps its bits
    if which == "pressure":
        G.SetPressure(0.0)
    else:
        pts = fc.points(case, axis, side).x.astype(np.float64)
        far = pts.min(axis=0) - 100.0
        normal = np.zeros(B.dim)
        normal[0] = 1.0
        G = far_contact_handle(case, axis, side, RigidPlane(list(far), list(normal), fc.PENALTY))
    G.Linearize(u)
    y = y0.copy()
    G.ApplyTangent(v, y, 0.7)
    assert np.array_equal(y, y0)


def far_contact_handle(case, axis, side, body):
    from mimi_amd.integrators import MortarContact
    return MortarContact(body, "contact", pattern_of(case), fc.product_patch(case), axis, side).Prepare()


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
def _boundary_system(name, fac0):
    """test_matrix_free_gpu.py::_operator_system with a contact face (axis 2, side 1, a plane through the deformed face's
    mean height) and a pressure face (axis 1, side 1): (domain, contact, pressure, solver, J, values, patch, ess, u, b)"""
    from mimi_amd.integrators import CSRPattern, FollowerPressure, MortarContact, NonlinearSolid, RigidPlane
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
    plane = RigidPlane([0.0, 0.0, float(x[top, 2].mean())], [0.0, 0.0, -1.0], 1e4)
    contact = MortarContact(plane, "contact", pattern, B, 2, 1).Prepare()
    pressure = FollowerPressure("pressure", pattern, B, 1, 1).Prepare()
    pressure.SetPressure(25.0)
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    G.AddDomainResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    before = vals.copy()
    contact.AddBoundaryResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    contact.BoundaryPostTimeAdvance(u)
    nodal = contact.AveragePressure()
    assert contact.last_area_ > 0 and np.abs(vals - before).max() > 0 and np.any(nodal == 0.0) and np.any(nodal != 0.0)
    before = vals.copy()
    pressure.AddBoundaryResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    assert np.abs(vals - before).max() > 0
    S = _kronecker_solver(pattern, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))
    S.Eliminate(None, vals)
    J = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs))
    return G, contact, pressure, S, J, vals, P, ess, u, b


def test_gmres_with_the_boundary_terms():
    name, fac0 = "p2_6x4x2", 1e-2
    G, contact, pressure, S, J, vals, P, ess, u, b = _boundary_system(name, fac0)
    S.max_iter = 3000
    restated = ref.gmres(J, b, ref.dense_preconditioner(P, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0)), max_iter=3000)
    assert restated.converged and ref.margin(restated) >= kc.MARGIN
    nan = lambda: np.full(len(b), np.nan)
    S.preconditioner = "kronecker"
    # the rules of the seam
    with pytest.raises(RuntimeError, match="no domain operator is set"):
        S.AddBoundaryOperator(contact, fac0)
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(u)
    other = contact_handle("rep3d_p2", 2, 1, -1, "plane")
    with pytest.raises(RuntimeError, match="dofs"):
        S.AddBoundaryOperator(other, fac0)
    S.AddBoundaryOperator(contact, fac0)
    with pytest.raises(RuntimeError, match="before any mimi_hip_contact_linearize"):
        S.Mult(None, b, nan())
    contact.Linearize(u)
    pressure.Linearize(u)
    for _ in range(7):
        S.AddBoundaryOperator(pressure, 0.0)
    with pytest.raises(RuntimeError, match="at most 8"):
        S.AddBoundaryOperator(pressure, fac0)
    # domain alone, then domain and both faces: the second is the system
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    x_domain = S.Mult(None, b, nan())
    S.AddBoundaryOperator(contact, fac0)
    S.AddBoundaryOperator(pressure, fac0)
    x = S.Mult(None, b, nan())
    x_ref = np.array([float(v) for v in ref.solve_extended(J, b)])
    dev = np.abs(x - x_ref).max() / np.abs(x_ref).max()
    print(f"\n{name} fac0 {fac0:g} with a contact and a pressure term: iterations {S.final_iter_} (restatement "
          f"{restated.iterations}), x deviates {dev:.3g} (bar {kc.BAR * kc.DEV_SOLVE:.3g}); without the terms x is "
          f"{np.abs(x_domain - x_ref).max() / np.abs(x_ref).max():.3g} away")
    assert S.converged_ and np.isfinite(x).all()
    assert S.final_iter_ == restated.iterations
    assert dev <= kc.BAR * kc.DEV_SOLVE
    assert np.abs(x_domain - x_ref).max() > 1e3 * kc.BAR * kc.DEV_SOLVE * np.abs(x_ref).max()
    # with the values the CSR product runs as ever: the bits of a solver that never saw an operator
    from test_kronecker_gpu import _kronecker_solver
    _, B = kc.solve_patch(name)
    fresh = _kronecker_solver(S.pattern_, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))
    fresh.preconditioner, fresh.max_iter = "kronecker", 3000
    got = [(s.Mult(vals, b, nan()).tobytes(), s.final_iter_) for s in (S, fresh)]
    assert got[0] == got[1]
    # SetOperator drops the terms, ClearOperator too
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    assert np.array_equal(S.Mult(None, b, nan()), x_domain)
    S.AddBoundaryOperator(contact, fac0)
    S.ClearOperator()
    with pytest.raises(RuntimeError, match="no operator is set"):
        S.Mult(None, b, nan())
    with pytest.raises(RuntimeError, match="no domain operator is set"):
        S.AddBoundaryOperator(contact, fac0)


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
ASSEMBLED = [("use_iterative_solver", 1), ("use_kronecker_preconditioner", 1)]
MATRIX_FREE = ASSEMBLED + [("matrix_free", 1), ("matrix_free_boundary", 1)]


def _beam(runtime, mark):
    from test_nonlinear_solid import BEAM, GOLDEN_CASES, beam
    nl = beam("neohook", runtime=runtime, finish=False)
    mark(nl)
    nl.setup(1)
    nl.configure_newton(*BEAM["newton"])
    nl.time_step_size = GOLDEN_CASES["neohook"]["dt"]
    return nl


def _three_steps(nl):
    """(x after each step, Newton iterations, GMRES iterations); every linear solve must converge"""
    total = [0]
    mult = nl.linear_.Mult

    def counted(A, *args):
        assert (A is None) == nl.matrix_free_
        out = mult(A, *args)
        assert nl.linear_.converged_
        total[0] += nl.linear_.final_iter_
        return out
    nl.linear_.Mult = counted
    u = nl.solution_view("displacement", "x").ravel()
    xs, newton = [], 0
    for _ in range(3):
        nl.step_time2()
        h = nl.newton_history[-1]
        print(f"  step: Newton converged {h['converged']} after {h['iterations']} iterations, |r| {h['norm']:.3e} of {h['norm0']:.3e}")
        assert h["converged"]
        newton += h["iterations"]
        xs.append(u.copy())
    return xs, newton, total[0]


# The penalty of the facade's plane.  The contact tangent freezes the nodal pressure (mortar_contact.cpp:281-294), so on
# BOTH routes Newton is a fixed-point iteration in the pressure: it contracts only while the penalty stays small beside the
# beam's own stiffness (E = 2100 over a height of 1).  With RigidPlane's default 1e4 the assembled route -- the yardstick
# -- does not converge in the beam's 10 iterations (|r| 6e3 of 4e4 after step 3, iterates of size 1), and two runs that do
# not converge cannot be compared; at 1e2 it converges in 9 iterations per step.  That every step converges is asserted.
FACADE_PENALTY = 1.0e2


def _mark_contact(nl):
    from mimi_amd.integrators import RigidPlane
    x = nl.patch().control_points
    y0, height = x[:, 1].min(), x[:, 1].max() - x[:, 1].min()
    lower = [a - 1 for a, f in nl._faces.items() if f == (1, 0)][0]
    nl.boundary_condition.current.contact(lower, RigidPlane([0.0, y0 + 0.01 * height], [0.0, 1.0], FACADE_PENALTY))


def _mark_pressure(nl):
    nl.boundary_condition.initial.pressure(3, 1.0)


@pytest.mark.parametrize("load", ["contact", "pressure"])
def test_facade_matrix_free_against_assembled(load):
    mark = _mark_contact if load == "contact" else _mark_pressure
    routes = {}
    for route, flags in (("matrix-free", MATRIX_FREE), ("assembled", ASSEMBLED)):
        nl = _beam(flags, mark)
        faces = nl.contacts_ + nl.pressures_
        assert len(faces) == 1
        if route == "matrix-free":
            assert nl.matrix_free_ and not hasattr(nl, "d_jac_")
        else:
            assert not nl.matrix_free_ and hasattr(nl, "d_jac_")
        xs, newton, gmres = _three_steps(nl)
        if load == "contact":
            c = nl.contacts_[0]
            c.BoundaryPostTimeAdvance(nl.x)
            assert c.last_area_ > 0.0, "no contact: the comparison is void"
            assert np.abs(c.AveragePressure()).max() > 0.0
        if route == "matrix-free":
            assert not hasattr(nl, "d_jac_")
            assert all(not f.HoldsTangentBlocks() and f.LinearizationBytes() > 0 for f in faces)
        else:
            assert all(f.HoldsTangentBlocks() for f in faces)
        routes[route] = (xs, newton, gmres)
        print(f"\n{load} {route}: Newton iterations {newton}, GMRES iterations {gmres}")
    for x_mf, x_asm in zip(routes["matrix-free"][0], routes["assembled"][0]):
        assert np.abs(x_asm).max() > 0
        assert np.allclose(x_mf, x_asm)
    assert routes["matrix-free"][2] > 0


def test_facade_flag_rules():
    from test_nonlinear_solid import beam

    def prepared(runtime, mark=None):
        nl = beam("neohook", runtime=runtime, finish=False)
        if mark:
            mark(nl.boundary_condition)
        return nl

    with pytest.raises(RuntimeError, match="matrix_free_boundary needs matrix_free"):
        prepared(ASSEMBLED + [("matrix_free_boundary", 1)]).setup(1)
    with pytest.raises(RuntimeError, match="periodic"):
        prepared(MATRIX_FREE, lambda bc: bc.initial.periodic(1, 2)).setup(1)
    with pytest.raises(RuntimeError, match="use_kronecker_preconditioner"):
        prepared([("use_iterative_solver", 1), ("matrix_free", 1), ("matrix_free_boundary", 1)]).setup(1)
