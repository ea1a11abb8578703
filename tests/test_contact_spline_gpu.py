"""The rigid spline body of MortarContact on the device (csrc/contact.hip: contact_gap_area_kernel -> sb_nearest of
csrc/spline_body.hpp) against what does not pass through this project's own restatement of the search:

  (a) nodal area / gap / pressure and GapNorm against tests/_closest_point.py (long double, brute-force global closest
      point) -- no oracle in the loop;
  (b) a spline that IS a circle / sphere / plane against the analytic body, residual and exact tangent, on the device;
  (c) the moved body (NearestDistanceToSplines.plant_kd_tree -> UpdateBody), bit for bit against a fresh handle;
  (d) faces other than (last axis, side 1) through the contact kernels, against the oracle.

Bodies, blocks and bounds: tests/_spline_bodies.py (10 x a difference measured on the CPU with the oracle, floored at
1e-13, capped at 1e-10; each measured value stands there beside its case)."""
import types

import numpy as np
import pytest

import _closest_point as cp
import _spline_bodies as sb
from _cases import synthetic_u

pytestmark = pytest.mark.gpu


def device_contact(P, n_el, p, axis, side, body):
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, MortarContact
    rowptr, col = P.sparsity()
    patch = mimi_amd.BSplinePatch.block(n_el, p)
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), rowptr[-1])
    return MortarContact(body, "contact", pattern, patch, axis, side).Prepare(), rowptr


def product_body(body, coefficient=1e4):
    from mimi_amd.integrators import RigidPlane, RigidSphere, RigidSpline
    if body["kind"] == "sphere":
        return RigidSphere(body["center"], body["radius"], coefficient)
    if body["kind"] == "plane":
        return RigidPlane(body["point"], body["normal"], coefficient)
    return RigidSpline(body["degrees"], body["knots"], body["control_points"], body["weights"], resolution=body["resolution"],
                       coefficient=coefficient)


# ---- (a) nodal sums against the long-double reference -----------------------------------------------------------------
@pytest.mark.parametrize("case", sb.CASES, ids=sb.CASE_IDS)
def test_spline_body_nodal_sums_against_reference_gpu(case):
    block, name = case
    (n_el, p, axis), cid = block, sb.CASE_IDS[sb.CASES.index(case)]
    P, patch, tables, u, body = sb.setup(block, name)
    B, ref = sb.reference(block, name)
    cp.check_conditions(ref, B, clipping=name in sb.CLIPPING)
    G, rowptr = device_contact(P, n_el, p, axis, 1, product_body(body))
    assert np.array_equal(G.MarkedNodes(), ref.nodes)
    G.GapArea(u)
    area, gap = np.zeros(len(ref.nodes)), np.zeros(len(ref.nodes))
    G.GetNodal(area, gap)
    r = np.zeros(P.n_vdofs)
    G.AddBoundaryResidual(u, r)
    errs = (sb.rel(area, ref.area), sb.rel(gap, ref.gap), sb.rel(G.AveragePressure(), ref.pressure),
            sb.rel(G.GapNorm(u), ref.gap_norm))
    print(cid, "area, gap, pressure, GapNorm:", errs, "bound", sb.bound(sb.MEASURED_NODAL[cid]))
    assert np.abs(r).max() > 0
    assert max(errs) < sb.bound(sb.MEASURED_NODAL[cid])


# ---- (b) spline body == analytic body, on the device -------------------------------------------------------------------
TWINS = [(c, cid) for c, cid in zip(sb.CASES, sb.CASE_IDS) if cid in sb.MEASURED_TWIN and "open-arc" not in cid]


@pytest.mark.parametrize("case", [c for c, _ in TWINS], ids=[cid for _, cid in TWINS])
def test_spline_body_equals_analytic_body_gpu(case):
    block, name = case
    (n_el, p, axis), cid = block, sb.CASE_IDS[sb.CASES.index(case)]
    P, patch, tables, u, body = sb.setup(block, name)
    out = []
    for b in (body, body["twin"]):
        G, rowptr = device_contact(P, n_el, p, axis, 1, product_body(b))
        r, A = np.zeros(P.n_vdofs), np.zeros(rowptr[-1])
        G.AddBoundaryResidualAndGrad(u, 0.6, r, A)
        out.append((r, A))
    assert np.abs(out[1][0]).max() > 0 and np.abs(out[1][1]).max() > 0
    errs = (sb.rel(out[0][0], out[1][0]), sb.rel(out[0][1], out[1][1]))
    print(cid, "residual, tangent against the analytic body:", errs, "bound", sb.bound(sb.MEASURED_TWIN[cid]))
    assert max(errs) < sb.bound(sb.MEASURED_TWIN[cid])


# ---- (c) the moved body --------------------------------------------------------------------------------------------------
def _scene(body, resolution):
    from mimi_amd.integrators import NearestDistanceToSplines
    spline = types.SimpleNamespace(degrees=body["degrees"], knot_vectors=body["knots"],
                                   control_points=np.array(body["control_points"], dtype=float), weights=body["weights"])
    scene = NearestDistanceToSplines()
    scene.add_spline(spline)
    scene.plant_kd_tree(resolution, 1)
    return scene, spline


def _evaluate(G, u, r0, A0):
    r, A = r0.copy(), A0.copy()
    G.AddBoundaryResidualAndGrad(u, 0.6, r, A)
    G.BoundaryPostTimeAdvance(u)
    return r, A, G.AveragePressure().copy(), G.GapNorm(u), np.array(G.last_force_)


@pytest.mark.parametrize("block,name", [(sb.BLOCKS_2D[0], "circle-seam-down"), (sb.BLOCKS_3D[0], "dome")])
def test_moved_spline_body_gpu(block, name):
    n_el, p, axis = block
    P, patch, tables, u, body = sb.setup(block, name)
    rng = np.random.default_rng(8)
    scene, spline = _scene(body, body["resolution"])
    G, rowptr = device_contact(P, n_el, p, axis, 1, scene)
    r0, A0 = rng.standard_normal(P.n_vdofs), rng.standard_normal(rowptr[-1])
    unmoved = _evaluate(G, u, r0, A0)
    assert np.abs(unmoved[0] - r0).max() > 0 and unmoved[2].min() < 0
    # translate the control points (sideways and a little deeper) and re-plant: the handle must hold the moved body
    shift = np.zeros(P.dim)
    shift[0], shift[axis] = 0.37, -0.011
    spline.control_points += shift
    scene.plant_kd_tree(body["resolution"], 1)
    moved = _evaluate(G, u, r0, A0)
    fresh_scene, _ = _scene(dict(body, control_points=spline.control_points), body["resolution"])
    fresh_handle, _ = device_contact(P, n_el, p, axis, 1, fresh_scene)
    fresh = _evaluate(fresh_handle, u, r0, A0)
    for a, b in zip(moved, fresh):
        assert np.array_equal(a, b)                                   # the same bits
    assert np.abs(moved[0] - unmoved[0]).max() > 1e-3 * np.abs(unmoved[0] - r0).max()
    assert np.abs(moved[2] - unmoved[2]).max() > 1e-3 * np.abs(unmoved[2]).max() and moved[3] != unmoved[3]
    # the coefficient is read at every evaluation: the pressures scale by the ratio (one rounding each)
    scene.coefficient = 2.5e4
    stiffer = _evaluate(G, u, r0, A0)
    assert np.allclose(stiffer[2], 2.5 * moved[2], rtol=1e-15, atol=0.0) and np.abs(moved[2]).max() > 0
    assert stiffer[3] == moved[3]
    # out of reach: r and A come back untouched, bit for bit, and nothing of the previous call survives
    spline.control_points[:, axis] += 10.0
    scene.plant_kd_tree(body["resolution"], 1)
    away = _evaluate(G, u, r0, A0)
    assert np.array_equal(away[0], r0) and np.array_equal(away[1], A0)
    assert np.all(away[2] == 0.0) and away[3] == 0.0 and np.all(away[4] == 0.0)
    r = r0.copy()
    G.AddBoundaryResidual(u, r)
    assert np.array_equal(r, r0)


# ---- (d) other faces through the contact kernels ------------------------------------------------------------------------
FACES = [((6, 3), 2, 0, 1), ((6, 3), 2, 0, 0), ((4, 4, 2), 2, 1, 0), ((4, 4, 2), 2, 0, 1)]


def _body_outside(P, axis, side, kind):
    """sphere_over_top / the plane of test_contact_parity_gpu, on the outward side of the face (axis, side)"""
    L = P.ctrl.max(axis=0)
    out = np.zeros(P.dim)
    out[axis] = 1.0 if side == 1 else -1.0
    face = 0.5 * L
    face[axis] = L[axis] if side == 1 else 0.0
    if kind == "sphere":
        R = 0.25 * max(L[d] for d in range(P.dim) if d != axis)
        return dict(kind="sphere", center=list(face + 0.9 * R * out), radius=float(R))
    return dict(kind="plane", point=list(face - 0.03 * out), normal=list(-out))


@pytest.mark.parametrize("n_el,p,axis,side", FACES)
@pytest.mark.parametrize("bodykind", ["sphere", "plane"])
def test_contact_parity_on_other_faces_gpu(n_el, p, axis, side, bodykind):
    """test_contact_parity_gpu (tests/test_contact.py) only ever marks (last axis, side 1): the same comparison, at the
    same tolerances, on faces whose tangent order and orientation differ"""
    from oracle import iga, ref_path as rp
    P = iga.Patch.block(n_el, p)
    rowptr, col = P.sparsity()
    body = _body_outside(P, axis, side, bodykind)
    Cn = rp.ContactOracle(P, axis, side, body, penalty=1e4, rowptr=rowptr, col=col)
    G, _ = device_contact(P, n_el, p, axis, side, product_body(body))
    u = synthetic_u(P, scale=0.01)
    r0 = np.random.default_rng(5).standard_normal(P.n_vdofs)
    A0 = np.random.default_rng(6).standard_normal(rowptr[-1])

    def rel(a, b):
        return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)

    r_o, r_g = r0.copy(), r0.copy()
    Cn.add_boundary_residual(u, r_o)
    G.AddBoundaryResidual(u, r_g)
    assert np.abs(r_o - r0).max() > 0 and Cn.pressure.min() < 0
    assert Cn.last_force[axis] * (1.0 if side == 1 else -1.0) < 0            # the body pushes the face inwards
    assert np.array_equal(G.MarkedNodes(), Cn.marked_nodes)
    assert rel(r_g - r0, r_o - r0) < 1e-12
    assert np.allclose(G.AveragePressure(), Cn.pressure, rtol=1e-12, atol=1e-12)
    G.BoundaryPostTimeAdvance(u)
    assert np.isclose(G.last_area_, Cn.last_area, rtol=1e-13)
    assert np.allclose(G.last_force_, Cn.last_force, rtol=1e-11, atol=1e-12)
    assert np.isclose(G.last_pressure_, Cn.last_pressure, rtol=1e-11)
    assert np.isclose(G.GapNorm(u), Cn.gap_norm(u), rtol=1e-12)
    for mode, tol in ((rp.TANGENT_EXACT, 1e-11), (rp.TANGENT_FD, 1e-4)):
        G.SetTangentMode(0 if mode == rp.TANGENT_EXACT else 1)
        r_o, r_g, A_o, A_g = r0.copy(), r0.copy(), A0.copy(), A0.copy()
        Cn.add_boundary_residual_and_grad(u, 0.6, r_o, A_o, mode)
        G.AddBoundaryResidualAndGrad(u, 0.6, r_g, A_g)
        assert np.abs(A_o - A0).max() > 0
        assert rel(r_g - r0, r_o - r0) < 1e-12
        assert rel(A_g - A0, A_o - A0) < tol
