"""The friction reference (tests/_friction_reference.py) and the inputs of the friction tests (tests/_friction_cases.py),
without a GPU: (1) the cases give what tests/test_friction_gpu.py relies on -- enough eligible points, stick and slip at
u1, no point on the kink of the Coulomb cone or on the discontinuity of min(g, 0); (2) the reference's analytic tangent is
the derivative of its residual (central differences in long double, pressures / state / branch frozen); (3) closed forms on a
flat face pushed uniformly into a plane and slid along it; (4) the C ABI declares and exports the friction entries and its
version has not moved."""
import re
import os
import types

import numpy as np
import pytest

import _face_cases as fc
import _face_reference as fr
import _friction_cases as fx
import _friction_reference as fq

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mimi_hip_contact_set_friction", "mimi_hip_contact_set_body_increment", "mimi_hip_contact_post_time_advance",
           "mimi_hip_contact_reset_friction", "mimi_hip_contact_friction_history", "mimi_hip_contact_friction_state"]
FD_COLUMNS = 6           # columns of the tangent checked per face (spread over the face's dofs)


def every_face(case, order):
    return [(axis, side, kind) for axis, side in fc.faces(case) for kind in fx.KINDS]


@pytest.mark.parametrize("case,order", fx.CASES, ids=lambda c: str(c))
def test_cases_hold_what_the_gpu_test_relies_on(case, order):
    worst = dict(eligible=10 ** 9, share_lo=1.0, share_hi=0.0, kink=np.inf, gap=np.inf, margin=np.inf)
    for axis, side, kind in every_face(case, order):
        ref, size = fx.reference(case, axis, side, order, kind), fx.sizing(case, axis, side, order, kind)
        assert size.n_eligible >= 4, (axis, side, kind, size.n_eligible)
        tr1 = ref.ev1.tr
        assert int(tr1.on.sum()) == size.n_eligible
        share = ref.ev1.n_stick / size.n_eligible
        for ev in (ref.ev1, ref.ev2):
            if ev.tr.on.any():
                worst["kink"] = min(worst["kink"], float(np.abs(ev.tr.ratio[ev.tr.on] - 1).min()))
        for c in ref.contact:
            worst["gap"] = min(worst["gap"], float(np.abs(c.g).min()) / ref.extent)
        worst["eligible"] = min(worst["eligible"], size.n_eligible)
        worst["share_lo"], worst["share_hi"] = min(worst["share_lo"], share), max(worst["share_hi"], share)
        worst["margin"] = min(worst["margin"], size.margin)
        assert ref.ev0.n_stick == ref.ev0.n_slip == 0 and not np.any(ref.ev0.r)      # contact new in the step: no traction
    print(f"figures friction cases {case} order {order}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert 0.25 <= worst["share_lo"] and worst["share_hi"] <= 0.75
    assert worst["kink"] > 1e-6
    assert worst["gap"] > 1e-9


@pytest.mark.parametrize("case,order", fx.CASES, ids=lambda c: str(c))
def test_reference_tangent_is_the_derivative_of_its_residual(case, order):
    """central differences of the reference residual in long double, with p_A, the state, d and the branch frozen, on
    FD_COLUMNS columns per face and kind, at u2 (stick, slip, a body increment and a non-zero elastic slip).  The step is
    1e-7 extents: the slip direction s / |s| has |s| of about 1e-3 extents, so the truncation error of the quotient,
    (h / |s|)^2, is 1e-8 at that step and its rounding error, 1e-19 / 1e-7, far below"""
    B = fc.product_patch(case)
    dim = B.dim
    x2 = B.control_points.astype(LD) + fx.displacements(case)[2].reshape(-1, dim).astype(LD)
    worst = 0.0
    for axis, side, kind in every_face(case, order):
        ref = fx.reference(case, axis, side, order, kind)
        fb, ev = ref.pts[2].fb, ref.ev2
        ph = fq.point_pressure(ref.pts[2], ref.contact[2])
        K = fq.tangent(ref.pts[2], ev.tr, fx.MU, ref.eps_t)
        vd = (ref.nodes[:, None] * dim + np.arange(dim)).ravel()
        h = LD(1e-7) * LD(ref.extent)
        for col in vd[np.linspace(0, len(vd) - 1, FD_COLUMNS).astype(int)]:
            rs = []
            for sgn in (1, -1):
                x = x2.copy()
                x[col // dim, col % dim] += sgn * h
                pts = fr.face_points(fb, x)
                rs.append(fq.residual(pts, fq.tractions(pts, ph, ref.ev1.trial, fx.MU, ref.eps_t, ref.d, branch=ev.tr.branch)))
            fd = (rs[0] - rs[1]) / (2 * h)
            worst = max(worst, float(np.abs(fd - K[:, col]).max() / np.abs(K).max()))
    print(f"figures friction tangent against central differences {case} order {order}: {worst:.2e}")
    assert worst <= 1e-8


def flat_face(depth, eps, order=-1):
    """the face xi_1 = 0 of the block of block2d_p4 pushed `depth` into the plane y = depth: p_N = eps depth everywhere"""
    B = fc.product_patch("block2d_p4")
    fb = fr.face_basis(B.degrees, B.knots, 1, 0, order)
    X = B.control_points.astype(LD)
    body = dict(kind="plane", point=[0.0, depth], normal=[0.0, 1.0])
    return B, fb, X, body


@pytest.mark.parametrize("delta,branch", [(1.0e-4, "stick"), (5.0e-3, "slip")])
def test_closed_forms_on_a_flat_face(delta, branch):
    depth, eps, eps_t, mu = 1.0e-3, 1.0e4, 2.0e4, 0.3
    B, fb, X, body = flat_face(depth, eps)
    assert np.allclose(X[fr.face_node_ids(B.n_ctrl, 1, 0), 1].astype(float), 0.0)
    p0 = fr.face_points(fb, X)
    area = float(p0.da.sum())
    ev0 = fq.evaluate(p0, fr.mortar_contact(p0, body, eps, with_tangent=False), fq.initial_state(len(p0.x), 2), mu, eps_t,
                      with_tangent=False)
    assert ev0.trial.c.all() and not np.any(ev0.r)
    shift = np.zeros_like(X)
    shift[:, 0] = delta
    p1 = fr.face_points(fb, X + shift)
    ev1 = fq.evaluate(p1, fr.mortar_contact(p1, body, eps, with_tangent=False), ev0.trial, mu, eps_t, with_tangent=False)
    expected = eps_t * delta * area if branch == "stick" else mu * eps * depth * area
    assert (ev1.n_stick, ev1.n_slip) == ((len(p1.x), 0) if branch == "stick" else (0, len(p1.x)))
    assert abs(float(ev1.force[0]) - expected) <= 1e-15 * expected and abs(float(ev1.force[1])) <= 1e-15 * expected
    assert abs(float(ev1.traction) - expected) <= 1e-15 * expected
    assert np.all(np.einsum("qi,qi->q", ev1.tr.t, p1.x - p0.x) >= 0)                     # dissipation
    # the body moving along instead of the block: no slip, no traction
    ev_d = fq.evaluate(p1, fr.mortar_contact(p1, body, eps, with_tangent=False), ev0.trial, mu, eps_t, d=[delta, 0.0],
                       with_tangent=False)
    # (x_q - xbar - d cancels to the rounding of coordinates of size |X|: a few long-double units of it, times eps_T)
    assert float(np.abs(ev_d.tr.t).max()) <= 16 * float(np.finfo(LD).eps) * float(np.abs(X).max()) * eps_t


def test_dissipation_is_not_negative_at_any_point_of_the_cases():
    for case, order in fx.CASES[:2]:
        for axis, side, kind in every_face(case, order):
            ref = fx.reference(case, axis, side, order, kind)
            dx = ref.pts[1].x - ref.pts[0].x                                             # xi = 0, d = 0: a = x_q - xbar
            assert np.all(np.einsum("qi,qi->q", ref.ev1.tr.t, dx) >= 0)


def test_abi_declares_and_exports_the_friction_entries():
    import ctypes

    from mimi_amd import _capi, build
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mimi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mimi_hip_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(build.build())
    for entry in ENTRIES:
        assert entry in declared and entry in _capi.EXPORTS and hasattr(lib, entry), entry
    assert sorted(_capi.EXPORTS) == sorted(declared)
    lib.mimi_hip_abi_version.restype = ctypes.c_int
    assert lib.mimi_hip_abi_version() == 12
    assert "MIMI_HIP_ABI_VERSION 12" in open(os.path.join(ROOT, "include", "mimi_hip.h")).read()
    # no new field in the tables of a contact handle
    assert [f[0] for f in _capi.ContactTables._fields_][-1] == "spline"


def test_bodies_carry_friction_and_default_to_none():
    from mimi_amd.integrators import NearestDistanceToSplines, RigidPlane, RigidSphere, RigidSpline
    bodies = [RigidSphere([0, 0], 1.0, 5.0e3), RigidPlane([0, 0], [0, 1], 5.0e3),
              RigidSpline([1], [[0, 0, 1, 1]], [[0, 0], [1, 0]], coefficient=5.0e3), NearestDistanceToSplines()]
    for b in bodies:
        assert b.friction == 0.0 and b.step_displacement is None
        assert b.tangential_coefficient == b.coefficient
        b.friction, b.step_displacement = 0.3, [0.1, 0.0]
        assert b.friction == 0.3 and list(b.step_displacement) == [0.1, 0.0]
        b.tangential_coefficient = 2.0e4
        assert b.tangential_coefficient == 2.0e4
    assert RigidPlane([0, 0], [0, 1], friction=0.2, tangential_coefficient=7.0, step_displacement=[1, 2]).friction == 0.2


def test_the_facade_refuses_friction_with_matrix_free_boundary():
    """resolved before any device work: a contact body with friction and the matrix-free boundary actions do not combine;
    friction = 0 on the same body resolves as before"""
    from _explicit_cases import facade
    from mimi_amd import solid
    from mimi_amd.integrators import RigidPlane
    plane = RigidPlane([0.0, 0.0, 2.0], [0.0, 0.0, -1.0], friction=0.3)

    def configure(bc):
        for c in range(3):
            bc.initial.dirichlet(0, c)
        bc.current.contact(1, plane)
    flags = ("use_iterative_solver", "use_kronecker_preconditioner", "matrix_free", "matrix_free_boundary")
    nl = facade("cube_p2", "neohook", flags=tuple((k, 1) for k in flags), configure=configure, setup=False)
    with pytest.raises(RuntimeError, match="friction"):
        solid.resolve_route(nl.runtime_communication, nl.boundary_condition, [])
    with pytest.raises(RuntimeError, match="friction"):
        nl.setup(1)
    plane.friction = 0.0
    assert solid.resolve_route(nl.runtime_communication, nl.boundary_condition, []).boundary_actions


def test_sharded_contact_refuses_a_body_with_friction():
    from mimi_amd.integrators import RigidPlane
    from mimi_amd.parallel import ShardedContact
    with pytest.raises(RuntimeError, match="friction"):
        ShardedContact(None, RigidPlane([0.0, 0.0], [0.0, 1.0], friction=0.3), None, 1, 0)
