"""Augmented-Lagrangian mortar contact without a GPU:
(1) closed forms of the long-double reference (tests/_augmented_reference.py) on a flat face parallel to a plane at offset
    delta: gt_i = -delta at every node (partition of unity), p_i = min(0, lambda - eps delta), total force |p| area n, release
    exactly when lambda + eps gt >= 0;
(2) with lambda = 0 and a body deep enough that every point penetrates the reference equals _face_reference.mortar_contact;
(3) the reference's consistent K against the central difference of its own residual, on the scale and step rule of
    tests/_contact_consistent_cases.py, within 10 x _augmented_cases.LD_WORST; the float64 quotient at the device test's step
    is printed beside the bar that test uses;
(4) the inputs of tests/test_augmented_gpu.py are what tests/_augmented_cases.py says they are;
(5) the flag rules of solid.resolve_route, the header and the export list;
(6) the stepping restatement (tests/_augmented_stepping.py): every Newton solve converges, the violation falls by the factors
    its docstring records, the first violation of the impact step is positive.

Figures measured: (3) long double worst 2.4e-12 over the (face, body) pairs of CASES (block2d_p4, face (1, 0), plane), float64 on FD_CASES
worst 1.0e-10 (rep2d_p3, sphere) of the device test's bar 9.5e-10."""
import os
import re

import numpy as np
import pytest

import _augmented_cases as ac
import _augmented_reference as ar
import _face_cases as fc
import _face_reference as fr
from test_boundary_action_cpu import vectors

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mimi_hip_contact_set_augmented", "mimi_hip_contact_lagrange", "mimi_hip_contact_update_lagrange")


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
def flat_face():
    """the lower edge y = 0 of the undeformed block2d_p4 and its length"""
    B = fc.product_patch("block2d_p4")
    pts = fr.face_points(fc.face_basis("block2d_p4", 1, 0), B.control_points.astype(LD))
    return pts, pts.da.sum()


@pytest.mark.parametrize("delta,lam,released", [(0.01, 0.0, False), (0.01, -3.0, False), (-0.005, -1.0, False), (-0.01, -1.0, True),
                                                (-0.02, -1.0, True), (-0.02, 0.0, True)])
def test_closed_forms_on_a_flat_face(delta, lam, released):
    eps = 100.0
    pts, length = flat_face()
    body = dict(kind="plane", point=[0.0, delta], normal=[0.0, 1.0])     # the half space y < delta: g = y - delta
    n = len(fr.face_node_ids(pts.fb.n_ctrl, 1, 0))
    out = ar.augmented_contact(pts, body, eps, np.full(n, lam))
    tiny = 1e-17
    assert np.abs(out.gt + LD(delta)).max() <= tiny
    p = min(0.0, lam - eps * delta)
    assert np.abs(out.pressure - LD(p)).max() <= 1e-15
    assert released == (lam + eps * -delta >= 0) and bool(np.all(out.pressure == 0)) == released and out.n_active == (0 if released else n)
    # total force on the body: sum_q w p m = p length n, n = (0, -1) the outward normal of the edge
    assert np.abs(out.last_force - LD(p) * length * np.array([0, -1], dtype=LD)).max() <= 1e-15
    assert abs(out.r.reshape(-1, 2)[:, 1].sum() - LD(p) * length) <= 1e-15 and np.abs(out.r.reshape(-1, 2)[:, 0]).max() <= tiny
    assert abs(out.violation - abs(p - lam) / eps) <= tiny and abs(out.norm - abs(p - lam) * np.sqrt(length)) <= 1e-15
    if released:
        assert not np.any(out.r) and not np.any(out.K)


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,axis,side", [("rep2d_p2", 1, 0), ("rep3d_p1", 2, 1)])
def test_zero_multipliers_and_full_penetration_are_the_penalty_law(case, axis, side):
    pts = fc.points(case, axis, side)
    b = fc.body(case, axis, side, -1, "plane")
    normal = np.asarray(b["normal"])
    depth = float(((pts.x.astype(np.float64) - np.asarray(b["point"])) @ normal).max())
    deep = dict(kind="plane", point=list(np.asarray(b["point"]) + (depth + 0.05) * normal), normal=b["normal"])
    pen = fr.mortar_contact(pts, deep, fc.PENALTY, fc.GRAD_FACTOR)
    assert np.all(pen.g < 0)
    aug = ar.augmented_contact(pts, deep, fc.PENALTY, np.zeros(len(pen.nodes)), fc.GRAD_FACTOR)
    for a, b_ in ((aug.pressure, pen.pressure), (aug.r, pen.r), (aug.K_frozen, pen.K), (aug.area, pen.area), (aug.gap, pen.gap),
                  (aug.dlambda, pen.pressure)):
        assert np.abs(a - b_).max() <= 1e-17 * max(float(np.abs(b_).max()), 1.0)      # (rounding of long double: 1e-19)
    assert aug.n_active == len(pen.nodes)


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
def quotient(case, axis, side, order, kind, v, h, dtype):
    x = ac.cc.configuration(case)
    lam = ac.multipliers(case, axis, side, order, kind)[0]
    dv = np.asarray(v, dtype=LD).reshape(x.shape)
    rp, _ = ac.residual(case, axis, side, order, kind, (x + LD(h) * dv).astype(dtype), lam, dtype)
    rm, _ = ac.residual(case, axis, side, order, kind, (x - LD(h) * dv).astype(dtype), lam, dtype)
    return (rp - rm) / dtype(2 * h)


def test_consistent_tangent_is_the_derivative_of_the_reference_residual():
    worst, where = 0.0, None
    for case, order, axis, side, kind in ac.all_faces():
        R = ac.reference(case, axis, side, order, kind)
        for k, v in enumerate(vectors(case, axis, side)):
            d = R.switch / fc.PENALTY                                  # a length: the nearest switch in units of the gap
            h = min(1.0e-6, 1.0e-3 * d / float(np.abs(v).max()))
            q = quotient(case, axis, side, order, kind, v, h, LD) * LD(fc.GRAD_FACTOR)
            if R.n_active == 0:
                assert not np.any(q) and not np.any(R.Kv[k])
                continue
            dev = float(np.abs(q - R.Kv[k]).max() / R.scale[k].max())
            if dev > worst:
                worst, where = dev, (case, order, axis, side, kind)
    print(f"figures augmented consistent K against the central difference: worst {worst:.2e} at {where}")
    assert worst <= 10 * ac.LD_WORST


@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("case", ac.FD_CASES)
def test_float64_quotient_at_the_device_tests_step(case, kind):
    """what tests/test_augmented_gpu.py asks of the device's quotient, asked of the reference rounded to doubles: no node
    crosses its switch within the step, and the quotient meets that test's bar"""
    worst = 0.0
    for axis, side in fc.faces(case):
        R = ac.reference(case, axis, side, -1, kind)
        for k, v in enumerate(vectors(case, axis, side)):
            q = quotient(case, axis, side, -1, kind, v, ac.FD_STEP, np.float64) * fc.GRAD_FACTOR
            worst = max(worst, float(np.abs(q - R.Kv[k]).max() / R.scale[k].max()))
    print(f"figures augmented float64 quotient {case} {kind}: {worst:.2e} (bar {10 * ac.F64_WORST:.2e})")
    assert worst <= 10 * ac.F64_WORST


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
def test_inputs_are_what_the_cases_file_says():
    no_active, no_released, no_positive, smallest = [], [], [], (np.inf, None)
    for case, order, axis, side, kind in ac.all_faces():
        R = ac.reference(case, axis, side, order, kind)                # (asserts the switch margin)
        if R.n_active == 0:
            no_active.append((case, order, axis, side, kind))
        if not np.any((R.lam < 0) & (R.pressure == 0)):
            no_released.append((case, order, axis, side, kind))
        if not np.any(R.active & (R.gt > 0)):
            no_positive.append((case, order, axis, side, kind))
        rel = R.switch / (fc.PENALTY * R.s)
        if rel < smallest[0]:
            smallest = (rel, (case, order, axis, side, kind))
        assert (np.abs(R.Kv_new).max() > 0 and np.abs(R.r).max() > 0) == (R.n_active > 0)
    print(f"figures augmented inputs: no active node on {no_active}; no released node with a multiplier on {no_released}; "
          f"{len(no_positive)} of {len(ac.all_faces())} without a node active at a positive gap; smallest switch distance "
          f"{smallest[0]:.2e} eps s at {smallest[1]}")
    assert no_active == [("mix2d_31", 41, 0, 0, "plane"), ("mix2d_31", 41, 0, 0, "sphere")]
    assert no_released == [("block2d_p4", -1, 0, 0, "sphere")]
    assert len(no_positive) == 9
    assert smallest[1] == ("rep3d_p1", 15, 1, 1, "plane") and abs(smallest[0] - 9.9e-4) < 1e-5 and smallest[0] >= ac.SWITCH_MARGIN


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
class _Flags:
    def __init__(self, **kw):
        self.kw = kw

    def get_int(self, key, default=0):
        return self.kw.get(key, default)


class _Markers:
    def __init__(self):
        import types
        self.initial = types.SimpleNamespace(contact_={}, pressure_={})
        self.current = types.SimpleNamespace(contact_={})


ITERATIVE = dict(use_iterative_solver=1, use_kronecker_preconditioner=1)
MATRIX_FREE = dict(ITERATIVE, matrix_free=1, matrix_free_boundary=1)


@pytest.mark.parametrize("flags", [dict(), dict(use_iterative_solver=1), ITERATIVE, MATRIX_FREE,
                                   dict(MATRIX_FREE, contact_consistent_tangent=1),
                                   dict(MATRIX_FREE, contact_consistent_tangent=1, friction_matrix_free=1),
                                   dict(MATRIX_FREE, friction_matrix_free=1)], ids=lambda f: "+".join(f) or "direct")
def test_route_accepts_the_flag_on_every_implicit_route(flags):
    from mimi_amd.solid import Route, resolve_route
    off = resolve_route(_Flags(**flags), _Markers(), ())
    on = resolve_route(_Flags(**flags, contact_augmented_lagrange=1), _Markers(), ())
    assert not off.augmented_contact and on.augmented_contact and on == off._replace(augmented_contact=True)
    assert Route().augmented_contact is False and Route._fields[-1] == "augmented_contact"


def test_route_refuses_the_flag_with_explicit_dynamics():
    from mimi_amd.solid import resolve_route
    with pytest.raises(RuntimeError, match="contact_augmented_lagrange cannot be combined with explicit_dynamics"):
        resolve_route(_Flags(explicit_dynamics=1, contact_augmented_lagrange=1), _Markers(), ())
    assert resolve_route(_Flags(explicit_dynamics=1), _Markers(), ()).explicit


def test_header_and_exports_name_the_entries():
    from mimi_amd import _capi
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        text = f.read()
    for e in ENTRIES:
        assert re.search(r"^int " + e + r"\(mimi_hip_contact_t h", text, flags=re.M) and e in _capi.EXPORTS
    assert re.search(r"^#define MIMI_HIP_ABI_VERSION 12$", text, flags=re.M)


# ---- (6) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("penalty", [1.0e4, 2.0e3])
def test_stepping_restatement(penalty):
    import _augmented_stepping as st
    run = st.run(penalty)
    for k, step in enumerate(run.steps):
        assert all(info["converged"] for info in step.newton), (k, step.newton)
        print(f"figures augmented stepping eps {penalty:g} step {k + 1}: Newton iterations {[i['iterations'] for i in step.newton]}, "
              f"violations {' '.join(f'{v:.3e}' for v in step.violations)}")
        if step.violations[0] > 0:
            assert step.violations[-1] <= st.RATIO_BAR[penalty] * step.violations[0]
    assert run.steps[st.IMPACT_STEP].violations[0] > 0
    assert len(run.steps[st.IMPACT_STEP].violations) == st.AUGMENTATIONS + 1
