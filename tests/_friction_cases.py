"""Inputs of the friction tests (tests/test_friction_cpu.py, tests/test_friction_gpu.py) on the faces, bodies and
displacements of tests/_face_cases.py, with the long-double reference of tests/_friction_reference.py cached per
(case, axis, side, order, kind).

Three configurations per case: u0 = fc.displacement(case), u1 = u0 + a smooth increment of 0.25 U_SCALE (seed 2), u2 = u1 +
another (seed 3).  The staged history every test walks:
    commit at u0 (nothing in contact before: xi = 0, c = the contact set of u0)
    evaluation at u1 against that state                                       -> ev1   (stick and slip, r, K, history)
    commit at u1, then an evaluation at u2 with the body increment d          -> ev2
mu = 0.3.  The tangential penalty is sized per (case, face, order, kind) so that stick and slip both occur at u1 and no point
sits on the kink: with xi = 0 a point sticks iff |s| / p_N <= mu / eps_T, and the cut mu / eps_T is put into the middle of
the widest gap between neighbouring sorted |s| / p_N inside the WINDOW quantiles (the idea of fc._widest_gap).
tests/test_friction_cpu.py asserts what that gives.

Bars: r to fc.TOL["contact_r"], K to fc.TOL["contact_K"] (relative to the largest reference entry), the elastic slip to
XI_TOL, relative to its largest entry -- the bars of the frictionless kernels on these faces; the one new cancellation,
x_q - xbar at increments of 5e-3 of the extent, costs about 1e-13."""
import functools
import types

import numpy as np

import _face_cases as fc
import _face_reference as fr
import _friction_reference as fq

LD = np.longdouble
MU = 0.3
WINDOW = (0.25, 0.75)
XI_TOL = 1e-12
BODY_STEP = 0.002            # |d| of stage 6, in extents of the face
CASES = [("rep2d_p3", -1), ("mix3d_211", -1), ("rep3d_p2", -1), ("block2d_p4", -1), ("rep3d_p1", 15), ("mix2d_31", 41),
         ("nonuni3d_p3", -1)]
KINDS = ("plane", "sphere")


@functools.lru_cache(maxsize=None)
def displacements(case):
    X = fc.product_patch(case).control_points
    u0 = np.array(fc.displacement(case))
    u1 = u0 + fc.smooth_displacement(X, 0.25 * fc.U_SCALE, seed=2)
    u2 = u1 + fc.smooth_displacement(X, 0.25 * fc.U_SCALE, seed=3)
    for u in (u0, u1, u2):
        u.setflags(write=False)
    return u0, u1, u2


@functools.lru_cache(maxsize=None)
def points(case, axis, side, order, k):
    """reference points of the face on X + u_k"""
    B = fc.product_patch(case)
    x = B.control_points.astype(LD) + displacements(case)[k].reshape(-1, B.dim).astype(LD)
    return fr.face_points(fc.face_basis(case, axis, side, order), x)


@functools.lru_cache(maxsize=None)
def contact(case, axis, side, order, kind, k):
    """the frictionless reference at u_k (nodal pressures; r and K with fc.GRAD_FACTOR)"""
    return fr.mortar_contact(points(case, axis, side, order, k), fc.body(case, axis, side, order, kind), fc.PENALTY, fc.GRAD_FACTOR)


def extent(case, axis, side, order):
    pts = points(case, axis, side, order, 0)
    x, da = pts.x.astype(np.float64), pts.da.astype(np.float64)
    centroid = (da[:, None] * x).sum(axis=0) / da.sum()
    return float(np.linalg.norm(x - centroid, axis=1).max())


def body_step(case, axis, side, order):
    """d of stage 6: BODY_STEP extents along the mean first surface tangent of the face at u0"""
    pts = points(case, axis, side, order, 0)
    t = (pts.da[:, None] * pts.t[:, 0, :]).sum(axis=0).astype(np.float64)
    return BODY_STEP * extent(case, axis, side, order) * t / np.linalg.norm(t)


def _cut(values):
    """(the middle of the widest gap between neighbouring sorted values inside the WINDOW quantiles, the gap / the cut)"""
    v = np.sort(np.asarray(values, dtype=np.float64))
    n = len(v)
    lo = max(1, int(np.ceil(WINDOW[0] * n)))
    hi = max(lo + 1, min(n, int(np.floor(WINDOW[1] * n)) + 1))
    k = lo + int(np.argmax(np.diff(v[lo - 1:hi])))
    cut = 0.5 * (v[k - 1] + v[k])
    return cut, (v[k] - v[k - 1]) / cut


@functools.lru_cache(maxsize=None)
def sizing(case, axis, side, order, kind):
    """eps_T and what it was sized on: the eligible points of u1 (in contact at u0 and at u1)"""
    p0, p1 = points(case, axis, side, order, 0), points(case, axis, side, order, 1)
    c0 = fq.point_pressure(p0, contact(case, axis, side, order, kind, 0)) < 0
    state = types.SimpleNamespace(xi=np.zeros_like(p0.x), xbar=p0.x, c=c0)
    tr = fq.tractions(p1, fq.point_pressure(p1, contact(case, axis, side, order, kind, 1)), state, MU, 1.0)
    ratio = (tr.sn[tr.on] / tr.pn[tr.on]).astype(np.float64)
    if len(ratio) < 2:
        return types.SimpleNamespace(eps_t=1.0, n_eligible=len(ratio), margin=0.0)
    cut, margin = _cut(ratio)
    return types.SimpleNamespace(eps_t=float(MU / cut), n_eligible=len(ratio), margin=float(margin))


@functools.lru_cache(maxsize=None)
def reference(case, axis, side, order, kind):
    """the staged history: st0 (initial), ev0 / st1 (at u0, committed), ev1 / st2 (at u1, committed), ev2 (at u2 with d)"""
    eps_t = sizing(case, axis, side, order, kind).eps_t
    p = [points(case, axis, side, order, k) for k in range(3)]
    c = [contact(case, axis, side, order, kind, k) for k in range(3)]
    st0 = fq.initial_state(len(p[0].x), p[0].fb.dim)
    ev0 = fq.evaluate(p[0], c[0], st0, MU, eps_t, with_tangent=False)
    ev1 = fq.evaluate(p[1], c[1], ev0.trial, MU, eps_t, grad_factor=fc.GRAD_FACTOR)
    d = body_step(case, axis, side, order)
    ev2 = fq.evaluate(p[2], c[2], ev1.trial, MU, eps_t, d=d, grad_factor=fc.GRAD_FACTOR)
    return types.SimpleNamespace(eps_t=eps_t, d=d, pts=p, contact=c, st0=st0, ev0=ev0, ev1=ev1, ev2=ev2, nodes=c[0].nodes,
                                 extent=extent(case, axis, side, order))


def product_body(b, **kw):
    from mimi_amd.integrators import RigidPlane, RigidSphere
    if b["kind"] == "plane":
        return RigidPlane(b["point"], b["normal"], fc.PENALTY, **kw)
    return RigidSphere(b["center"], b["radius"], fc.PENALTY, **kw)
