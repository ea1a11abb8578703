"""Inputs and recorded figures of the friction action's tests (tests/test_friction_action_cpu.py,
tests/test_friction_action_gpu.py): the staged history of tests/_friction_cases.py -- commit at u0, evaluate at u1, where
stick and slip both occur and no point sits on the kink -- on all of its cases and kinds of body, the two vectors per face of
tests/test_boundary_action_cpu.py, and per face the products of the long-double reference of
tests/_friction_action_reference.py with them -- cached, read-only; the dense matrices are not kept."""
import functools
import types

import numpy as np

import _contact_consistent_cases as cc
import _face_cases as fc
import _face_reference as fr
import _friction_action_reference as far
import _friction_cases as fx
from test_boundary_action_cpu import vectors

LD = np.longdouble
CASES, KINDS = fx.CASES, fx.KINDS
# the cases of the device's own difference quotient (test_friction_action_gpu.py (2)), at the default order
FD_CASES = cc.FD_CASES
FD_STEP = cc.FD_STEP

# Worst deviation of the central difference of the reference's total residual (contact + friction, committed state frozen)
# from the reference's K v, K = consistent contact + friction + the new part, on the scale max_i (|K| |v|)_i with |K|
# entrywise, measured by tests/test_friction_action_cpu.py on every face of CASES, plane and sphere:
#   long double, h = min(1e-6, 1e-3 min_q |g_true| / max |v|):   LD_WORST   (the reference is vetted at 10 x this)
#   float64, h = 1e-6, on the faces of FD_CASES:                  F64_WORST  (the device's quotient is held to 10 x this)
LD_WORST = 1.1e-10     # mix3d_211, plane (1.07e-10; sphere 9.7e-11): the h^2 term of the quotient; most faces sit below 1e-11
F64_WORST = 2.4e-10    # rep3d_p2, sphere (2.32e-10; rep2d_p3 plane 2.27e-10): the rounding of r over 2 h


def configuration(case, k=1):
    B = fc.product_patch(case)
    return B.control_points.astype(LD) + fx.displacements(case)[k].reshape(-1, B.dim).astype(LD)


def committed(case, axis, side, order, kind):
    """(the state committed at u0, eps_T)"""
    ref = fx.reference(case, axis, side, order, kind)
    return ref.ev0.trial, ref.eps_t


def residual(case, axis, side, order, kind, x, dtype=LD):
    """the reference's total residual on the configuration x [n_nodes, dim] against the state committed at u0, with the
    branch and the contact flag [g < 0] of every point"""
    state, eps_t = committed(case, axis, side, order, kind)
    pts = fr.face_points(fc.face_basis(case, axis, side, order), x)
    out = far.total_residual(pts, fc.body(case, axis, side, order, kind), fc.PENALTY, state, fx.MU, eps_t)
    return np.asarray(out.r, dtype=dtype), np.asarray(out.tr.branch), np.asarray(out.g < 0)


@functools.lru_cache(maxsize=None)
def products(case, axis, side, order, kind):
    """For the two vectors of the face [2, n_vdofs]: Kv (consistent total), Kv_frozen (frozen total), scale = |K| |v|,
    scale_frozen = |K_frozen| |v|, new = the friction's new part K_new v (K carries fc.GRAD_FACTOR); g_min = min_q |g_true|,
    the branches and contact flags at u1"""
    state, eps_t = committed(case, axis, side, order, kind)
    pts = fx.points(case, axis, side, order, 1)
    ref = far.total_tangents(pts, fc.body(case, axis, side, order, kind), fc.PENALTY, state, fx.MU, eps_t, grad_factor=fc.GRAD_FACTOR)
    v = vectors(case, axis, side).astype(LD)
    out = types.SimpleNamespace(Kv_ld=(ref.K @ v.T).T, scale_ld=(np.abs(ref.K) @ np.abs(v).T).T, g_min=float(np.abs(ref.g).min()),
                                branch=np.asarray(ref.tr.branch), inside=np.asarray(ref.g < 0))
    out.Kv = np.asarray(out.Kv_ld, dtype=np.float64)
    out.scale = np.asarray(out.scale_ld, dtype=np.float64)
    out.Kv_frozen = np.asarray((ref.K_frozen @ v.T).T, dtype=np.float64)
    out.scale_frozen = np.asarray((np.abs(ref.K_frozen) @ np.abs(v).T).T, dtype=np.float64)
    out.new = np.asarray((ref.K_new @ v.T).T, dtype=np.float64)
    for a in (out.Kv, out.scale, out.Kv_frozen, out.scale_frozen, out.new, out.branch, out.inside):
        a.setflags(write=False)
    return out


def dense_new_parts(pts, body, penalty, state, mu, eps_t, grad_factor):
    """what the consistent action adds to the assembled Jacobian (contact's new part + friction's), dense, in doubles"""
    ref = far.total_tangents(pts, body, penalty, state, mu, eps_t, grad_factor=grad_factor)
    return np.asarray(ref.K_contact_new + ref.K_new, dtype=np.float64)
