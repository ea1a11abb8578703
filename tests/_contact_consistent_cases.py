"""Inputs and recorded figures of the consistent contact tangent's tests (tests/test_contact_consistent_cpu.py,
tests/test_contact_consistent_gpu.py): the faces, bodies, displacement and penalty of tests/_face_cases.py, the two vectors
per face of tests/test_boundary_action_cpu.py, and per face the products of the long-double reference of
tests/_contact_consistent_reference.py with them -- cached, read-only; the dense matrices are not kept."""
import functools
import types

import numpy as np

import _contact_consistent_reference as ccr
import _face_cases as fc
import _face_reference as fr
import _patches
from test_boundary_action_cpu import vectors

LD = np.longdouble
KINDS = ("plane", "sphere")
ALL = [(c, -1) for c in list(_patches.CASES) + fc.BLOCKS] + fc.ORDERS_ALL + fc.ORDERS_CONTACT
# the cases of the device's own difference quotient (test_contact_consistent_gpu.py (2)), at the default order
FD_CASES = ("rep3d_p2", "rep2d_p3")
FD_STEP = 1.0e-6

# Worst deviation of the central difference of the reference residual from the reference's K v, on the scale
# max_i (K_abs |v|)_i, measured by tests/test_contact_consistent_cpu.py on every face of ALL, plane and sphere:
#   long double, h = min(1e-6, 1e-3 min_q |g_true| / max |v|):   LD_WORST   (the reference is vetted at 10 x this)
#   float64, h = 1e-6, on the faces of FD_CASES:                  F64_WORST  (the device's quotient is held to 10 x this)
LD_WORST = 1.27e-11     # mix2d_23, plane: the h^2 term of the quotient; most faces sit at 1e-12
F64_WORST = 9.5e-11     # rep3d_p2, plane (9.42e-11): the rounding of r over 2 h


def residual(case, axis, side, order, kind, x, dtype=LD):
    """the reference's contact residual on the configuration x [n_nodes, dim]"""
    pts = fr.face_points(fc.face_basis(case, axis, side, order), x)
    r = fr.mortar_contact(pts, fc.body(case, axis, side, order, kind), fc.PENALTY, with_tangent=False).r
    return np.asarray(r, dtype=dtype)


def configuration(case):
    B = fc.product_patch(case)
    return B.control_points.astype(LD) + fc.displacement(case).reshape(-1, B.dim).astype(LD)


@functools.lru_cache(maxsize=None)
def products(case, axis, side, order, kind):
    """Kv, scale = K_abs |v|, new = K_new v [2, n_vdofs] (doubles; K carries fc.GRAD_FACTOR) for the two vectors of the face,
    and g_min = min_q |g_true|"""
    ref = ccr.consistent_contact(fc.points(case, axis, side, order), fc.body(case, axis, side, order, kind), fc.PENALTY,
                                 fc.GRAD_FACTOR)
    v = vectors(case, axis, side).astype(LD)
    out = types.SimpleNamespace(Kv_ld=(ref.K @ v.T).T, scale_ld=(ref.K_abs @ np.abs(v).T).T,
                                g_min=float(np.abs(ref.g_true).min()))
    out.Kv = np.asarray(out.Kv_ld, dtype=np.float64)
    out.scale = np.asarray(out.scale_ld, dtype=np.float64)
    out.new = np.asarray((ref.K_new @ v.T).T, dtype=np.float64)
    for a in (out.Kv, out.scale, out.new):
        a.setflags(write=False)
    return out
