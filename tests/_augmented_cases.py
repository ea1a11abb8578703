"""Inputs and recorded figures of the augmented-Lagrangian contact tests (tests/test_augmented_cpu.py,
tests/test_augmented_gpu.py, tests/test_augmented_solid_gpu.py): the faces, bodies (plane, sphere), displacement and PENALTY
of tests/_face_cases.py, the two vectors per face of tests/test_boundary_action_cpu.py, the multipliers below and per
(face, body) the long-double reference of tests/_augmented_reference.py -- cached, read-only.

Multipliers of a face with n marked nodes (s = max_i |gt_i|, the largest nodal mean gap of the face against the body):
    rng = np.random.default_rng(7);  mask = rng.random(n) < 0.5;  lambda = where(mask, -PENALTY s rng.random(n), 0)
so that about half the nodes carry one of the order of the penalty pressure.  With that recipe every (face, body) of CASES
but mix2d_31 order 41 face (0, 0) (four nodes, one multiplier, every mean gap positive: nothing is active, residual and
tangents are zero and are compared as such) has active nodes; every one but block2d_p4 face (0, 0) against the sphere has
released nodes that carry a multiplier (lambda_i < 0, p_i = 0); all but nine have nodes active at a positive mean gap; the
smallest |lambda_i + eps gt_i| is 9.9e-4 eps s (rep3d_p1 order 15, face (1, 1), plane).  tests/test_augmented_cpu.py asserts
all of it.  No node is closer to its switch than SWITCH_MARGIN eps s (asserted in reference()); no node is excluded from a
comparison."""
import functools
import types

import numpy as np

import _augmented_reference as ar
import _contact_consistent_cases as cc
import _face_cases as fc
from test_boundary_action_cpu import vectors

LD = np.longdouble
KINDS = ("plane", "sphere")
CASES = [("rep2d_p2", -1), ("rep3d_p1", -1), ("mix3d_231", -1), ("block2d_p4", -1), ("rep3d_p1", 15), ("mix2d_31", 41)]
FD_CASES, FD_STEP = cc.FD_CASES, cc.FD_STEP          # the device's own difference quotient: cases, step and float64 figure
F64_WORST = cc.F64_WORST                             # of tests/_contact_consistent_cases.py
SWITCH_MARGIN = 1.0e-6
SEED = 7

# Worst deviation of the central difference of the reference's own residual (lambda fixed) from the reference's K v, on the
# scale max_i (K_abs |v|)_i with the step rule of tests/_contact_consistent_cases.py -- long double, h = min(1e-6, 1e-3 d / max
# |v|), d the distance to the nearest switch in units of the displacement (switch / eps) -- measured by
# tests/test_augmented_cpu.py on every (face, body) of CASES; the reference is vetted at 10 x this
LD_WORST = 2.4e-12      # block2d_p4, face (1, 0), plane

# Facade (tests/test_augmented_solid_gpu.py): the largest relative deviation of the device's violation sequence from the
# restatement's (tests/_augmented_stepping.py), over all steps and augmentations; the test holds the device to 10 x this
VIOLATION_DEVIATION = 3.7e-11     # measured on an MI355X at eps = 1e4 (impact step; 1.2e-13 absolute)


@functools.lru_cache(maxsize=None)
def multipliers(case, axis, side, order, kind):
    nodes, area, gap, _ = ar.nodal_gap(fc.points(case, axis, side, order), fc.body(case, axis, side, order, kind))
    s = float(np.abs(gap / area).max())
    rng = np.random.default_rng(SEED)
    n = len(nodes)
    mask = rng.random(n) < 0.5
    lam = np.where(mask, -fc.PENALTY * s * rng.random(n), 0.0)
    lam.setflags(write=False)
    return lam, s


@functools.lru_cache(maxsize=None)
def reference(case, axis, side, order, kind):
    """the reference at fc.displacement(case) with multipliers(...): K carries fc.GRAD_FACTOR; plus the products with the
    face's two vectors (the dense matrices are dropped)"""
    lam, s = multipliers(case, axis, side, order, kind)
    out = ar.augmented_contact(fc.points(case, axis, side, order), fc.body(case, axis, side, order, kind), fc.PENALTY, lam,
                               fc.GRAD_FACTOR)
    assert out.switch >= SWITCH_MARGIN * fc.PENALTY * s, (case, axis, side, order, kind, out.switch / (fc.PENALTY * s))
    v = vectors(case, axis, side).astype(LD)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    out.s, out.lam64 = s, np.array(lam)
    out.Kv, out.scale = f64((out.K @ v.T).T), f64((out.K_abs @ np.abs(v).T).T)
    out.Kv_frozen, out.scale_frozen = f64((out.K_frozen @ v.T).T), f64((out.K_frozen_abs @ np.abs(v).T).T)
    out.Kv_new = f64((out.K_new @ v.T).T)
    out.K_frozen64 = f64(out.K_frozen)
    for name in ("K", "K_abs", "K_new", "K_new_dense", "K_new_abs", "K_frozen", "K_frozen_dense", "K_frozen_abs"):
        delattr(out, name)
    return out


def residual(case, axis, side, order, kind, x, lam, dtype=LD):
    """the reference's residual on the configuration x [n_nodes, dim] with the multipliers lam"""
    import _face_reference as fr
    pts = fr.face_points(fc.face_basis(case, axis, side, order), x)
    out = ar.augmented_contact(pts, fc.body(case, axis, side, order, kind), fc.PENALTY, lam, with_tangent=False)
    return np.asarray(out.r, dtype=dtype), out


def all_faces(cases=None):
    return [(case, order, axis, side, kind) for case, order in (CASES if cases is None else cases) for axis, side in fc.faces(case)
            for kind in KINDS]
