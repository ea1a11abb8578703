"""Rigid spline bodies with a known answer, placed over the last face of a block like sphere_over_top / dome_surface of
tests/test_contact.py, for tests/test_spline_body_cpu.py and tests/test_contact_spline_gpu.py.  Every builder returns the
body dict of tests/test_contact.py and, where there is one, the analytic twin (`twin`: the body dict of ContactOracle).

Orientation: the rigid normal (t_y, -t_x) / S_u x S_v points out of the rigid body, i.e. DOWN onto the face."""
import functools

import numpy as np

from _cases import synthetic_u

BLOCKS_2D = [((6, 3), 2, 1), ((4, 3), 3, 1)]
BLOCKS_3D = [((4, 4, 2), 2, 2), ((3, 3, 2), 3, 2)]
S45 = np.sqrt(0.5)


def _spline(degrees, knots, ctrl, weights, resolution, **extra):
    return dict(kind="spline", degrees=list(degrees), knots=[np.asarray(k, dtype=float) for k in knots],
                control_points=np.asarray(ctrl, dtype=float), weights=None if weights is None else np.asarray(weights, dtype=float),
                resolution=resolution, **extra)


def _sphere(L, axis):
    R = 0.25 * L[0]
    c = 0.5 * L
    c[axis] = L[axis] + 0.9 * R
    return c, float(R)


CIRCLE_PTS = np.array([[1, 0], [1, 1], [0, 1], [-1, 1], [-1, 0], [-1, -1], [0, -1], [1, -1], [1, 0]], dtype=float)
CIRCLE_W = np.array([1, S45, 1, S45, 1, S45, 1, S45, 1])
CIRCLE_KNOTS = np.array([0, 0, 0, .25, .25, .5, .5, .75, .75, 1, 1, 1])
# where the seam S(0) = S(1) of the 9-point circle sits: quarter turns of the control points, orientation kept
TURNS = {"side": np.eye(2), "down": np.array([[0.0, 1.0], [-1.0, 0.0]]), "up": np.array([[0.0, -1.0], [1.0, 0.0]])}


def circle(L, seam):
    """the 9-point quadratic NURBS circle, counter-clockwise, with its seam at the side (+x), facing the face (down) or away"""
    c, R = _sphere(L, 1)
    pts = CIRCLE_PTS @ TURNS[seam].T
    return _spline([2], [CIRCLE_KNOTS], c + R * pts, CIRCLE_W, 64, twin=dict(kind="sphere", center=list(c), radius=R))


def parabola(L):
    """y = y0 + a (x - xc)^2 exactly: a quadratic B-spline on non-uniform knots whose control points are the blossom of
    the polynomial (x linear in the parameter), left to right"""
    xc, y0, a = 0.5 * L[0], L[1] - 0.05, 0.35
    U = np.array([0, 0, 0, 0.13, 0.37, 0.5, 0.81, 1, 1, 1])
    x0, dx = -0.4, L[0] + 0.8
    ctrl = [[x0 + dx * 0.5 * (U[i + 1] + U[i + 2]), y0 + a * (x0 - xc + dx * U[i + 1]) * (x0 - xc + dx * U[i + 2])]
            for i in range(len(U) - 3)]
    return _spline([2], [U], ctrl, None, 64, parabola=(xc, y0, a))


def _tilted(L, axis, along, slope=0.004, depth=0.03):
    normal = np.zeros(len(L))
    normal[axis], normal[along] = -1.0, slope
    normal /= np.linalg.norm(normal)
    point = 0.5 * L
    point[axis] = L[axis] - depth
    return point, normal


def _uneven_knots(p, n_inner, rng):
    inner = np.sort(rng.uniform(0.08, 0.92, n_inner))
    return np.concatenate([np.zeros(p + 1), inner, np.ones(p + 1)])


def _uneven_stations(n, rng):
    """n increasing stations in [0, 1] with uneven gaps, ends included"""
    gaps = rng.uniform(0.3, 1.7, n - 1)
    return np.concatenate([[0.0], np.cumsum(gaps) / gaps.sum()])


def flat_curve(L, p):
    """a straight, tilted curve of degree p: collinear, unevenly spaced control points on non-uniform knots"""
    rng = np.random.default_rng(100 + p)
    point, normal = _tilted(L, 1, 0)
    U = _uneven_knots(p, 3, rng)
    s = _uneven_stations(len(U) - p - 1, rng)
    t = np.array([-normal[1], normal[0]])                      # normal = (t_y, -t_x)
    ctrl = point + ((-0.5 * L[0] - 0.6) + (L[0] + 1.2) * s)[:, None] * t
    return _spline([p], [U], ctrl, None, 64, twin=dict(kind="plane", point=list(point), normal=list(normal)))


def open_arc(L):
    """a quarter of the circle (one rational quadratic segment, -135 deg to -45 deg): shorter than the face, so the
    face points beyond its ends are clipped to an end point"""
    c, R = _sphere(L, 1)
    ctrl = c + R * np.array([[-S45, -S45], [0.0, -np.sqrt(2.0)], [S45, -S45]])
    return _spline([2], [[0, 0, 0, 1, 1, 1]], ctrl, [1, S45, 1], 64, twin=dict(kind="sphere", center=list(c), radius=R))


def cylinder(L, seam):
    """a NURBS cylinder, degree 2 x 1, its axis along y above the top face: the first parametric direction is the
    9-point circle in the x-z plane (counter-clockwise seen from -y, so the axis runs from +y to -y for an outward
    normal), seam at the side or facing the face"""
    c, R = _sphere(L, 2)
    pts = CIRCLE_PTS @ TURNS[seam].T
    ring = np.zeros((9, 3))
    ring[:, 0], ring[:, 2] = c[0] + R * pts[:, 0], c[2] + R * pts[:, 1]
    ctrl = []
    for y in (L[1] + 0.5, -0.5):
        layer = ring.copy()
        layer[:, 1] = y
        ctrl.append(layer)
    return _spline([2, 1], [CIRCLE_KNOTS, [0, 0, 1, 1]], np.concatenate(ctrl), np.tile(CIRCLE_W, 2), 24,
                   axis_point=np.array([c[0], 0.0, c[2]]), axis_dir=np.array([0.0, 1.0, 0.0]), radius=R)


def sphere_patch(L):
    """a rational biquadratic patch of the sphere that stays away from its poles (on the y axis): 90 deg of longitude
    around the lowest point (first direction) x 90 deg of latitude (second direction, from +45 deg to -45 deg)"""
    c, R = _sphere(L, 2)
    arc = np.array([[-S45, -S45], [0.0, -np.sqrt(2.0)], [S45, -S45]])        # (x, z) of the unit circle, going +x
    mer = np.array([[S45, S45], [np.sqrt(2.0), 0.0], [S45, -S45]])           # (rho, y), from +y to -y
    w1 = np.array([1, S45, 1])
    ctrl, w = [], []
    for j in range(3):
        for i in range(3):
            ctrl.append([c[0] + R * mer[j, 0] * arc[i, 0], c[1] + R * mer[j, 1], c[2] + R * mer[j, 0] * arc[i, 1]])
            w.append(w1[i] * w1[j])
    k = [0, 0, 0, 1, 1, 1]
    return _spline([2, 2], [k, k], ctrl, w, 24, twin=dict(kind="sphere", center=list(c), radius=R))


def dome(L, frac, depth=0.06):
    """the dome of tests/test_contact.py: dome_surface over the middle `frac` of the top face only (frac > 1: beyond it)"""
    n = 6
    k = np.concatenate([np.zeros(2), np.linspace(0, 1, n - 1), np.ones(2)])
    g = np.array([k[i + 1:i + 3].sum() / 2 for i in range(n)])
    ctrl = np.zeros((n, n, 3))                       # [second (x)][first (y)]
    for ix in range(n):
        for iy in range(n):
            x, y = L[0] * (0.5 + frac * (g[ix] - 0.5)), L[1] * (0.5 + frac * (g[iy] - 0.5))
            r2 = ((x - 0.5 * L[0]) / L[0]) ** 2 + ((y - 0.5 * L[1]) / L[1]) ** 2
            ctrl[ix, iy] = [x, y, L[2] - depth + 0.8 * r2]
    return _spline([2, 2], [k, k], ctrl.reshape(-1, 3), None, 24)


def flat_surface(L, p):
    """a flat, tilted surface of degree p x p (first direction along y, second along x, as the dome): a tensor grid of
    unevenly spaced stations on non-uniform knots"""
    rng = np.random.default_rng(200 + p)
    point, normal = _tilted(L, 2, 0)
    U = [_uneven_knots(p, 2, rng) for _ in range(2)]
    sy, sx = (_uneven_stations(len(u) - p - 1, rng) for u in U)
    ex = np.array([normal[2], 0.0, -normal[0]])
    ex /= np.linalg.norm(ex)
    ey = np.cross(ex, normal)
    ctrl = []
    for b in sx:
        for a in sy:
            ctrl.append(point + ((-0.5 * L[0] - 0.6) + (L[0] + 1.2) * b) * ex + ((-0.5 * L[1] - 0.6) + (L[1] + 1.2) * a) * ey)
    ctrl = np.array(ctrl)
    # S_first x S_second must be the rigid normal
    first, second = ctrl[1] - ctrl[0], ctrl[len(sy)] - ctrl[0]
    assert np.dot(np.cross(first, second), normal) > 0
    return _spline([p, p], U, ctrl, None, 24, twin=dict(kind="plane", point=list(point), normal=list(normal)))


BODIES_2D = {
    "circle-seam-side": lambda L: circle(L, "side"),
    "circle-seam-down": lambda L: circle(L, "down"),
    "circle-seam-up": lambda L: circle(L, "up"),
    "parabola": parabola,
    "flat-p1": lambda L: flat_curve(L, 1),
    "flat-p2": lambda L: flat_curve(L, 2),
    "flat-p3": lambda L: flat_curve(L, 3),
    "flat-p5": lambda L: flat_curve(L, 5),
    "open-arc": open_arc,
}
BODIES_3D = {
    "cylinder-seam-side": lambda L: cylinder(L, "side"),
    "cylinder-seam-down": lambda L: cylinder(L, "down"),
    "sphere-patch": sphere_patch,
    "dome": lambda L: dome(L, 1.0 + 1.0 / min(L[0], L[1])),
    "small-dome": lambda L: dome(L, 0.5),
    "flat-p1xp1": lambda L: flat_surface(L, 1),
    "flat-p3xp3": lambda L: flat_surface(L, 3),
}
CLIPPING = {"open-arc", "sphere-patch", "small-dome"}          # cases about end / edge / corner clipping
CASES = ([(b, name) for b in BLOCKS_2D for name in BODIES_2D] + [(b, name) for b in BLOCKS_3D for name in BODIES_3D])
CASE_IDS = ["%s-p%d-%s" % ("x".join(map(str, b[0])), b[1], name) for b, name in CASES]


@functools.lru_cache(maxsize=None)
def setup(block, name):
    """(oracle Patch, product patch tables, u, body dict) of one case"""
    from mimi_amd import splines
    import mimi_amd
    from oracle import iga
    n_el, p, axis = block
    P = iga.Patch.block(n_el, p)
    L = P.ctrl.max(axis=0)
    body = (BODIES_2D if len(n_el) == 2 else BODIES_3D)[name](L)
    patch = mimi_amd.BSplinePatch.block(n_el, p)
    tables = splines.face_tables(patch, axis, 1)
    return P, patch, tables, synthetic_u(P, scale=0.01), body


@functools.lru_cache(maxsize=None)
def reference(block, name):
    """nodal_gap_area of the long-double reference for one case: computed once, shared, never modified"""
    import _closest_point as cp
    P, patch, tables, u, body = setup(block, name)
    B = cp.Body(body)
    return B, cp.nodal_gap_area(P, tables, u, B, penalty=1.0e4)


# ---- bounds -------------------------------------------------------------------------------------------------------------
# Every asserted bound is 10 x a difference MEASURED on the CPU with the oracle (oracle/contact_path.c, after the seam
# fix), floored at 1e-13 and capped at 1e-10 (the bound test_contact_spline_body_parity_gpu asserts): the factor of ten
# covers the other summation order of the device's fixed-order sums and its fused multiply-adds.  All differences are
# max |a - b| / max |b|.
#
# MEASURED_NODAL: oracle against the long-double reference (nodal_gap_area), the largest of nodal area, nodal gap, nodal
# pressure and GapNorm.  MEASURED_TWIN: the oracle's spline body against the oracle's analytic twin, the larger of
# residual and exact tangent (grad factor 0.6).
MEASURED_NODAL = {
    "6x3-p2-circle-seam-side": 1.7e-15,
    "6x3-p2-circle-seam-down": 1.9e-15,
    "6x3-p2-circle-seam-up": 1.9e-15,
    "6x3-p2-parabola": 6.3e-15,
    "6x3-p2-flat-p1": 1.1e-14,
    "6x3-p2-flat-p2": 1.6e-14,
    "6x3-p2-flat-p3": 1.6e-14,
    "6x3-p2-flat-p5": 1.6e-14,
    "6x3-p2-open-arc": 4.0e-15,
    "4x3-p3-circle-seam-side": 1.9e-15,
    "4x3-p3-circle-seam-down": 2.1e-15,
    "4x3-p3-circle-seam-up": 1.2e-15,
    "4x3-p3-parabola": 2.5e-15,
    "4x3-p3-flat-p1": 9.0e-15,
    "4x3-p3-flat-p2": 1.4e-14,
    "4x3-p3-flat-p3": 1.2e-14,
    "4x3-p3-flat-p5": 1.4e-14,
    "4x3-p3-open-arc": 1.8e-15,
    "4x4x2-p2-cylinder-seam-side": 4.7e-15,
    "4x4x2-p2-cylinder-seam-down": 7.0e-15,
    "4x4x2-p2-sphere-patch": 7.3e-15,
    "4x4x2-p2-dome": 1.4e-14,
    "4x4x2-p2-small-dome": 9.4e-15,
    "4x4x2-p2-flat-p1xp1": 4.8e-15,
    "4x4x2-p2-flat-p3xp3": 1.3e-14,
    "3x3x2-p3-cylinder-seam-side": 1.1e-14,
    "3x3x2-p3-cylinder-seam-down": 9.2e-15,
    "3x3x2-p3-sphere-patch": 1.2e-14,
    "3x3x2-p3-dome": 3.8e-14,
    "3x3x2-p3-small-dome": 1.3e-14,
    "3x3x2-p3-flat-p1xp1": 1.2e-14,
    "3x3x2-p3-flat-p3xp3": 1.9e-14,
}
MEASURED_TWIN = {
    "6x3-p2-circle-seam-side": 1.3e-15,
    "6x3-p2-circle-seam-down": 2.5e-16,
    "6x3-p2-circle-seam-up": 1.7e-15,
    "6x3-p2-flat-p1": 5.2e-15,
    "6x3-p2-flat-p2": 1.5e-14,
    "6x3-p2-flat-p3": 1.1e-14,
    "6x3-p2-flat-p5": 1.5e-14,
    "6x3-p2-open-arc": 2.0e-15,
    "4x3-p3-circle-seam-side": 5.8e-15,
    "4x3-p3-circle-seam-down": 6.0e-15,
    "4x3-p3-circle-seam-up": 3.1e-15,
    "4x3-p3-flat-p1": 8.3e-15,
    "4x3-p3-flat-p2": 1.3e-14,
    "4x3-p3-flat-p3": 1.4e-14,
    "4x3-p3-flat-p5": 1.4e-14,
    "4x3-p3-open-arc": 4.7e-15,
    "4x4x2-p2-sphere-patch": 1.1e-15,
    "4x4x2-p2-flat-p1xp1": 5.3e-15,
    "4x4x2-p2-flat-p3xp3": 1.3e-14,
    "3x3x2-p3-sphere-patch": 8.9e-15,
    "3x3x2-p3-flat-p1xp1": 3.5e-15,
    "3x3x2-p3-flat-p3xp3": 9.5e-15,
}


def bound(measured):
    return min(max(10.0 * measured, 1e-13), 1e-10)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / np.abs(b).max())
