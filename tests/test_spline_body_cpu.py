"""The rigid spline body of MortarContact (mimi_amd/csrc/spline_body.hpp: sb_evaluate, sb_closest_point, sb_nearest) compiled
for the host (tests/host_spline_body.hip, hipcc) and the oracle's restatement of it (oracle/contact_path.c: sp_nearest) against
an independent long-double reference (tests/_closest_point.py: Cox-de Boor from the definition, brute-force global closest
point) and against closed forms (circle, parabola, plane, cylinder, sphere).  No GPU.

Which side of a knot: sb_find_span returns the span with U[i] <= xi < U[i+1], so on an interior knot every derivative is the
one FROM THE RIGHT (from the left at the upper end of the box); the reference's N_{i,0} = [U_i <= x < U_{i+1}] takes the same
side.  S2 is compared on a knot only where it is continuous (degree - multiplicity >= 2).

Bounds: tests/_spline_bodies.py (`bound`): 10 x a measured oracle-vs-reference difference, floored at 1e-13, capped at 1e-10."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _closest_point as cp
import _spline_bodies as sb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble


@pytest.fixture(scope="module")
def host_lib():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = os.path.join(HERE, "_build", "libhost_spline_body.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(HERE, "host_spline_body.hip")])
    return C.CDLL(out)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def product_body(body):
    from mimi_amd.integrators import RigidSpline
    return RigidSpline(body["degrees"], body["knots"], body["control_points"], body["weights"], resolution=body["resolution"])


def host_evaluate(lib, body, xi):
    rs = product_body(body)
    st = rs.c_struct()
    dim, pd, n = rs.control_points.shape[1], len(rs.degrees), len(xi)
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    S, S1, S2 = np.zeros((n, dim)), np.zeros((n, pd, dim)), np.zeros((n, pd, pd, dim))
    lib.host_sb_evaluate(C.byref(st), dim, n, ptr(xi), ptr(S), ptr(S1), ptr(S2))
    return S, S1, S2


def host_closest(lib, body, xq):
    rs = product_body(body)
    st = rs.c_struct()
    dim, pd, n = rs.control_points.shape[1], len(rs.degrees), len(xq)
    xq = np.ascontiguousarray(xq, dtype=np.float64)
    xi, S, S1, g, d = np.zeros((n, pd)), np.zeros((n, dim)), np.zeros((n, pd, dim)), np.zeros(n), np.zeros(n)
    lib.host_sb_closest(C.byref(st), dim, n, ptr(xq), ptr(xi), ptr(S), ptr(S1), ptr(g), ptr(d))
    return xi, S, g, d


def oracle_closest(body, xq):
    """sp_nearest point by point (the ContactOracle only lends its spline fields: any patch of the right dimension)"""
    from oracle import iga, ref_path as rp
    dim = np.asarray(body["control_points"]).shape[1]
    Cn = rp.ContactOracle(iga.Patch.block((1,) * dim, 1), dim - 1, 1, body)
    out = [Cn.spline_nearest(q) for q in xq]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


# ---- sb_evaluate against the long-double evaluation ---------------------------------------------------------------------
def _eval_body(degrees, seed):
    """non-uniform knots with one DOUBLED interior knot per direction, uneven control points, rational weights in [0.5, 2]"""
    rng = np.random.default_rng(seed)
    knots, n = [], []
    for p in degrees:
        inner = np.sort(rng.uniform(0.1, 0.9, 4))
        inner = np.insert(inner, 2, inner[2])                       # multiplicity 2
        knots.append(np.concatenate([np.full(p + 1, -0.25), -0.25 + 1.75 * inner, np.full(p + 1, 1.5)]))
        n.append(len(knots[-1]) - p - 1)
    dim = len(degrees) + 1
    grid = np.meshgrid(*[np.cumsum(rng.uniform(0.3, 1.7, m)) for m in n[::-1]], indexing="ij")[::-1]
    ctrl = np.stack([g.ravel() for g in grid] + [np.zeros(grid[0].size)] * (dim - len(degrees)), axis=1)
    ctrl += 0.3 * rng.standard_normal(ctrl.shape)
    return dict(kind="spline", degrees=list(degrees), knots=knots, control_points=ctrl,
                weights=rng.uniform(0.5, 2.0, len(ctrl)), resolution=8)


EVAL_CASES = [(1,), (2,), (3,), (5,), (2, 1), (3, 2)]


@pytest.mark.parametrize("degrees", EVAL_CASES, ids=lambda d: "x".join(map(str, d)))
def test_sb_evaluate_against_long_double(host_lib, degrees):
    body = _eval_body(degrees, 40 + sum(degrees))
    B = cp.Body(body)
    rng = np.random.default_rng(3)
    lo, hi = B.lo.astype(float), B.hi.astype(float)
    pd = len(degrees)
    # random points, the two ends and every interior knot of every direction (crossed with random values of the other)
    xi = [lo + (hi - lo) * rng.uniform(size=(200, pd))]
    for k in range(pd):
        special = np.unique(np.asarray(body["knots"][k]))
        pts = lo + (hi - lo) * rng.uniform(size=(len(special), pd))
        pts[:, k] = special
        xi.append(pts)
    xi.append(np.array([lo, hi]))
    xi = np.concatenate(xi)
    S, S1, S2 = host_evaluate(host_lib, body, xi)
    R, R1, R2 = B.evaluate(xi)
    # where S2 is continuous: off the knots, and on a knot of multiplicity m only if degree - m >= 2
    smooth = np.ones(len(xi), dtype=bool)
    for k, p in enumerate(degrees):
        U = np.asarray(body["knots"][k])
        for kn in np.unique(U)[1:-1]:
            if p - int((U == kn).sum()) < 2:
                smooth &= xi[:, k] != kn
    assert smooth.sum() > 200 and bool((~smooth).any()) == (min(degrees) <= 3)      # (degree 5 is C3 on a doubled knot)
    # rounding of the recursion: a few ulp of the values, times p / (smallest knot span) per derivative
    scale = float(np.abs(body["control_points"]).max())
    span = min(float(np.diff(np.unique(np.asarray(k))).min()) for k in body["knots"])
    amp = max(degrees) / span
    errs = (float(np.abs(S - R).max()) / scale, float(np.abs(S1 - R1).max()) / (scale * amp),
            float(np.abs(S2[smooth] - R2[smooth]).max()) / (scale * amp ** 2))
    print("sb_evaluate", degrees, "relative errors of S, S1, S2:", errs)
    assert max(errs) < 1e-13            # measured: <= 4e-16 (S), 3e-16 (S1), 2e-16 (S2) in these units


# ---- sb_closest_point and sp_nearest against the brute-force reference -------------------------------------------------
def _band(B, n_xi, offsets, rng):
    """queries on a band around the body: foot points spread over the interior of the parametric box, moved along the
    body's normal to both sides"""
    lo, hi = B.lo.astype(float), B.hi.astype(float)
    xi = lo + (hi - lo) * (0.02 + 0.96 * rng.uniform(size=(n_xi, B.pd)))
    # next to the seam of a closed direction, on both sides of it and nearer to it than to any other of the body's samples
    for k in range(B.pd):
        if B.closed[k]:
            for t in (0.3, 0.01):
                for end in (lo[k] + t * (hi[k] - lo[k]) / (B.resolution - 1), hi[k] - t * (hi[k] - lo[k]) / (B.resolution - 1)):
                    extra = lo + (hi - lo) * (0.02 + 0.96 * rng.uniform(size=(2, B.pd)))
                    extra[:, k] = end
                    xi = np.concatenate([xi, extra])
    S, S1, _ = B.evaluate(xi)
    n = cp.body_normal(S1)
    return np.concatenate([(S + s * n).astype(np.float64) for s in offsets])


def _beyond(B, reach, offsets):
    """queries beyond the ends / edges / corners of an open body, on both sides"""
    lo, hi = B.lo.astype(float), B.hi.astype(float)
    out = []
    if B.pd == 1:
        for e, sign in ((lo, -1.0), (hi, 1.0)):
            S, S1, _ = B.evaluate(np.array([e]))
            t = S1[0, 0] / np.sqrt((S1[0, 0] ** 2).sum())
            n = cp.body_normal(S1)[0]
            out += [(S[0] + sign * r * t + s * n).astype(np.float64) for r in reach for s in offsets]
    else:
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                if (a, b) == (0, 0):
                    continue
                xi = np.array([[(lo[0] + hi[0]) / 2 if a == 0 else (lo[0] if a < 0 else hi[0]),
                                (lo[1] + hi[1]) / 2 if b == 0 else (lo[1] if b < 0 else hi[1])]])
                S, S1, _ = B.evaluate(xi)
                t0, t1 = (S1[0, k] / np.sqrt((S1[0, k] ** 2).sum()) for k in range(2))
                n = cp.body_normal(S1)[0]
                out += [(S[0] + r * (a * t0 + b * t1) + s * n).astype(np.float64) for r in reach for s in offsets]
    return np.array(out)


def _parabola_answer(body, xq):
    """closest point of y = y0 + a (x - xc)^2: the real roots of 2 a^2 t^3 + (1 - 2 a v) t - h = 0 (t = x - xc, (h, v) the
    query relative to the vertex), polished by Newton in long double, the nearest taken"""
    xc, y0, a = (LD(v) for v in body["parabola"])
    dist = []
    for q in xq:
        h, v = LD(q[0]) - xc, LD(q[1]) - y0
        roots = np.roots([float(2 * a * a), 0.0, float(1 - 2 * a * v), float(-h)])
        best = None
        for t in roots[np.abs(roots.imag) < 1e-9].real.astype(LD):
            for _ in range(6):
                t = t - (2 * a * a * t ** 3 + (1 - 2 * a * v) * t - h) / (6 * a * a * t * t + (1 - 2 * a * v))
            d = np.sqrt((t - h) ** 2 + (a * t * t - v) ** 2)
            best = d if best is None or d < best else best
        dist.append(best)
    return np.array(dist, dtype=LD)


def _pointwise_cases():
    L2, L3 = np.array([6.0, 3.0]), np.array([4.0, 4.0, 2.0])
    rng = np.random.default_rng(17)
    out = {}
    for name, make in sb.BODIES_2D.items():
        body = make(L2.copy())
        B = cp.Body(body)
        q = _band(B, 40, (-0.12, -0.01, 0.02, 0.2), rng)
        if name == "open-arc":
            q = np.concatenate([q, _beyond(B, (0.05, 0.4, 1.5), (-0.1, 0.15))])
        out[name] = (body, B, q)
    for name, make in sb.BODIES_3D.items():
        body = make(L3.copy())
        B = cp.Body(body)
        q = _band(B, 30, (-0.08, -0.01, 0.02, 0.15), rng)
        if name in ("small-dome", "sphere-patch"):
            q = np.concatenate([q, _beyond(B, (0.05, 0.5), (-0.05, 0.1))])
        out[name] = (body, B, q)
    return out


_POINTWISE = {}


def pointwise(name):
    """(body, Body, queries, brute-force answer): computed once, shared"""
    if not _POINTWISE:
        _POINTWISE.update(_pointwise_cases())
    if len(_POINTWISE[name]) == 3:
        body, B, q = _POINTWISE[name]
        _POINTWISE[name] = (body, B, q, cp.closest(B, q))
    return _POINTWISE[name]


ALL_BODIES = list(sb.BODIES_2D) + list(sb.BODIES_3D)

# True gap, distance and the NORMAL component of S, relative to the size of the body (max |control point|): the largest
# oracle-vs-reference difference over the queries of pointwise(name) was measured as 3.6e-16 (circle-seam-down; every
# body lies between 7.6e-17 and 3.6e-16) -> the floor, 1e-13
POINT_BOUND = sb.bound(3.6e-16)
# xi and the TANGENTIAL part of S carry the square root of the distance's accuracy: the search moves while the squared
# distance does not grow, and that is flat to rounding within |d xi| ~ sqrt(eps) of the foot point -- a property of the
# scheme, not an error of the gap, which is of second order in it.  So these two take 10 x their measured difference
# without the floor or the cap of the gap's bound.  xi, where the reference's Hessian is well conditioned, relative to
# the parametric range, host harness against reference: measured <= 4.3e-9 (sphere-patch; 1.8e-16 for the flat curve of
# degree 1, whose Newton step is exact).  |S - S_ref| relative to the size of the body, oracle against reference:
# measured <= 2.2e-9 (sphere-patch).
XI_BOUND = 10 * 4.3e-9
TANGENTIAL_BOUND = 10 * 2.2e-9


@pytest.mark.parametrize("name", [n for n in ALL_BODIES if "dome" not in n])
def test_reference_closest_point_against_closed_form(name):
    """the brute-force reference itself, where the answer is known in closed form (every body but the domes, where the
    polish's own KKT check is the witness)"""
    body, B, xq, ref = pointwise(name)
    q = xq.astype(LD)
    twin = body.get("twin")
    if name == "parabola":
        exact = _parabola_answer(body, xq)
    elif name.startswith("cylinder"):
        d = q - body["axis_point"].astype(LD)
        d = d - (d @ body["axis_dir"].astype(LD))[:, None] * body["axis_dir"].astype(LD)
        exact = np.abs(np.sqrt((d * d).sum(axis=1)) - LD(body["radius"]))
    elif twin is not None and twin["kind"] == "plane":
        exact = np.abs((q - np.asarray(twin["point"], dtype=LD)) @ np.asarray(twin["normal"], dtype=LD))
    elif twin is not None and name != "open-arc" and name != "sphere-patch":
        d = q - np.asarray(twin["center"], dtype=LD)
        exact = np.abs(np.sqrt((d * d).sum(axis=1)) - LD(twin["radius"]))
    elif twin is not None:
        # a piece of the circle / sphere: the analytic answer where the foot point is not clipped
        free = ~ref.pinned.any(axis=1)
        assert free.sum() > 20 and (~free).sum() > 4
        d = q - np.asarray(twin["center"], dtype=LD)
        exact = np.abs(np.sqrt((d * d).sum(axis=1)) - LD(twin["radius"]))
        assert np.all(ref.distance[~free] > exact[~free] + 1e-6)              # clipped: farther than the full circle
        exact = np.where(free, exact, ref.distance)
    else:
        raise AssertionError("no closed form for " + name)
    err = float(np.abs(ref.distance - exact).max())
    print(name, "reference against closed form:", err)
    # the control points and weights are doubles (sqrt(1/2), the tilted normal): the body is the analytic one to ~1e-16
    assert err < 2e-15 * float(np.abs(body["control_points"]).max())


@pytest.mark.parametrize("name", ALL_BODIES)
@pytest.mark.parametrize("which", ["host", "oracle"])
def test_closest_point_against_brute_force(host_lib, which, name):
    body, B, xq, ref = pointwise(name)
    # preconditions, on the reference alone
    assert np.all(ref.distance > 0)
    assert np.all(ref.margin >= B.sample_spacing())
    if name in sb.CLIPPING:
        assert ref.pinned.any(axis=1).sum() > 4
        if B.pd == 2:
            assert (ref.pinned.sum(axis=1) == 1).any() and (ref.pinned.sum(axis=1) == 2).any()     # edges and corners
    xi, S, g, d = host_closest(host_lib, body, xq) if which == "host" else oracle_closest(body, xq)
    n = cp.body_normal(ref.S1)
    pmq = ref.S - xq.astype(LD)
    g_ref = -(n * pmq).sum(axis=1)
    scale = float(np.abs(body["control_points"]).max())
    dS = S - ref.S
    errs = (float(np.abs((dS * n).sum(axis=1)).max()) / scale, float(np.abs(g - g_ref).max()) / scale,
            float(np.abs(d - ref.distance).max()) / scale)
    tangential = float(np.sqrt((dS * dS).sum(axis=1)).max()) / scale
    wc = ref.well_conditioned
    assert wc.sum() > 20
    dxi = np.abs(xi - ref.xi)[wc]
    for k in range(B.pd):
        period = float(B.hi[k] - B.lo[k])
        if B.closed[k]:
            dxi[:, k] = np.minimum(dxi[:, k], period - dxi[:, k])       # the seam is one point with two names
        dxi[:, k] /= period
    print(which, name, "S along the normal, gap, distance:", errs, "|S - S_ref|:", tangential, "xi:", float(dxi.max()))
    assert max(errs) < POINT_BOUND
    assert tangential < TANGENTIAL_BOUND
    assert float(dxi.max()) < XI_BOUND
    if name in sb.CLIPPING:
        # end-clipped: the end point comes back, with an angle far above the tolerance
        pin = ref.pinned.any(axis=1)
        angle = np.arccos(np.minimum(np.abs(g[pin]) / d[pin], 1.0))
        assert angle.min() > 1e-2


# ---- ContactOracle against nodal_gap_area on the blocks of the GPU tests ---------------------------------------------
@pytest.mark.parametrize("case", sb.CASES, ids=sb.CASE_IDS)
def test_oracle_nodal_sums_against_reference(case):
    from oracle import ref_path as rp
    block, name = case
    cid = sb.CASE_IDS[sb.CASES.index(case)]
    P, patch, tables, u, body = sb.setup(block, name)
    B, ref = sb.reference(block, name)
    cp.check_conditions(ref, B, clipping=name in sb.CLIPPING)
    Cn = rp.ContactOracle(P, block[2], 1, body, penalty=1e4)
    r = np.zeros(P.n_vdofs)
    Cn.add_boundary_residual(u, r)
    assert np.array_equal(Cn.marked_nodes, ref.nodes)
    errs = (sb.rel(Cn.area, ref.area), sb.rel(Cn.gap, ref.gap), sb.rel(Cn.pressure, ref.pressure),
            sb.rel(Cn.gap_norm(u), ref.gap_norm))
    print(cid, "area, gap, pressure, GapNorm:", errs)
    assert sb.rel(Cn.last_area, ref.total_area) < 1e-13
    assert max(errs) < sb.bound(sb.MEASURED_NODAL[cid])


TWIN_CASES = [c for c, cid in zip(sb.CASES, sb.CASE_IDS) if cid in sb.MEASURED_TWIN]
TWIN_IDS = [cid for cid in sb.CASE_IDS if cid in sb.MEASURED_TWIN]


@pytest.mark.parametrize("case", TWIN_CASES, ids=TWIN_IDS)
def test_oracle_spline_body_equals_analytic_twin(case):
    """the spline IS the circle / sphere / plane: residual and exact tangent of the spline body equal the analytic body's.
    With a search that stops at the seam of a closed body the seam-down circle misses this by 0.23."""
    from oracle import ref_path as rp
    block, name = case
    cid = sb.CASE_IDS[sb.CASES.index(case)]
    P, patch, tables, u, body = sb.setup(block, name)
    rowptr, col = P.sparsity()
    out = []
    for b in (body, body["twin"]):
        Cn = rp.ContactOracle(P, block[2], 1, b, penalty=1e4, rowptr=rowptr, col=col)
        r, A = np.zeros(P.n_vdofs), np.zeros(rowptr[-1])
        Cn.add_boundary_residual_and_grad(u, 0.6, r, A, rp.TANGENT_EXACT)
        out.append((r, A))
    assert np.abs(out[1][0]).max() > 0
    errs = (sb.rel(out[0][0], out[1][0]), sb.rel(out[0][1], out[1][1]))
    print(cid, "residual, tangent against the analytic twin:", errs)
    assert max(errs) < sb.bound(sb.MEASURED_TWIN[cid])


def test_closed_directions_are_found_at_set_up(host_lib):
    """sb_fill_host decides `closed` from the samples: the circle and the circular direction of the cylinder, nothing else"""
    L2, L3 = np.array([6.0, 3.0]), np.array([4.0, 4.0, 2.0])
    for bodies, L in ((sb.BODIES_2D, L2), (sb.BODIES_3D, L3)):
        for name, make in bodies.items():
            body = make(L.copy())
            st = product_body(body)
            s = st.c_struct()
            closed = (C.c_int * 2)()
            host_lib.host_sb_closed(C.byref(s), len(L), closed)
            assert list(closed)[:len(body["degrees"])] == [int(c) for c in cp.Body(body).closed], name
            assert bool(closed[0]) == name.startswith(("circle", "cylinder")) and not closed[1]
