"""The boundary faces of a tensor-product B-spline patch and what the three boundary integrators (csrc/contact.hip,
csrc/pressure.hip, csrc/surface.hip) sum over them, in numpy long double -- written from the definitions, from plain arrays
(degrees, knot vectors, control points + displacement, axis, side, quadrature order), sharing neither code nor scheme with
mimi_amd.splines.face_tables, oracle.iga.Patch.face_tables or the kernels.

    basis        Cox-de Boor recursion over ALL functions of an axis, N_{i,0} = [U_i <= x < U_{i+1}] (the upper end belongs
                 to the last non-empty span), 0/0 = 0; N'_{i,p} = p (N_{i,p-1} / (U_{i+p} - U_i) - N_{i+1,p-1} / (U_{i+p+1} -
                 U_{i+1})).  No span index, no element connectivity: a face point carries the dense vectors N_A and
                 dN_A / dxi_d (d = every direction of the VOLUME map) over all nodes of the patch, A = A0 + n0 (A1 + n1 A2).
    quadrature   Gauss-Legendre, order // 2 + 1 points per direction on every non-empty knot span, order = 2 max(degrees) + 3
                 by default (include/mimi_hip.h); the nodes of numpy's leggauss polished by Newton on the Legendre recurrence
                 in long double, the weights 2 / ((1 - x^2) P_n'(x)^2) recomputed from them, scaled by the span lengths.
    normal       m = +-(t_1 x t_2) (3-D) or +-(t_y, -t_x) (2-D) from the tangents d x / d xi_t on the face, the tangential
                 directions in ascending order; the sign is the one with m . (d x / d xi_axis) (side ? +1 : -1) > 0 -- the
                 through-face derivative is information no face table holds -- asserted away from zero at every point.
    sums         order-free nodal sums over all points of the face (no face numbering): follower pressure (residual, dense
                 tangent, area, force), coupling surface (points, nodal load), mortar contact against an analytic plane or
                 sphere (integrators/mortar_contact.cpp:148-261, mortar_contact.hpp:99-134: nodal area and gap, pressure,
                 residual, frozen-pressure tangent, GapNorm, last_area / last_force / last_pressure).  A face whose nodal
                 pressures are all zero has p_h = 0 on it, so the sums need no IsPressureZero rule.

Vectors are [n_nodes * dim], node-major (entry A * dim + i); the tangents are dense [n_vdofs, n_vdofs]."""
import functools
import types

import numpy as np

LD = np.longdouble


# ---- basis ---------------------------------------------------------------------------------------------------------------
def basis_table(U, p, x):
    """tabs[d][:, i] = N_{i,d}(x) for d = 0 .. p and every i, straight from the Cox-de Boor definition"""
    U, x = np.asarray(U, dtype=LD), np.asarray(x, dtype=LD)
    m = len(U)
    N0 = np.zeros((len(x), m - 1), dtype=LD)
    nonempty = [i for i in range(m - 1) if U[i] < U[i + 1]]
    for i in nonempty:
        N0[:, i] = (U[i] <= x) & (x < U[i + 1])
    N0[x == U[-1], nonempty[-1]] = 1
    tabs = [N0]
    for d in range(1, p + 1):
        prev, Nd = tabs[-1], np.zeros((len(x), m - d - 1), dtype=LD)
        for i in range(m - d - 1):
            a, b = U[i + d] - U[i], U[i + d + 1] - U[i + 1]
            if a > 0:
                Nd[:, i] += (x - U[i]) / a * prev[:, i]
            if b > 0:
                Nd[:, i] += (U[i + d + 1] - x) / b * prev[:, i + 1]
        tabs.append(Nd)
    return tabs


def basis_and_derivative(U, p, x):
    """(N[:, i], N'[:, i]) of all len(U) - p - 1 functions of degree p at the parameters x"""
    U = np.asarray(U, dtype=LD)
    tabs = basis_table(U, p, x)
    N = tabs[p]
    dN = np.zeros_like(N)
    if p >= 1:
        low = tabs[p - 1]
        for i in range(N.shape[1]):
            a, b = U[i + p] - U[i], U[i + p + 1] - U[i + 1]
            if a > 0:
                dN[:, i] += p / a * low[:, i]
            if b > 0:
                dN[:, i] -= p / b * low[:, i + 1]
    return N, dN


# ---- quadrature ----------------------------------------------------------------------------------------------------------
def gauss_legendre(n):
    """n-point Gauss-Legendre rule on [-1, 1] in long double"""
    x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for _ in range(4):
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    dp = n * (x * p1 - p0) / (x * x - 1)
    return x, 2 / ((1 - x * x) * dp * dp)


def rule_on_spans(U, p, nq):
    """(points, weights) of the nq-point rule on every non-empty knot span of U, spans ascending"""
    U = np.asarray(U, dtype=LD)
    x, w = gauss_legendre(nq)
    xs, ws = [], []
    for i in range(len(U) - 1):
        h = U[i + 1] - U[i]
        if h > 0:
            xs.append(U[i] + (x + 1) / 2 * h)
            ws.append(w / 2 * h)
    return np.concatenate(xs), np.concatenate(ws)


def points_per_direction(degrees, order=-1):
    return (2 * max(degrees) + 3 if order < 0 else order) // 2 + 1


def _dense(factors):
    """[n_points, n_nodes] from per-direction [n_points, n_d]: the first direction fastest"""
    out = factors[0]
    for f in factors[1:]:
        out = (f[:, :, None] * out[:, None, :]).reshape(len(out), -1)
    return out


def _point_tables(degrees, knots, params, weights):
    """dense N [q, A], dN [q, d, A] at the tensor grid of the per-direction parameter lists (first direction fastest) and
    the product weights"""
    dim = len(degrees)
    grids = np.meshgrid(*[np.arange(len(x)) for x in params], indexing="ij")
    idx = [g.ravel(order="F") for g in grids]
    BD = [basis_and_derivative(knots[d], degrees[d], params[d]) for d in range(dim)]
    B = [BD[d][0][idx[d]] for d in range(dim)]
    D = [BD[d][1][idx[d]] for d in range(dim)]
    N = _dense(B)
    dN = np.stack([_dense([D[k] if k == d else B[k] for k in range(dim)]) for d in range(dim)], axis=1)
    w = np.ones(len(N), dtype=LD)
    for d in range(dim):
        w = w * weights[d][idx[d]]
    return N, dN, w


def _key(degrees, knots):
    return tuple(int(p) for p in degrees), tuple(tuple(float(v) for v in k) for k in knots)


@functools.lru_cache(maxsize=None)
def _face_basis(degrees, knots, axis, side, order):
    dim = len(degrees)
    nq = points_per_direction(degrees, order)
    params, weights = [], []
    for d in range(dim):
        if d == axis:
            params.append(np.array([knots[d][-1] if side else knots[d][0]], dtype=LD))
            weights.append(np.ones(1, dtype=LD))
        else:
            x, w = rule_on_spans(knots[d], degrees[d], nq)
            params.append(x)
            weights.append(w)
    N, dN, w = _point_tables(degrees, knots, params, weights)
    for a in (N, dN, w):
        a.setflags(write=False)
    n_ctrl = [len(k) - p - 1 for k, p in zip(knots, degrees)]
    return types.SimpleNamespace(dim=dim, axis=axis, side=side, N=N, dN=dN, w=w, n_nodes=int(np.prod(n_ctrl)), n_ctrl=n_ctrl,
                                 tang=[d for d in range(dim) if d != axis], n_q_face=nq ** (dim - 1))


def face_basis(degrees, knots, axis, side, order=-1):
    """the quadrature points of the face {xi_axis = end}: dense N [q, A], dN [q, d, A] (d over ALL directions) and the
    weights scaled by the span lengths.  Cached; never modified."""
    return _face_basis(*_key(degrees, knots), int(axis), int(side), int(order))


@functools.lru_cache(maxsize=None)
def _volume_basis(degrees, knots, order):
    nq = points_per_direction(degrees, order)
    rules = [rule_on_spans(k, p, nq) for k, p in zip(knots, degrees)]
    return _point_tables(degrees, knots, [r[0] for r in rules], [r[1] for r in rules])


def volume(degrees, knots, x, order=-1):
    """sum_q w det(dx / dxi) over the whole patch, with the same basis routine"""
    N, dN, w = _volume_basis(*_key(degrees, knots), int(order))
    G = np.einsum("qdA,Ai->qid", dN, np.asarray(x, dtype=LD))
    if G.shape[1] == 2:
        det = G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]
    else:
        det = np.einsum("qi,qi->q", G[:, :, 0], np.cross(G[:, :, 1], G[:, :, 2]))
    return (w * det).sum()


def face_node_ids(n_ctrl, axis, side):
    """sorted ids of the nodes whose index along `axis` is the first / last"""
    idx = np.arange(int(np.prod(n_ctrl)))
    for d, n in enumerate(n_ctrl):
        if d == axis:
            return np.nonzero(idx % n == (n - 1 if side else 0))[0]
        idx = idx // n


# ---- the points of a configuration ---------------------------------------------------------------------------------------
def _cross_matrix(dim, sign, t, dN_t):
    """D[q, B, i, j] = d m_i / d x_Bj of m = sign (t_1 x t_2) or sign (t_y, -t_x), t_k = sum_B dN_t[q, k, B] x_B"""
    nq, _, nb = dN_t.shape
    D = np.zeros((nq, nb, dim, dim), dtype=LD)
    if dim == 2:
        D[:, :, 0, 1] = dN_t[:, 0, :]
        D[:, :, 1, 0] = -dN_t[:, 0, :]
    else:
        eye = np.eye(3, dtype=LD)
        for j in range(3):
            e_x_t2 = np.cross(eye[j][None, :], t[:, 1, :])           # [q, i]
            t1_x_e = np.cross(t[:, 0, :], eye[j][None, :])
            D[:, :, :, j] = dN_t[:, 0, :, None] * e_x_t2[:, None, :] + dN_t[:, 1, :, None] * t1_x_e[:, None, :]
    return sign[:, None, None, None] * D


def face_points(fb, x):
    """the points of the face basis fb on the configuration x [n_nodes, dim] (control points + displacement): position,
    volume-map derivatives, the outward non-normalised normal m, unit normal n, da = w |m|"""
    x = np.asarray(x, dtype=LD).reshape(fb.n_nodes, fb.dim)
    xq = fb.N @ x
    G = np.einsum("qdA,Ai->qdi", fb.dN, x)                           # d x_i / d xi_d
    t = G[:, fb.tang, :]
    if fb.dim == 2:
        m = np.stack([t[:, 0, 1], -t[:, 0, 0]], axis=-1)
    else:
        m = np.cross(t[:, 0, :], t[:, 1, :])
    through = np.einsum("qi,qi->q", m, G[:, fb.axis, :]) * (1 if fb.side else -1)
    size = np.linalg.norm(m, axis=-1) * np.linalg.norm(G[:, fb.axis, :], axis=-1)
    assert np.all(np.abs(through) > 1e-3 * size), "the face normal is nearly tangent to the through-face direction"
    sign = np.where(through > 0, LD(1), LD(-1))
    m = sign[:, None] * m
    length = np.linalg.norm(m, axis=-1)
    return types.SimpleNamespace(fb=fb, x=xq, G=G, t=t, sign=sign, m=m, n=m / length[:, None], da=fb.w * length)


def _support(fb):
    """the nodes some face point sees (from the values, not from an index rule)"""
    return np.nonzero(np.any(fb.N != 0, axis=0) | np.any(fb.dN[:, fb.tang, :] != 0, axis=(0, 1)))[0]


def _nodal_vector(fb, wv):
    """sum_q wv[q, i] N_A: [n_nodes * dim]"""
    return np.einsum("qA,qi->Ai", fb.N, wv).reshape(-1)


def _tangent(pts, wp):
    """sum_q wp[q] N_A d m_i / d x_Bj, dense [n_vdofs, n_vdofs]"""
    fb = pts.fb
    dim = fb.dim
    sup = _support(fb)
    D = _cross_matrix(dim, pts.sign, pts.t, fb.dN[:, fb.tang, :][:, :, sup])
    Ks = np.einsum("q,qa,qbij->aibj", wp, fb.N[:, sup], D)
    K = np.zeros((fb.n_nodes * dim, fb.n_nodes * dim), dtype=LD)
    vd = (sup[:, None] * dim + np.arange(dim)).ravel()
    K[np.ix_(vd, vd)] = Ks.reshape(len(vd), len(vd))
    return K


# ---- follower pressure ---------------------------------------------------------------------------------------------------
def point_pressure(fb, pressure, nodes=None):
    """p at the points: a scalar, or values at the sorted face nodes `nodes` (p_h = sum_A N_A p_A)"""
    if np.isscalar(pressure):
        return np.full(len(fb.w), LD(pressure))
    pa = np.zeros(fb.n_nodes, dtype=LD)
    pa[nodes] = np.asarray(pressure, dtype=LD)
    return fb.N @ pa


def follower_pressure(pts, pressure, nodes=None, with_tangent=True):
    """residual sum w p N_A m_i, tangent sum w p N_A dm_i / dx_Bj, area sum w |m|, force -sum w p m"""
    fb = pts.fb
    wp = fb.w * point_pressure(fb, pressure, nodes)
    r = _nodal_vector(fb, wp[:, None] * pts.m)
    K = _tangent(pts, wp) if with_tangent else None
    return types.SimpleNamespace(r=r, K=K, area=pts.da.sum(), force=-(wp[:, None] * pts.m).sum(axis=0))


# ---- coupling surface ----------------------------------------------------------------------------------------------------
def surface_load(pts, t):
    """sum_q da_q t[q, i] N_A for a traction per unit current area at the points (in the order of pts)"""
    return _nodal_vector(pts.fb, pts.da[:, None] * np.asarray(t, dtype=LD))


def match_points(x_ref, x_other):
    """perm with x_other[perm[q]] the point nearest to x_ref[q]; asserts that it is a bijection.  Returns (perm, largest
    distance)"""
    d = np.linalg.norm(np.asarray(x_ref, dtype=np.float64)[:, None, :] - np.asarray(x_other, dtype=np.float64)[None, :, :], axis=-1)
    perm = d.argmin(axis=1)
    assert len(x_ref) == len(x_other) and len(np.unique(perm)) == len(perm), "the point sets do not match one to one"
    return perm, d[np.arange(len(perm)), perm].max()


# ---- mortar contact against an analytic body -----------------------------------------------------------------------------
def body_gap(body, x):
    """g(x) of dict(kind="plane", point, normal (unit)) or dict(kind="sphere", center, radius): negative inside"""
    x = np.asarray(x, dtype=LD)
    if body["kind"] == "plane":
        return (x - np.asarray(body["point"], dtype=LD)) @ np.asarray(body["normal"], dtype=LD)
    return np.linalg.norm(x - np.asarray(body["center"], dtype=LD), axis=-1) - LD(body["radius"])


def mortar_contact(pts, body, penalty, grad_factor=1.0, with_tangent=True):
    fb = pts.fb
    dim = fb.dim
    nodes = face_node_ids(fb.n_ctrl, fb.axis, fb.side)
    g_true = body_gap(body, pts.x)
    g = np.minimum(g_true, 0)
    area = fb.N.T @ pts.da
    gap = fb.N.T @ (pts.da * g)
    assert np.all(area[nodes] > 0) and np.all(np.delete(area, nodes) == 0)
    pa = np.zeros(fb.n_nodes, dtype=LD)
    pa[nodes] = LD(penalty) * gap[nodes] / area[nodes]
    ph = fb.N @ pa
    wp = fb.w * ph
    r = -_nodal_vector(fb, wp[:, None] * pts.m)
    K = -LD(grad_factor) * _tangent(pts, wp) if with_tangent else None
    return types.SimpleNamespace(nodes=nodes, g=g_true, area=area[nodes], gap=gap[nodes], pressure=pa[nodes], r=r, K=K,
                                 gap_norm=np.sqrt((g * g).sum()), last_area=pts.da.sum(), last_force=(wp[:, None] * pts.m).sum(axis=0),
                                 last_pressure=(pts.da * ph).sum())
