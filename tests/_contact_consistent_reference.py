"""The consistent mortar-contact tangent (csrc/kernels_face_consistent.hpp), dense and in numpy long double, written from
the definitions on the points of tests/_face_reference.py (face_points) -- no face numbering, no incidence list, no kernel
code.  With w the quadrature weight, m the outward non-normalised normal, n = m / |m|, g = min(g_true, 0), chi = [g != 0],
nu the body's unit normal at the closest point (the gradient of the gap), N_i the dense basis values:

    A_i = sum_q w |m| N_i        G_i = sum_q w |m| g N_i        p_i = eps G_i / A_i        p_q = sum_i N_i p_i
    r(a,i) = -sum_q w p_q N_a m_i
    K_frozen (a,i),(b,j) = -sum_q w p_q N_a dm_i/dx_bj
    K_new    (a,i),(b,j) = -sum_q w N_a m_i dp_q/dx_bj,    dp_q = sum_i N_i dp_i,    dp_i = (eps dG_i - p_i dA_i) / A_i
    dA_i/dx_bj = sum_q w N_i d|m|/dx_bj,    dG_i/dx_bj = sum_q w N_i (d|m|/dx_bj g + |m| chi nu_j N_b),    d|m| = n . dm

K = grad_factor (K_frozen + K_new); K_abs is the same chain of products formed from the absolute values of every factor --
the scale without cancellation (eps dG - p dA cancels exactly for a uniform gap, so |K| itself can be far below what the
rounding of its terms is measured against)."""
import types

import numpy as np

import _face_reference as fr

LD = np.longdouble


def normal_derivative(pts):
    """D[q, B, i, j] = dm_i / dx_Bj over ALL nodes B, from the definition of m on the face's tangents"""
    fb = pts.fb
    dim = fb.dim
    dN = fb.dN[:, fb.tang, :]                                         # [q, k, B]
    nq, _, nb = dN.shape
    D = np.zeros((nq, nb, dim, dim), dtype=LD)
    if dim == 2:                                                      # m = sign (t_y, -t_x)
        D[:, :, 0, 1] = dN[:, 0, :]
        D[:, :, 1, 0] = -dN[:, 0, :]
    else:                                                             # m = sign t_1 x t_2
        eye = np.eye(3, dtype=LD)
        for j in range(3):
            first = np.cross(eye[j][None, :], pts.t[:, 1, :])         # e_j x t_2   [q, i]
            second = np.cross(pts.t[:, 0, :], eye[j][None, :])        # t_1 x e_j
            D[:, :, :, j] = dN[:, 0, :, None] * first[:, None, :] + dN[:, 1, :, None] * second[:, None, :]
    return pts.sign[:, None, None, None] * D


def body_normal(body, x):
    """nu [q, dim]: the gradient of fr.body_gap"""
    x = np.asarray(x, dtype=LD)
    if body["kind"] == "plane":
        return np.broadcast_to(np.asarray(body["normal"], dtype=LD), x.shape).copy()
    d = x - np.asarray(body["center"], dtype=LD)
    return d / np.linalg.norm(d, axis=-1)[:, None]


def spline_body_gap(body, x, angle_tol=1.0e-5):
    """(g_true, g, nu) at the points x of a rigid spline body of tests/_spline_bodies.py, through the long-double closest
    point of tests/_closest_point.py: g after min(., 0) and the angle rule (mortar_contact.cpp:172-181), nu the body's unit
    normal at the closest point"""
    import _closest_point as cp
    x = np.asarray(x, dtype=LD)
    c = cp.closest(cp.Body(body), x)
    nu = cp.body_normal(c.S1)
    pmq = c.S - x
    g_true = -(nu * pmq).sum(axis=1)
    g = np.where(cp._angle(nu, pmq, g_true) > LD(angle_tol), 0, np.minimum(g_true, 0))
    return g_true, g, nu


def consistent_contact(pts, body, penalty, grad_factor=1.0):
    """K, K_frozen, K_new, K_abs dense [n_vdofs, n_vdofs] in long double (all carry grad_factor), and g_true at the points.
    body: the plane / sphere dicts of _face_reference.body_gap, or a rigid spline body of tests/_spline_bodies.py"""
    fb = pts.fb
    dim, nn = fb.dim, fb.n_nodes
    eps, gf = LD(penalty), LD(grad_factor)
    nodes = fr.face_node_ids(fb.n_ctrl, fb.axis, fb.side)
    w, N = fb.w, fb.N[:, nodes]                                       # [q], [q, S]
    ns = len(nodes)
    D = normal_derivative(pts)[:, nodes]                              # [q, S, i, j]
    length = np.linalg.norm(pts.m, axis=-1)
    if body["kind"] == "spline":
        g_true, g, nu = spline_body_gap(body, pts.x)
    else:
        g_true = fr.body_gap(body, pts.x)
        g, nu = np.minimum(g_true, 0), body_normal(body, pts.x)
    chi = (g != 0).astype(LD)
    area = N.T @ (w * length)
    gap = N.T @ (w * length * g)
    p = eps * gap / area
    pq = N @ p
    out = types.SimpleNamespace(g_true=g_true, nodes=nodes)
    for name, f in (("plain", lambda a: a), ("abs", np.abs)):
        Da, na, ma = f(D), f(pts.n), f(pts.m)
        dlen = np.einsum("qi,qbij->qbj", na, Da).reshape(len(w), ns * dim)                     # d|m| / dx_bj   [q, (b j)]
        dx = (N[:, :, None] * (chi[:, None] * f(nu))[:, None, :]).reshape(len(w), ns * dim)    # chi nu_j N_b
        dA = (w[:, None] * N).T @ dlen                                                         # [S, (b j)]
        dG = (w[:, None] * N).T @ (dlen * f(g)[:, None] + length[:, None] * dx)
        if name == "plain":
            dp = (eps * dG - p[:, None] * dA) / area[:, None]
            pq_f = pq
        else:
            dp = (eps * dG + np.abs(p)[:, None] * dA) / area[:, None]
            pq_f = N @ np.abs(p)
        dpq = N @ dp                                                                           # [q, (b j)]
        left = (w[:, None, None] * N[:, :, None] * ma[:, None, :]).reshape(len(w), ns * dim)   # w N_a m_i   [q, (a i)]
        new = left.T @ dpq
        frozen = np.einsum("q,qa,qbij->aibj", w * pq_f, N, Da).reshape(ns * dim, ns * dim)
        sgn = LD(-1) if name == "plain" else LD(1)
        vd = (nodes[:, None] * dim + np.arange(dim)).ravel()
        for key, block in (("frozen", frozen), ("new", new)):
            K = np.zeros((nn * dim, nn * dim), dtype=LD)
            K[np.ix_(vd, vd)] = sgn * (gf if name == "plain" else abs(gf)) * block
            setattr(out, f"K_{key}" if name == "plain" else f"K_{key}_abs", K)
    out.K = out.K_frozen + out.K_new
    out.K_abs = out.K_frozen_abs + out.K_new_abs
    return out
