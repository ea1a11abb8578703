"""Augmented-Lagrangian mortar contact (csrc/kernels_face_augmented.hpp and the AUG variants of csrc/contact.hip and
csrc/kernels_face_consistent.hpp), dense and in numpy long double, written from the law on the points of
tests/_face_reference.py (face_points, body_gap, _nodal_vector, _tangent) -- no face numbering, no incidence list, no kernel
code.  With w the quadrature weight, m the outward non-normalised normal, g the UNCLAMPED gap at the points (the analytic
bodies never meet the angle rule: their closest point lies along the normal), nu the body's unit normal, lambda_i <= 0:

    A_i = sum_q w |m| N_i     Gt_i = sum_q w |m| g N_i     gt_i = Gt_i / A_i     p_i = min(0, lambda_i + eps gt_i)
    r(a,i) = -sum_q w p_q N_a m_i,   p_q = sum_i N_i p_i
    K_frozen (a,i),(b,j) = -sum_q w p_q N_a dm_i/dx_bj
    K_new    (a,i),(b,j) = -sum_q w N_a m_i dp_q/dx_bj,   dp_i = [p_i < 0] eps (dGt_i - gt_i dA_i) / A_i
    dA_i/dx_bj = sum_q w N_i d|m|/dx_bj,   dGt_i/dx_bj = sum_q w N_i (d|m|/dx_bj g + |m| nu_j N_b),   d|m| = n . dm
    dlambda_i = p_i - lambda_i;  violation = max |dlambda_i| / eps,  norm = sqrt(sum A_i dlambda_i^2),
    n_active = #{p_i < 0},  max_lagrange = max |lambda_i| after the update (lambda_i <- p_i when applied)

K = grad_factor (K_frozen + K_new); K_abs is the same chain from the absolute values of every factor, the scale without
cancellation (as tests/_contact_consistent_reference.py).  `switch` is the smallest |lambda_i + eps gt_i|: the distance of
the nearest node from the kink of min(0, .)."""
import types

import numpy as np

import _face_reference as fr
from _contact_consistent_reference import body_normal, normal_derivative

LD = np.longdouble


def nodal_gap(pts, body):
    """(nodes, A_i, Gt_i) at the sorted face nodes, g_true at the points"""
    fb = pts.fb
    nodes = fr.face_node_ids(fb.n_ctrl, fb.axis, fb.side)
    g = fr.body_gap(body, pts.x)
    N = fb.N[:, nodes]
    return nodes, N.T @ pts.da, N.T @ (pts.da * g), g


def augmented_contact(pts, body, penalty, lam, grad_factor=1.0, with_tangent=True):
    """lam: the multipliers at the sorted face nodes (projected onto <= 0 here as on the device)"""
    fb = pts.fb
    dim, nn = fb.dim, fb.n_nodes
    eps, gf = LD(penalty), LD(grad_factor)
    nodes, area, gap, g = nodal_gap(pts, body)
    lam = np.minimum(np.asarray(lam, dtype=LD), 0)
    assert np.all(area > 0)
    gt = gap / area
    trial = lam + eps * gt
    p = np.minimum(trial, 0)
    active = p < 0
    pa = np.zeros(nn, dtype=LD)
    pa[nodes] = p
    ph = fb.N @ pa
    wp = fb.w * ph
    dl = p - lam
    out = types.SimpleNamespace(
        nodes=nodes, g=g, area=area, gap=gap, gt=gt, pressure=p, active=active, lam=lam, switch=float(np.abs(trial).min()),
        r=-fr._nodal_vector(fb, wp[:, None] * pts.m), last_area=pts.da.sum(), last_force=(wp[:, None] * pts.m).sum(axis=0),
        last_pressure=(pts.da * ph).sum(), dlambda=dl, violation=np.abs(dl).max() / eps, norm=np.sqrt((area * dl * dl).sum()),
        n_active=int(active.sum()), max_lagrange_applied=np.abs(p).max(), max_lagrange_kept=np.abs(lam).max())
    if not with_tangent:
        return out
    out.K_frozen = -gf * fr._tangent(pts, wp)
    w, N = fb.w, fb.N[:, nodes]
    ns = len(nodes)
    D = normal_derivative(pts)[:, nodes]                              # [q, S, i, j]
    length = np.linalg.norm(pts.m, axis=-1)
    nu = body_normal(body, pts.x)
    vd = (nodes[:, None] * dim + np.arange(dim)).ravel()
    for name, f in (("plain", lambda a: a), ("abs", np.abs)):
        Da, na, ma = f(D), f(pts.n), f(pts.m)
        dlen = np.einsum("qi,qbij->qbj", na, Da).reshape(len(w), ns * dim)                     # d|m| / dx_bj   [q, (b j)]
        dx = (N[:, :, None] * f(nu)[:, None, :]).reshape(len(w), ns * dim)                     # nu_j N_b
        dA = (w[:, None] * N).T @ dlen                                                         # [S, (b j)]
        dG = (w[:, None] * N).T @ (dlen * f(g)[:, None] + length[:, None] * dx)
        if name == "plain":
            dp = eps * (dG - gt[:, None] * dA) / area[:, None]
            pq_f = N @ p
        else:
            dp = eps * (dG + np.abs(gt)[:, None] * dA) / area[:, None]
            pq_f = N @ np.abs(p)
        dp = np.where(active[:, None], dp, 0)
        dpq = N @ dp                                                                           # [q, (b j)]
        left = (w[:, None, None] * N[:, :, None] * ma[:, None, :]).reshape(len(w), ns * dim)   # w N_a m_i   [q, (a i)]
        new = left.T @ dpq
        frozen = np.einsum("q,qa,qbij->aibj", w * pq_f, N, Da).reshape(ns * dim, ns * dim)
        sgn = LD(-1) if name == "plain" else LD(1)
        for key, block in (("frozen", frozen), ("new", new)):
            K = np.zeros((nn * dim, nn * dim), dtype=LD)
            K[np.ix_(vd, vd)] = sgn * (gf if name == "plain" else abs(gf)) * block
            setattr(out, f"K_{key}_dense" if name == "plain" else f"K_{key}_abs", K)
    # (the frozen part twice: through _face_reference._tangent and through the chain above)
    assert np.abs(out.K_frozen_dense - out.K_frozen).max() <= 1e-15 * max(float(np.abs(out.K_frozen).max()), 1e-300)
    out.K_new = out.K_new_dense
    out.K = out.K_frozen + out.K_new
    out.K_abs = out.K_frozen_abs + out.K_new_abs
    return out
