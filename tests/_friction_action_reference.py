"""Coulomb friction on the matrix-free route (csrc/kernels_face_friction_action.hpp), dense and in numpy long double, written
from the model on the points of tests/_face_reference.py -- no face numbering, no incidence list, no kernel code.

The frozen friction tangent is tests/_friction_reference.py's (`tangent`): p_A, the committed state, d and the branch frozen.
With the CONSISTENT contact tangent the nodal pressure is not frozen, and in slip the traction t = mu p_N s / |s| carries it:
p_N = -p_q, p_q = sum_i N_i p_i, so the residual r(a,i) = sum_q w |m| N_a t_i has the further term

    K_new (a,i),(b,j) = -sum_q w |m| N_a [slip] mu sh_i dp_q/dx_bj,      sh = s / |s|,

    dp_q = sum_i N_i dp_i,   dp_i = (eps dG_i - p_i dA_i) / A_i,   A_i = sum_q w |m| N_i,   G_i = sum_q w |m| g N_i,
    dA_i/dx_bj = sum_q w N_i d|m|/dx_bj,   dG_i/dx_bj = sum_q w N_i (d|m|/dx_bj g + |m| chi nu_j N_b),   d|m| = n . dm

(the definitions of tests/_contact_consistent_reference.py's docstring, recomputed here: that module does not hand out dp_i).
In stick t = eps_T s does not see the pressure.  The total tangent of contact + friction with the committed state frozen is
    frozen:      K_contact_frozen + K_friction
    consistent:  K_contact_consistent + K_friction + K_new
each the exact derivative of what it claims wherever no point sits on a switch (gap, contact flag, stick / slip kink)."""
import types

import numpy as np

import _contact_consistent_reference as ccr
import _face_reference as fr
import _friction_reference as fq

LD = np.longdouble


def pressure_rate(pts, body, penalty):
    """dp_q/dx_bj [q, (b j)] over the sorted face nodes b, with those nodes, N on them and g_true at the points"""
    fb = pts.fb
    dim = fb.dim
    eps = LD(penalty)
    nodes = fr.face_node_ids(fb.n_ctrl, fb.axis, fb.side)
    w, N = fb.w, fb.N[:, nodes]
    ns, nq = len(nodes), len(w)
    D = ccr.normal_derivative(pts)[:, nodes]                                   # dm_i/dx_bj   [q, b, i, j]
    length = np.linalg.norm(pts.m, axis=-1)
    g_true = fr.body_gap(body, pts.x)
    g = np.minimum(g_true, 0)
    chi = (g != 0).astype(LD)
    nu = ccr.body_normal(body, pts.x)
    area = N.T @ (w * length)
    p = eps * (N.T @ (w * length * g)) / area
    dlen = np.einsum("qi,qbij->qbj", pts.n, D).reshape(nq, ns * dim)            # d|m|/dx_bj
    dgap = (N[:, :, None] * (chi[:, None] * nu)[:, None, :]).reshape(nq, ns * dim)
    dA = (w[:, None] * N).T @ dlen
    dG = (w[:, None] * N).T @ (dlen * g[:, None] + length[:, None] * dgap)
    dp = (eps * dG - p[:, None] * dA) / area[:, None]
    return types.SimpleNamespace(nodes=nodes, N=N, dpq=N @ dp, g_true=g_true, pressure=p)


def new_part(pts, body, penalty, tr, mu, grad_factor=1.0):
    """K_new dense [n_vdofs, n_vdofs] for the tractions tr of _friction_reference.tractions at pts"""
    fb = pts.fb
    dim, nn = fb.dim, fb.n_nodes
    rate = pressure_rate(pts, body, penalty)
    nodes, N = rate.nodes, rate.N
    length = np.linalg.norm(pts.m, axis=-1)
    slip = (tr.branch == 2).astype(LD)
    left = ((fb.w * length * slip * LD(mu))[:, None, None] * N[:, :, None] * tr.sh[:, None, :]).reshape(len(fb.w), len(nodes) * dim)
    K = np.zeros((nn * dim, nn * dim), dtype=LD)
    vd = (nodes[:, None] * dim + np.arange(dim)).ravel()
    K[np.ix_(vd, vd)] = -LD(grad_factor) * (left.T @ rate.dpq)
    return K


def total_residual(pts, body, penalty, state, mu, eps_t, d=None, branch=None):
    """contact + friction residual at pts against the committed `state`, with the tractions (branch, contact set) it took"""
    contact = fr.mortar_contact(pts, body, penalty, with_tangent=False)
    tr = fq.tractions(pts, fq.point_pressure(pts, contact), state, mu, eps_t, d, branch)
    return types.SimpleNamespace(r=contact.r + fq.residual(pts, tr), tr=tr, g=contact.g)


def total_tangents(pts, body, penalty, state, mu, eps_t, d=None, grad_factor=1.0):
    """K_frozen, K (consistent), K_new dense in long double, all with grad_factor, and the tractions"""
    contact = fr.mortar_contact(pts, body, penalty, grad_factor)
    tr = fq.tractions(pts, fq.point_pressure(pts, contact), state, mu, eps_t, d)
    K_fric = fq.tangent(pts, tr, mu, eps_t, grad_factor)
    K_new = new_part(pts, body, penalty, tr, mu, grad_factor)
    cons = ccr.consistent_contact(pts, body, penalty, grad_factor)
    return types.SimpleNamespace(K_frozen=contact.K + K_fric, K=cons.K + K_fric + K_new, K_new=K_new, K_contact_new=cons.K_new,
                                 tr=tr, g=contact.g)
