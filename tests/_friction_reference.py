"""Coulomb friction of the mortar contact integrator (csrc/kernels_face_friction.hpp) in numpy long double, on the points,
normals and nodal pressures of tests/_face_reference.py -- written from the model, sharing no code with the kernels.

    at a face point   p_N = -p_h = -sum_A N_A p_A (p_A: mortar_contact's nodal pressures); committed state (xi, xbar, c)
      p_N = 0            t = 0, trial (xi' = 0, c' = 0)
      p_N > 0, c = 0     t = 0, trial (xi' = 0, c' = 1)
      p_N > 0, c = 1     a = xi + x_q - xbar - d,  s = (I - n n^T) a
                           stick  eps_T |s| <= mu p_N:  t = eps_T s,          xi' = s
                           slip   otherwise:            t = mu p_N s / |s|,   xi' = t / eps_T          c' = 1
      xbar' = x_q in every branch
    residual          r_Ai = sum_q w |m| N_A t_i
    tangent           K_AiBj = grad_factor sum_q w N_A (t_i n_k D_kBj + |m| dt_i/dx_Bj), D = dm/dx (_cross_matrix), with p_A, xi,
                      xbar, d, c and the branch frozen:  d|m| = n_k D_kBj,  dn_i = (delta_ik - n_i n_k) D_kBj / |m|,
                      ds_i = (delta_ij - n_i n_j) N_B - dn_i (n . a) - n_i dn_k a_k,
                      stick dt = eps_T ds,  slip dt_i = (mu p_N / |s|) (delta_ik - sh_i sh_k) ds_k,  sh = s / |s|

Points are in the order of the face basis (no face numbering); vectors [n_nodes * dim] node-major, K dense."""
import types

import numpy as np

import _face_reference as fr

LD = np.longdouble


def initial_state(n_points, dim):
    return types.SimpleNamespace(xi=np.zeros((n_points, dim), dtype=LD), xbar=np.zeros((n_points, dim), dtype=LD),
                                 c=np.zeros(n_points, dtype=bool))


def point_pressure(pts, contact):
    """p_h at the points from the nodal pressures of fr.mortar_contact(pts, ...)"""
    return fr.point_pressure(pts.fb, contact.pressure, contact.nodes)


def tractions(pts, ph, state, mu, eps_t, d=None, branch=None):
    """the state machine at the points: a, s, |s|, t, the branch (0 none, 1 stick, 2 slip; `branch` given: frozen to it,
    for difference quotients) and the trial state"""
    dim = pts.fb.dim
    mu, eps_t = LD(mu), LD(eps_t)
    d = np.zeros(dim, dtype=LD) if d is None else np.asarray(d, dtype=LD)
    pn = -np.asarray(ph, dtype=LD)
    on = (pn > 0) & state.c
    a = state.xi + pts.x - state.xbar - d
    s = a - pts.n * np.einsum("qi,qi->q", pts.n, a)[:, None]
    sn = np.linalg.norm(s, axis=-1)
    if branch is None:
        branch = np.where(on, np.where(eps_t * sn <= mu * pn, 1, 2), 0)
    safe = np.where(sn > 0, sn, LD(1))
    sh = s / safe[:, None]
    t = np.zeros_like(s)
    t[branch == 1] = eps_t * s[branch == 1]
    t[branch == 2] = (mu * pn[:, None] * sh)[branch == 2]
    xi_new = np.zeros_like(s)
    xi_new[branch == 1] = s[branch == 1]
    xi_new[branch == 2] = t[branch == 2] / eps_t
    trial = types.SimpleNamespace(xi=xi_new, xbar=pts.x.copy(), c=pn > 0)
    ratio = np.where(on, eps_t * sn / np.where(pn > 0, mu * pn, LD(1)), LD(0))      # 1 on the kink
    return types.SimpleNamespace(pn=pn, on=on, a=a, s=s, sn=sn, sh=sh, t=t, branch=branch, trial=trial, ratio=ratio)


def residual(pts, tr):
    return fr._nodal_vector(pts.fb, pts.da[:, None] * tr.t)


def tangent(pts, tr, mu, eps_t, grad_factor=1.0):
    fb = pts.fb
    dim = fb.dim
    mu, eps_t = LD(mu), LD(eps_t)
    sup = fr._support(fb)
    D = fr._cross_matrix(dim, pts.sign, pts.t, fb.dN[:, fb.tang, :][:, :, sup])            # [q, B, k, j]
    n, length = pts.n, np.linalg.norm(pts.m, axis=-1)
    dlen = np.einsum("qk,qbkj->qbj", n, D)
    dn = (D - n[:, None, :, None] * dlen[:, :, None, :]) / length[:, None, None, None]     # [q, B, i, j]
    na = np.einsum("qi,qi->q", n, tr.a)
    proj = np.eye(dim, dtype=LD)[None] - n[:, :, None] * n[:, None, :]
    ds = (proj[:, None, :, :] * fb.N[:, sup][:, :, None, None] - dn * na[:, None, None, None]
          - n[:, None, :, None] * np.einsum("qbkj,qk->qbj", dn, tr.a)[:, :, None, :])
    coef = np.where(tr.branch == 1, eps_t, np.where(tr.branch == 2, mu * tr.pn / np.where(tr.sn > 0, tr.sn, LD(1)), LD(0)))
    beta = (tr.branch == 2).astype(LD)
    dt = coef[:, None, None, None] * (ds - beta[:, None, None, None] * tr.sh[:, None, :, None]
                                      * np.einsum("qk,qbkj->qbj", tr.sh, ds)[:, :, None, :])
    Ks = np.einsum("q,qa,qbij->aibj", fb.w, fb.N[:, sup],
                   tr.t[:, None, :, None] * dlen[:, :, None, :] + length[:, None, None, None] * dt)
    K = np.zeros((fb.n_nodes * dim, fb.n_nodes * dim), dtype=LD)
    vd = (sup[:, None] * dim + np.arange(dim)).ravel()
    K[np.ix_(vd, vd)] = LD(grad_factor) * Ks.reshape(len(vd), len(vd))
    return K


def evaluate(pts, contact, state, mu, eps_t, d=None, grad_factor=1.0, with_tangent=True):
    """one evaluation at the configuration of pts: residual, tangent, history sums and the trial state"""
    tr = tractions(pts, point_pressure(pts, contact), state, mu, eps_t, d)
    tn = np.linalg.norm(tr.t, axis=-1)
    return types.SimpleNamespace(tr=tr, trial=tr.trial, r=residual(pts, tr),
                                 K=tangent(pts, tr, mu, eps_t, grad_factor) if with_tangent else None,
                                 force=(pts.da[:, None] * tr.t).sum(axis=0), traction=(pts.da * tn).sum(),
                                 n_stick=int((tr.branch == 1).sum()), n_slip=int((tr.branch == 2).sum()))
