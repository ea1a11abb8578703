"""Yardstick of the field output (tests/test_fields_*.py): pure numpy on the oracle, no product code.

At every quadrature point: F = I + grad u from the oracle patch's dN_dX tables and connectivity, P from
oracle.ref_path.point_pk1 with the state the DomainOracle holds (dt as given), sigma = P F^T / det F, the von Mises stress
q = sqrt(3/2) |sigma - tr(sigma)/dim I|_F (the trace over dim, as the reference's Dev, material_utils.hpp:33,44) and det F.
At the nodes: sum[A] = sum_e sum_q w det N_A f, weight[A] = sum_e sum_q w det N_A, with np.add.at over tables()["N"]."""
import functools

import numpy as np

FIELDS = ("cauchy_stress", "von_mises_stress", "det_F", "accumulated_plastic_strain", "temperature")
MATERIALS = ("neohook", "stvk", "j2", "j2linear", "j2simo", "j2log")
J2_MODELS = ("j2", "j2linear", "j2simo", "j2log")


def deformation_gradients(tables, u, dim):
    """F[e, q, i, J] = delta_iJ + sum_a u[conn[e, a], i] dN_dX[e, q, a, J]"""
    ue = np.asarray(u).reshape(-1, dim)[tables["conn"]]
    return np.eye(dim) + np.einsum("eai,eqaJ->eqiJ", ue, tables["dN_dX"])


def cauchy_of(Pk, F):
    return Pk @ F.T / np.linalg.det(F)


def von_mises_of(sig):
    dim = sig.shape[0]
    dev = sig - np.trace(sig) / dim * np.eye(dim)
    return np.sqrt(1.5) * np.linalg.norm(dev)


def point_fields(D, u, dt):
    """name -> [n_el, n_q, ncomp] from the oracle integrator D (its tables, material and committed state); the Cauchy
    stress column-major ([i + j dim]).  The two state fields only for a material that has state."""
    from oracle import ref_path as rp
    dim = D.patch.dim
    F = deformation_gradients(D.tables, u, dim)
    ne, nq = F.shape[:2]
    sig = np.zeros((ne, nq, dim * dim))
    q = np.zeros((ne, nq, 1))
    for e in range(ne):
        for k in range(nq):
            if D.has_states:
                Pk, _ = rp.point_pk1(D.material, F[e, k], dt, plastic_strain=D.plastic_strain[e, k].reshape(dim, dim).T,
                                     eqps=D.eqps[e, k], temperature=D.temperature[e, k],
                                     state2=D.state2[e, k].reshape(dim, dim).T)
            else:
                Pk, _ = rp.point_pk1(D.material, F[e, k], dt)
            s = cauchy_of(Pk, F[e, k])
            sig[e, k] = s.ravel(order="F")
            q[e, k, 0] = von_mises_of(s)
    out = {"cauchy_stress": sig, "von_mises_stress": q, "det_F": np.linalg.det(F)[..., None]}
    if D.has_states:
        out["accumulated_plastic_strain"] = D.eqps[..., None].copy()
        # J2Linear has no temperature: the second scalar of its state is created zero and never written
        # (materials.cpp:130-131, materials.hpp:153-160); the oracle's array for it is storage the material never reads
        from oracle.ref_path import MAT_J2LINEAR
        T = np.zeros_like(D.temperature) if D.material.kind == MAT_J2LINEAR else D.temperature
        out["temperature"] = T[..., None].copy()
    return out


def nodal_sums(tables, n_nodes, f):
    """(sum [n_nodes, ncomp], weight [n_nodes]) of point values f [n_el, n_q, ncomp]"""
    wd = tables["weight"] * tables["det"]
    N, conn = tables["N"], tables["conn"]
    s = np.zeros((n_nodes, f.shape[2]))
    w = np.zeros(n_nodes)
    np.add.at(w, conn, np.einsum("eq,eqa->ea", wd, N))
    np.add.at(s, conn, np.einsum("eq,eqa,eqc->eac", wd, N, f))
    return s, w


def nodal_fields(tables, n_nodes, fields):
    out = {}
    for name, f in fields.items():
        s, w = nodal_sums(tables, n_nodes, f)
        out[name] = s / w[:, None]
    return out


def lame():
    from _cases import POISSON, YOUNG
    return YOUNG * POISSON / ((1 + POISSON) * (1 - 2 * POISSON)), YOUNG / (2 * (1 + POISSON))


def closed_form_sigma(matname, F0):
    """neo-Hookean: mu/J (F F^T - I) + lambda (J - 1) I (materials.cpp:96-118); St. Venant-Kirchhoff: F S F^T / J with
    S = lambda tr(E) I + 2 mu E, E = (F^T F - I) / 2 (materials.cpp:72-94)"""
    lam, mu = lame()
    dim = F0.shape[0]
    J = np.linalg.det(F0)
    eye = np.eye(dim)
    if matname == "neohook":
        return mu / J * (F0 @ F0.T - eye) + lam * (J - 1.0) * eye
    E = 0.5 * (F0.T @ F0 - eye)
    S = lam * np.trace(E) * eye + 2.0 * mu * E
    return F0 @ S @ F0.T / J


def homogeneous_F(dim):
    G = np.array([[0.05, 0.02, -0.01], [0.01, -0.03, 0.02], [0.0, 0.015, 0.04]])
    return np.eye(dim) + G[:dim, :dim]


def homogeneous_u(ctrl, F0):
    """u_a = (F0 - I) X_a: control points at the Greville abscissae reproduce the affine map exactly"""
    dim = F0.shape[0]
    return (np.asarray(ctrl).reshape(-1, dim) @ (F0 - np.eye(dim)).T).ravel()


# ---- the committed state and the reference of one (shape, material), computed once --------------------------------------
DT = 0.05
SHAPES = {
    "3x4p2": ((3, 4), 2, None, "bspline"),
    "2x2p3": ((2, 2), 3, [5.0, 1.0], "bspline"),
    "2x2x2p1": ((2, 2, 2), 1, None, "bspline"),
    "4x3x3p2": ((4, 3, 3), 2, None, "bspline"),
    "4x4x5p3": ((4, 4, 5), 3, None, "bspline"),
    "3x2x2p2-tables": ((3, 2, 2), 2, None, "tables"),
}


@functools.lru_cache(maxsize=None)
def reference(shape, matname):
    """(oracle patch, oracle integrator with the committed state, u0 of the commit, u, point fields, nodal fields): commit
    synthetic_u(scale=0.03, seed=7), then u = synthetic_u(scale=0.02), dt = 0.05.  Shared and never modified."""
    from _cases import oracle_material, synthetic_u
    from oracle import iga, ref_path as rp
    n_el, p, lengths, _ = SHAPES[shape]
    P = iga.Patch.block(n_el, p, lengths)
    D = rp.DomainOracle(P, oracle_material(matname), n_threads=2)
    D.set_dt(DT)
    u0 = synthetic_u(P, scale=0.03, seed=7)
    if D.has_states:
        D.domain_post_time_advance(u0)
    u = synthetic_u(P, scale=0.02)
    pts = point_fields(D, u, DT)
    nod = nodal_fields(D.tables, P.n_nodes, pts)
    for a in list(pts.values()) + list(nod.values()) + [u0, u]:
        a.setflags(write=False)
    return P, D, u0, u, pts, nod
