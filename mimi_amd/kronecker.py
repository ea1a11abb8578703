"""Host side of the fast-diagonalisation (Kronecker) preconditioner of the device Krylov solvers (csrc/kronecker.hpp;
Sangalli & Tani, "Isogeometric preconditioners based on fast solvers for the Sylvester equation").

On one tensor-product patch  J = M + fac0 K (+ fac1 C)  is replaced, per displacement component c, by

    P_c = rho (x)_d M_d + sum_d (fac0 e_cd + fac1 eta) K_d (x) (M of the other axes)

with the 1-D mass and stiffness matrices M_d, K_d of the patch's own B-spline basis (NURBS weights ignored) on an interval
of length L_d, the mean length of the control polygons along axis d, and  e_cd = lambda + 2 mu  for d == c, mu otherwise
(linear elasticity at F = I, the coupling between the components dropped).  What the device needs are the generalised
eigenpairs  K_d U = M_d U diag(lam),  U^T M_d U = I  per (component, axis): a Dirichlet face removes the boundary function
of its axis for the components it clamps, so the pairs differ between components.  On a periodic axis (periodic_axes) the
first and last basis function are one function: the 1-D matrices are the folded P1^T M_d P1, P1^T K_d P1 on n_d - 1 functions,
and the operator lives on the folded grid of integrators.periodic_node_map.  Nothing here touches the device."""
import numpy as np
import scipy.linalg

from . import splines


def matrices_1d(knots, degree):
    """(M, K) of the B-spline basis of `knots` on the UNIT interval (the knots rescaled to [0, 1]): M_ab = int N_a N_b,
    K_ab = int N_a' N_b', by the Gauss rule with degree + 1 points per span, which is exact for both"""
    knots = np.asarray(knots, dtype=np.float64)
    p = int(degree)
    n = len(knots) - p - 1
    total = knots[-1] - knots[0]
    spans, B, D, w = splines._tables_1d(knots, p, p + 1)       # D: derivative in the span's own [0, 1] coordinate
    M, K = np.zeros((n, n)), np.zeros((n, n))
    for e, s in enumerate(spans):
        h = (knots[s + 1] - knots[s]) / total
        sl = slice(s - p, s + 1)
        M[sl, sl] += h * np.einsum("q,aq,bq->ab", w, B[e], B[e])
        K[sl, sl] += np.einsum("q,aq,bq->ab", w, D[e], D[e]) / h
    return M, K


def axis_lengths(patch):
    """L_d: the mean length of the control polygons along axis d"""
    pts = patch.control_points.reshape(list(patch.n_ctrl[::-1]) + [patch.dim])      # [i2][i1][i0][xyz]
    out = []
    for d in range(patch.dim):
        steps = np.diff(pts, axis=patch.dim - 1 - d)
        out.append(float(np.linalg.norm(steps, axis=-1).sum(axis=patch.dim - 1 - d).mean()))
    return out


def folded_matrices(M, K):
    """P1^T M P1, P1^T K P1 of a periodic axis: the last basis function is the first one (P1 the n x (n - 1) 0/1 map with
    P1[n - 1, 0] = 1), so its row and column are added to the first's -- with few spans their cross terms land on the
    diagonal, which the two additions do by themselves"""
    out = []
    for A in (M, K):
        A = np.array(A, dtype=np.float64)
        A[0, :] += A[-1, :]
        A[:, 0] += A[:, -1]
        out.append(np.ascontiguousarray(A[:-1, :-1]))
    return out


def removed_functions(patch, essential_dofs, dim, periodic_axes=()):
    """kept[c][d]: bool[n_d], False for the boundary function of axis d that component c loses: the one of a face ALL of
    whose dofs (node, c) are essential.  Essential dofs that do not fill a face remove nothing.  With periodic axes the
    essential dofs are in the folded numbering (integrators.periodic_node_map): a periodic axis has n_d - 1 functions and no
    face, and the nodes of the other axes' faces are looked up through the node map."""
    periodic_axes = sorted(set(int(a) for a in periodic_axes))
    n_dir = [int(n) - (d in periodic_axes) for d, n in enumerate(patch.n_ctrl)]
    node_map = None
    if periodic_axes:
        from .integrators import periodic_node_map
        node_map = periodic_node_map(patch.n_ctrl, periodic_axes)
    ess = np.zeros(int(np.prod(n_dir)) * dim, dtype=bool)
    ess[np.asarray(essential_dofs, dtype=np.int64)] = True
    kept = [[np.ones(n_dir[d], dtype=bool) for d in range(patch.dim)] for _ in range(dim)]
    for d in range(patch.dim):
        if d in periodic_axes:
            continue
        for side in (0, 1):
            nodes = patch.boundary_nodes(d, side)
            if node_map is not None:
                nodes = np.unique(node_map[nodes])
            for c in range(dim):
                if ess[nodes * dim + c].all():
                    kept[c][d][0 if side == 0 else -1] = False
    return kept


def stiffness_coefficients(lame_lambda, lame_mu, fac0, fac1=0.0, viscosity=0.0, dim=3):
    """stiff[c * dim + d] = fac0 e_cd + fac1 eta of the operator"""
    e = np.full((dim, dim), float(lame_mu))
    e[np.arange(dim), np.arange(dim)] = lame_lambda + 2.0 * lame_mu
    return np.ascontiguousarray((fac0 * e + fac1 * max(float(viscosity), 0.0)).ravel())


class KroneckerOperator:
    """The eigen-decompositions of one patch and list of essential dofs (byVDIM numbering, dof = node * dim + c).

    periodic_axes  the axes whose two end faces are joined (boundary_condition.initial.periodic): the first and last basis
                 function of such an axis are one function, the essential dofs are in the folded numbering of
                 integrators.periodic_node_map, and everything below lives on the reduced grid
    n_dir        nodes per axis (n_d - 1 on a periodic axis)
    lengths      L_d (on a periodic axis the whole unwrapped polygon: the period)
    M, K         the scaled 1-D matrices L_d M^_d and K^_d / L_d, per axis
    kept         kept[c][d], see removed_functions
    U_cd, lam_cd per [c][d]: U (n_d x n_d; zero rows and columns for removed functions) and lam (n_d; -1 marks a removed
                 function, which the device turns into a zero of the scaling)
    U, lam       the same, flattened and concatenated over [component][axis]: the arguments of LinearSolver.SetKronecker"""

    def __init__(self, patch, essential_dofs, dim, periodic_axes=()):
        if dim != patch.dim:
            raise RuntimeError(f"Kronecker preconditioner: {dim} components on a {patch.dim}-D patch")
        self.dim = dim
        self.periodic_axes = sorted(set(int(a) for a in periodic_axes))
        if any(a < 0 or a >= patch.dim for a in self.periodic_axes):
            raise RuntimeError(f"Kronecker preconditioner: periodic axes {self.periodic_axes} on a {patch.dim}-D patch")
        self.n_dir = [int(n) - (d in self.periodic_axes) for d, n in enumerate(patch.n_ctrl)]
        self.n = int(np.prod(self.n_dir)) * dim
        self.lengths = axis_lengths(patch)
        self.M, self.K = [], []
        for d in range(patch.dim):
            M, K = matrices_1d(patch.knots[d], patch.degrees[d])
            if d in self.periodic_axes:
                M, K = folded_matrices(M, K)
            self.M.append(self.lengths[d] * M)
            self.K.append(K / self.lengths[d])
        self.essential_dofs = np.unique(np.asarray(essential_dofs if essential_dofs is not None else [], dtype=np.int64))
        self.kept = removed_functions(patch, self.essential_dofs, dim, self.periodic_axes)
        self.U_cd, self.lam_cd = [], []
        for c in range(dim):
            Us, lams = [], []
            for d in range(patch.dim):
                keep = np.nonzero(self.kept[c][d])[0]
                n = self.n_dir[d]
                U, lam = np.zeros((n, n)), np.full(n, -1.0)
                if len(keep):
                    w, V = scipy.linalg.eigh(self.K[d][np.ix_(keep, keep)], self.M[d][np.ix_(keep, keep)])
                    U[np.ix_(keep, np.arange(len(keep)))] = V
                    lam[:len(keep)] = np.maximum(w, 0.0)       # (the constant's eigenvalue is a rounded zero of either sign)
                Us.append(U)
                lams.append(lam)
            self.U_cd.append(Us)
            self.lam_cd.append(lams)
        self.U = np.ascontiguousarray(np.concatenate([U.ravel() for Us in self.U_cd for U in Us]))
        self.lam = np.ascontiguousarray(np.concatenate([lam for lams in self.lam_cd for lam in lams]))

    def scaling(self, mass, stiff):
        """D[node, c] of the coefficients (the array the device rebuilds), shape [n_nodes, dim]"""
        stiff = np.asarray(stiff, dtype=np.float64).reshape(self.dim, self.dim)
        D = np.zeros(self.n_dir[::-1] + [self.dim])
        for c in range(self.dim):
            s = np.full(self.n_dir[::-1], float(mass))
            removed = np.zeros(self.n_dir[::-1], dtype=bool)
            for d in range(self.dim):
                shape = [1] * self.dim
                shape[self.dim - 1 - d] = -1
                lam = self.lam_cd[c][d].reshape(shape)
                s = s + stiff[c, d] * lam
                removed = removed | (lam < 0.0)
            ok = ~removed & (s > 0.0)
            D[..., c] = np.where(ok, 1.0 / np.where(ok, s, 1.0), 0.0)
        return D.reshape(-1, self.dim)

    def apply(self, r, mass, stiff):
        """z = P^-1 r, z[ess] = r[ess] in numpy: what the device computes, for checks and small problems"""
        r = np.asarray(r, dtype=np.float64)
        X = r.reshape(self.n_dir[::-1] + [self.dim])
        D = self.scaling(mass, stiff).reshape(X.shape)
        Z = np.empty_like(X)
        for c in range(self.dim):
            t = X[..., c]
            for d in range(self.dim):                      # towards the eigenbasis: U^T along every axis
                t = np.moveaxis(np.tensordot(self.U_cd[c][d].T, t, axes=(1, self.dim - 1 - d)), 0, self.dim - 1 - d)
            t = t * D[..., c]
            for d in reversed(range(self.dim)):
                t = np.moveaxis(np.tensordot(self.U_cd[c][d], t, axes=(1, self.dim - 1 - d)), 0, self.dim - 1 - d)
            Z[..., c] = t
        z = Z.reshape(-1)
        z[self.essential_dofs] = r[self.essential_dofs]
        return z
