"""TEST INFRASTRUCTURE ONLY.  References for the fast-diagonalisation (Kronecker) preconditioner, written from its
definition and sharing nothing with mimi_amd/kronecker.py: no eigen-decomposition, no mode product.

1. matrices_1d: the 1-D mass and stiffness matrices of a knot vector by a Gauss loop of its own over the basis functions of
   oracle/iga.py; axis_lengths: the mean control-polygon length; kept_functions: the face rule.
2. component_operator: the DENSE  P_c = mass (x)_d M_d + sum_d stiff[c][d] K_d (x) (M of the other axes)  on the functions
   component c keeps (numpy.kron, first axis fastest), and apply_extended: z = P^-1 r, z[ess] = r[ess] with every P_c solved
   in extended precision (mpmath, 50 digits).  solve_extended does that for any matrix: an fp64 LU factorisation refined
   with residuals formed in mpmath from the matrix' exact fp64 entries, until the residual is below 1e-40 of the right-hand
   side -- the answer of a dense 50-digit elimination at a cost the larger node grids of the tests can afford (a pure
   mpmath LU of 560 unknowns takes minutes); the final residual is asserted, so the digits do not rest on the fp64 factors.
3. gmres / cg: oracle/krylov.py restated line by line with the preconditioner as a callable z = precond(r) (oracle/ cannot
   change), returning the residual history over the goal as well so that a case's margin can be asserted."""
import collections

import numpy as np
import scipy.linalg
import scipy.sparse as sp
from mpmath import mp, mpf

DPS = 50

Solve = collections.namedtuple("Solve", "x iterations final_norm converged history")
Solve.__doc__ = "history: every residual the stopping rule saw, divided by the goal (the start first)"


def margin(solve):
    """how far, relatively, the closest residual of the solve stays from the goal"""
    return min(abs(h - 1.0) for h in solve.history)


# ---- 1. the ingredients ------------------------------------------------------------------------------------------------
def matrices_1d(knots, p):
    """(M^, K^) on the unit interval: int N_a N_b / T and T int N_a' N_b' over the knots' own interval of length T"""
    from oracle import iga
    knots = np.asarray(knots, dtype=np.float64)
    n = len(knots) - p - 1
    T = knots[-1] - knots[0]
    x, w = iga.gauss_legendre_01(p + 1)
    M, K = np.zeros((n, n)), np.zeros((n, n))
    for s in range(p, n):
        h = knots[s + 1] - knots[s]
        if h <= 0:
            continue
        for xq, wq in zip(x, w):
            N, dN = iga.basis_ders(knots, p, s, knots[s] + xq * h)
            for a in range(p + 1):
                for b in range(p + 1):
                    M[s - p + a, s - p + b] += wq * h * N[a] * N[b] / T
                    K[s - p + a, s - p + b] += wq * h * dN[a] * dN[b] * T
    return M, K


def axis_lengths(P):
    """mean over the control polygons along axis d of their length (P: oracle iga.Patch)"""
    strides = [int(np.prod(P.n[:d])) for d in range(P.dim)]
    out = []
    for d in range(P.dim):
        lengths = []
        for start in range(P.n_nodes):
            if (start // strides[d]) % P.n[d] != 0:
                continue
            line = P.ctrl[start + strides[d] * np.arange(P.n[d])]
            lengths.append(sum(np.linalg.norm(line[i + 1] - line[i]) for i in range(P.n[d] - 1)))
        out.append(float(np.mean(lengths)))
    return out


def scaled_matrices(P):
    """per axis (L_d M^_d, K^_d / L_d)"""
    L = axis_lengths(P)
    out = []
    for d in range(P.dim):
        M, K = matrices_1d(P.knots[d], P.p[d])
        out.append((L[d] * M, K / L[d]))
    return out


def kept_functions(P, ess, dim):
    """kept[c][d][i]: False when i is the boundary function of a face of axis d whose dofs (node, c) are ALL essential"""
    ess = set(int(e) for e in ess)
    kept = [[np.ones(P.n[d], dtype=bool) for d in range(P.dim)] for _ in range(dim)]
    for d in range(P.dim):
        for side in (0, 1):
            nodes = P.boundary_nodes(d, side)
            for c in range(dim):
                if all(int(a) * dim + c in ess for a in nodes):
                    kept[c][d][0 if side == 0 else P.n[d] - 1] = False
    return kept


def _kron(factors):
    """(x) with the FIRST axis fastest"""
    out = np.ones((1, 1))
    for f in factors:
        out = np.kron(f, out)
    return out


def component_operator(P, c, mass, stiff, kept, matrices=None):
    """(dense P_c on the kept functions, their node indices)"""
    matrices = matrices or scaled_matrices(P)
    dim = P.dim
    stiff = np.asarray(stiff, dtype=np.float64).reshape(dim, dim)
    red = [(M[np.ix_(k, k)], K[np.ix_(k, k)]) for (M, K), k in zip(matrices, kept[c])]
    Pc = mass * _kron([m for m, _ in red])
    for d in range(dim):
        Pc = Pc + stiff[c, d] * _kron([red[e][1] if e == d else red[e][0] for e in range(dim)])
    mask = _kron([k.reshape(-1, 1).astype(np.float64) for k in kept[c]]).ravel() > 0
    return Pc, np.nonzero(mask)[0]


# ---- 2. extended precision -----------------------------------------------------------------------------------------------
def solve_extended(A, b):
    """A^-1 b to about 40 digits, as mpf: fp64 LU, residuals in mpmath.  A: dense array or scipy sparse."""
    with mp.workdps(DPS):
        A = sp.csr_matrix(A)
        n = A.shape[0]
        lu = scipy.linalg.lu_factor(A.toarray())
        rows = [[(int(A.indices[k]), mpf(float(A.data[k]))) for k in range(A.indptr[i], A.indptr[i + 1])] for i in range(n)]
        bm = [mpf(float(v)) for v in b]
        scale = max(abs(v) for v in bm)
        x = [mpf(0)] * n
        if scale == 0:
            return x
        for _ in range(12):
            res = [bi - mp.fsum(a * x[j] for j, a in row) for bi, row in zip(bm, rows)]
            worst = max(abs(v) for v in res)
            if worst <= mpf(10) ** -40 * scale:
                return x
            d = scipy.linalg.lu_solve(lu, np.array([float(v / worst) for v in res]))
            x = [xi + worst * mpf(float(di)) for xi, di in zip(x, d)]
        raise ArithmeticError("the refinement did not reach 1e-40: not a matrix for this reference")


def apply_extended(P, ess, dim, mass, stiff, r):
    """z = P^-1 r on the kept functions, 0 on the removed ones, then z[ess] = r[ess]; fp64 roundings of the 40-digit values"""
    kept = kept_functions(P, ess, dim)
    matrices = scaled_matrices(P)
    z = np.zeros(P.n_nodes * dim)
    for c in range(dim):
        Pc, nodes = component_operator(P, c, mass, stiff, kept, matrices)
        z[nodes * dim + c] = [float(v) for v in solve_extended(Pc, r[nodes * dim + c])]
    ess = np.asarray(list(ess), dtype=np.int64)
    z[ess] = r[ess]
    return z


def dense_preconditioner(P, ess, dim, mass, stiff):
    """the same map in fp64 as a callable (a Cholesky factorisation per component): the preconditioner of the restated
    solvers below"""
    kept = kept_functions(P, ess, dim)
    matrices = scaled_matrices(P)
    parts = []
    for c in range(dim):
        Pc, nodes = component_operator(P, c, mass, stiff, kept, matrices)
        parts.append((scipy.linalg.cho_factor(Pc), nodes * dim + c))
    ess = np.asarray(list(ess), dtype=np.int64)

    def precond(r):
        z = np.zeros_like(r)
        for chol, dofs in parts:
            z[dofs] = scipy.linalg.cho_solve(chol, r[dofs])
        z[ess] = r[ess]
        return z
    return precond


# ---- 3. oracle/krylov.py with a preconditioner callable -------------------------------------------------------------------
def gmres(A, b, precond, rel_tol=1e-8, abs_tol=1e-12, max_iter=300, kdim=50):
    n = len(b)
    x = np.zeros(n)
    r = precond(b)
    beta = np.linalg.norm(r)
    goal = max(rel_tol * beta, abs_tol)
    history = [beta / goal]
    if beta <= goal:
        return Solve(x, 0, beta, True, history)
    m = kdim
    j = 1
    while j <= max_iter:
        V = np.zeros((m + 1, n))
        H = np.zeros((m + 1, m))
        cs, sn, s = np.zeros(m + 1), np.zeros(m + 1), np.zeros(m + 1)
        V[0] = r / beta
        s[0] = beta
        i = 0
        while i < m and j <= max_iter:
            w = precond(A @ V[i])
            for k in range(i + 1):                     # modified Gram-Schmidt
                H[k, i] = w @ V[k]
                w -= H[k, i] * V[k]
            H[i + 1, i] = np.linalg.norm(w)
            V[i + 1] = w / H[i + 1, i]
            for k in range(i):                         # ApplyPlaneRotation
                t = cs[k] * H[k, i] + sn[k] * H[k + 1, i]
                H[k + 1, i] = -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
                H[k, i] = t
            dx, dy = H[i, i], H[i + 1, i]              # GeneratePlaneRotation
            if dy == 0.0:
                cs[i], sn[i] = 1.0, 0.0
            elif abs(dy) > abs(dx):
                t = dx / dy
                sn[i] = 1.0 / np.sqrt(1.0 + t * t)
                cs[i] = t * sn[i]
            else:
                t = dy / dx
                cs[i] = 1.0 / np.sqrt(1.0 + t * t)
                sn[i] = t * cs[i]
            H[i, i] = cs[i] * dx + sn[i] * dy
            H[i + 1, i] = 0.0
            s[i + 1] = -sn[i] * s[i]
            s[i] = cs[i] * s[i]
            resid = abs(s[i + 1])
            history.append(resid / goal)
            if resid <= goal:
                y = np.linalg.solve(np.triu(H[:i + 1, :i + 1]), s[:i + 1])
                return Solve(x + y @ V[:i + 1], j, resid, True, history)
            i += 1
            j += 1
        y = np.linalg.solve(np.triu(H[:i, :i]), s[:i])
        x = x + y @ V[:i]
        r = precond(b - A @ x)
        beta = np.linalg.norm(r)
        history.append(beta / goal)
        if beta <= goal:
            return Solve(x, j - 1, beta, True, history)
    return Solve(x, max_iter, beta, False, history)


def cg(A, b, precond, rel_tol=1e-8, abs_tol=1e-12, max_iter=1000):
    n = len(b)
    x = np.zeros(n)
    r = b.copy()
    z = precond(r)
    d = z.copy()
    nom = r @ z
    r0 = max(nom * rel_tol * rel_tol, abs_tol * abs_tol)
    root = lambda v: np.sqrt(abs(v))
    history = [root(nom) / np.sqrt(r0)] if r0 > 0 else [0.0]
    if nom <= r0:
        return Solve(x, 0, root(nom), True, history)
    q = A @ d
    den = q @ d
    if not den > 0:
        return Solve(x, 0, root(nom), False, history)
    it = 1
    while True:
        alpha = nom / den
        x += alpha * d
        r -= alpha * q
        z = precond(r)
        betanom = r @ z
        history.append(root(betanom) / np.sqrt(r0))
        if betanom <= r0:
            return Solve(x, it, root(betanom), True, history)
        if it >= max_iter:
            return Solve(x, it, root(betanom), False, history)
        beta = betanom / nom
        d = z + beta * d
        q = A @ d
        den = d @ q
        if not den > 0:
            return Solve(x, it, root(betanom), False, history)
        nom = betanom
        it += 1
