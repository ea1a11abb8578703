"""TEST INFRASTRUCTURE ONLY.  A 120-digit reference of the two Krylov solvers of csrc/krylov.hip (restated in fp64 by
oracle/krylov.py), written from the DEFINITION of the methods and sharing nothing with either: no Arnoldi recurrence, no
Hessenberg matrix, no Givens rotation, no two-term CG recurrences, no numpy in the arithmetic (mpmath only), nothing
imported from oracle/ or mimi_amd/.

GMRES(m), left-preconditioned.  B = M A with M = diag(A)^-1 or I.  In a cycle that starts from (x, r = M (b - A x)) the
k-th iterate is x + Q c, where the columns of Q are an orthonormal basis of K_k(B, r) (twice-repeated Gram-Schmidt at
the working precision) and c minimises ||r - B Q c||_2.  The least-squares problem is solved densely, by a QR
factorisation of the n x k matrix B Q (twice-repeated Gram-Schmidt again; the factorisation of the first k - 1 columns is
kept from one k to the next).  The solve stops at the first k whose minimum is <= goal = max(rel ||M b||, abs).  After m
steps x <- x + Q c, r <- M (b - A x), and the same test is made on ||r||.  The accounting is mfem's GMRESSolver::Mult
with iterative_mode false: `iterations` counts the Krylov steps made, a solve that runs out of them returns max_iter and
the norm of the last restart residual.

CG, Jacobi-preconditioned.  x_k is the Galerkin solution over K_k(M A, M b): (Q^T A Q) c = Q^T b, solved densely.  The
stopping quantity (r_k, M r_k) comes from r_k = b - A x_k; the solve stops on <= max(rel^2 (r_0, M r_0), abs^2) or at
max_iter.  The step x_{k+1} - x_k is a multiple of the k-th search direction d_k of the recurrence form, so
(d_k, A d_k) <= 0, where mfem's CGSolver gives up, is seen as (x_{k+1} - x_k, A (x_{k+1} - x_k)) <= 0.

At 120 digits the Krylov bases stay numerically independent over a cycle (every case has n <= 60), so what is returned
is the exact-arithmetic answer to about 100 digits: the iteration count is a property of the problem as long as no
residual of the history sits on the goal (`Solve.margin`, which the tests assert).

A matrix goes in as a dense nested sequence or as a CSR triple (rowptr, col, val) of plain sequences; fp64 inputs are
taken exactly."""
import collections

from mpmath import mp, mpf

DPS = 120

Solve = collections.namedtuple("Solve", "x iterations final_norm converged history restarts indefinite iterates goal")
Solve.__doc__ = """x: the iterate returned (list of mpf); history: residual_k / goal for every step k = 1, 2, ... (for CG:
sqrt((r_k, M r_k)) / sqrt(goal^2), negative when (r_k, M r_k) < 0), preceded in history[0] by that of the start;
restarts: ||r|| / goal recomputed at every GMRES restart; indefinite: CG met (d, A d) <= 0; iterates: x_0, x_1, ...
(CG) or the x at every restart (GMRES); goal: the stopping threshold on the norm."""


def margin(solve):
    """how far, relatively, the closest residual of the solve stays from the goal"""
    return min(abs(h - 1) for h in list(solve.history) + list(solve.restarts))


class _Matrix:
    def __init__(self, A, n):
        if isinstance(A, tuple):
            rowptr, col, val = A
            self.rows = [[(int(col[k]), mpf(float(val[k]))) for k in range(int(rowptr[i]), int(rowptr[i + 1]))]
                         for i in range(n)]
        else:
            self.rows = [[(j, mpf(float(a))) for j, a in enumerate(A[i]) if float(a) != 0.0] for i in range(n)]
        self.n = n

    def mult(self, x):
        return [mp.fsum(a * x[j] for j, a in row) for row in self.rows]

    def diagonal(self):
        return [mp.fsum(a for j, a in row if j == i) for i, row in enumerate(self.rows)]

    def dense(self):
        D = mp.zeros(self.n, self.n)
        for i, row in enumerate(self.rows):
            for j, a in row:
                D[i, j] += a
        return D


def _dot(a, b):
    return mp.fdot(a, b)


def _norm(a):
    return mp.sqrt(mp.fdot(a, a))


def _orthogonalise(v, basis):
    """v minus its components along the orthonormal `basis`, Gram-Schmidt made twice; (the rest, the components)"""
    v = list(v)
    coef = [mpf(0)] * len(basis)
    for _ in range(2):
        for k, q in enumerate(basis):
            h = _dot(v, q)
            coef[k] += h
            v = [vi - h * qi for vi, qi in zip(v, q)]
    return v, coef


def _back_substitute(R_cols, g):
    """R c = g for the upper triangular R whose k-th column is R_cols[k] (k + 1 entries)"""
    k = len(g)
    c = [mpf(0)] * k
    for i in range(k - 1, -1, -1):
        t = g[i] - mp.fsum(R_cols[j][i] * c[j] for j in range(i + 1, k))
        c[i] = t / R_cols[i][i]
    return c


def _combine(x, Q, c):
    return [xi + mp.fsum(cj * q[i] for cj, q in zip(c, Q)) for i, xi in enumerate(x)]


def solve_direct(A, b):
    """A^-1 b by a dense LU factorisation at the working precision"""
    with mp.workdps(DPS):
        n = len(b)
        x = mp.lu_solve(_Matrix(A, n).dense(), mp.matrix([mpf(float(v)) for v in b]))
        return [x[i] for i in range(n)]


def gmres(A, b, rel_tol=1e-8, abs_tol=1e-12, max_iter=300, kdim=50, jacobi=True):
    with mp.workdps(DPS):
        n = len(b)
        op = _Matrix(A, n)
        b = [mpf(float(v)) for v in b]
        minv = [1 / d for d in op.diagonal()] if jacobi else [mpf(1)] * n

        def precond_residual(x):
            return [m * (bi - t) for m, bi, t in zip(minv, b, op.mult(x))]

        def B(v):
            return [m * t for m, t in zip(minv, op.mult(v))]

        x = [mpf(0)] * n
        r = [m * bi for m, bi in zip(minv, b)]
        beta = _norm(r)
        goal = max(mpf(rel_tol) * beta, mpf(abs_tol))
        ratio = (lambda v: v / goal) if goal > 0 else (lambda v: mpf(0) if v == 0 else mp.inf)
        history, restarts, iterates = [ratio(beta)], [], []
        if beta <= goal:
            return Solve(x, 0, beta, True, history, restarts, False, iterates, goal)
        j = 0                                   # Krylov steps made
        while j < max_iter:
            Q, U, R_cols, g = [], [], [], []     # basis of K_k(B, r); B Q = U R; g = U^T r
            rho = list(r)                        # r - U U^T r: the least-squares residual
            k = 0
            while k < kdim and j < max_iter:
                q, _ = _orthogonalise(r if not Q else B(Q[-1]), Q)
                nq = _norm(q)
                if nq <= mpf(10) ** (-DPS // 2) * beta:
                    raise ArithmeticError("the Krylov space is exhausted above the goal: not a case for this reference")
                Q.append([v / nq for v in q])
                u, coef = _orthogonalise(B(Q[-1]), U)
                nu = _norm(u)
                U.append([v / nu for v in u])
                R_cols.append(coef + [nu])
                g.append(_dot(U[-1], r))
                rho = [v - g[-1] * ui for v, ui in zip(rho, U[-1])]
                resid = _norm(rho)
                k += 1
                j += 1
                history.append(ratio(resid))
                if resid <= goal:
                    x = _combine(x, Q, _back_substitute(R_cols, g))
                    # the minimum, formed the long way
                    assert abs(_norm(precond_residual(x)) - resid) <= mpf(10) ** (-80) * beta
                    return Solve(x, j, resid, True, history, restarts, False, iterates, goal)
            x = _combine(x, Q, _back_substitute(R_cols, g))
            iterates.append(x)
            r = precond_residual(x)
            beta = _norm(r)
            assert abs(beta - resid) <= mpf(10) ** (-80) * history[0] * goal
            restarts.append(ratio(beta))
            if beta <= goal:
                return Solve(x, j, beta, True, history, restarts, False, iterates, goal)
        return Solve(x, max_iter, beta, False, history, restarts, False, iterates, goal)


def cg(A, b, rel_tol=1e-8, abs_tol=1e-12, max_iter=1000, jacobi=True):
    with mp.workdps(DPS):
        n = len(b)
        op = _Matrix(A, n)
        b = [mpf(float(v)) for v in b]
        minv = [1 / d for d in op.diagonal()] if jacobi else [mpf(1)] * n

        def stopping(x):
            r = [bi - t for bi, t in zip(b, op.mult(x))]
            return mp.fsum(m * ri * ri for m, ri in zip(minv, r))

        def root(v):
            return mp.sqrt(abs(v))

        x = [mpf(0)] * n
        nom = stopping(x)
        r0 = max(nom * mpf(rel_tol) ** 2, mpf(abs_tol) ** 2)
        goal = mp.sqrt(r0)
        ratio = (lambda v: mp.sign(v) * root(v) / goal) if goal > 0 else (lambda v: mpf(0) if v == 0 else mp.inf)
        history, iterates = [ratio(nom)], [x]
        if nom <= r0:
            return Solve(x, 0, root(nom), True, history, [], False, iterates, goal)
        Q, AQ, G, f = [], [], [], []             # basis of K_k(M A, M b); G = Q^T A Q; f = Q^T b
        k = 0
        v = [m * bi for m, bi in zip(minv, b)]
        while True:
            q, _ = _orthogonalise(v, Q)
            nq = _norm(q)
            Q.append([t / nq for t in q])
            AQ.append(op.mult(Q[-1]))
            for i, row in enumerate(G):
                row.append(_dot(Q[i], AQ[-1]))
            G.append([_dot(Q[-1], aq) for aq in AQ])
            f.append(_dot(Q[-1], b))
            c = mp.lu_solve(mp.matrix(G), mp.matrix(f))
            x_new = _combine([mpf(0)] * n, Q, [c[i] for i in range(len(f))])
            step = [a - o for a, o in zip(x_new, x)]
            if _dot(step, op.mult(step)) <= 0:    # (d_k, A d_k) <= 0
                return Solve(x, k, root(nom), False, history, [], True, iterates, goal)
            x = x_new
            k += 1
            nom = stopping(x)
            history.append(ratio(nom))
            iterates.append(x)
            if nom <= r0:
                return Solve(x, k, root(nom), True, history, [], False, iterates, goal)
            if k >= max_iter:
                return Solve(x, k, root(nom), False, history, [], False, iterates, goal)
            v = [m * t for m, t in zip(minv, AQ[-1])]
