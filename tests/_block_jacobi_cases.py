"""The fixed systems on which the node-block Jacobi preconditioner of csrc/krylov.hip (preconditioner id 3) is held to the
references of tests/_krylov_reference.py (120 digits) and tests/_kronecker_reference.py (the fp64 restatement with a
callable preconditioner): one table, used by test_block_jacobi_cpu.py and test_block_jacobi_gpu.py.

The preconditioner is M = blockdiag(B_A^-1), B_A the vdim x vdim block of node A (an entry the pattern lacks is zero).  The
120-digit reference has Jacobi or nothing, so the GPU tests lean on two equivalences, both vetted on the CPU between the two
references (test_block_jacobi_cpu.py):
    GMRES   left-preconditioned GMRES on (A, b) with M is plain GMRES on (M A, M b): the same iterates, the same residuals;
    CG      with B_A = L_A L_A^T (Cholesky) and C = blockdiag(L_A^-T), M = C C^T, and CG on (A, b) with M is plain CG on
            (C^T A C, C^T b) in x^ = C^-1 x; its stopping quantity (r, M r) is r^T r of the transformed system.
M and C are formed in fp64 (numpy), the products M A, M b, C^T A C, C^T b in long double and rounded to fp64 once (the
references take fp64 inputs exactly).

DEV_X is MEASURED, on the CPU, by test_block_jacobi_cpu.py::test_restatement_equals_reference: the worst deviation
max|x - x_ref| / max|x_ref| of the fp64 restatement (the callable applies the same fp64 M) from the 120-digit answer over the
table below,
    measured 5.36e-16 (nodes12x3_dropped), recorded as 5.4e-16.
The bar of the GPU test is BAR = 20 times it (the convention of tests/_krylov_cases.py): it comes from the rounding of an
fp64 solve of these systems and never from what the device returns.  MARGIN is the rule of tests/test_krylov_reference_cpu.py:
no residual of a reference solve within 1e-3 of the goal, asserted on the CPU for every case (the diagonal strengths below
are chosen so that it holds)."""
import functools

import numpy as np
import scipy.sparse as sp

import _krylov_cases as kc
import _krylov_reference as kref

LD = np.longdouble
DEV_X = 5.4e-16
BAR = 20.0
MARGIN = 1e-3


def _dropped():
    """nodes12x3_dropped of _krylov_cases (no middle dof of the OTHER nodes), and entry ((a, 0), (a, 2)) of every node's own
    block taken out of the pattern as well: a block entry that is missing counts as zero"""
    A, b = kc.node_system(12, 3, 32, drop_middle=True)
    A = A.tolil()
    for a in range(12):
        A[3 * a, 3 * a + 2] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A, b


# name: (method, builder, vdim, solver settings)
CASES = {
    "nodes12x3": ("gmres", lambda: kc.node_system(12, 3, 31), 3, dict(kdim=7)),
    "nodes12x3_dropped": ("gmres", _dropped, 3, dict(kdim=50)),
    "nodes17x2": ("gmres", lambda: kc.node_system(17, 2, 33), 2, dict(kdim=5)),
    "nodes12x3_cg": ("cg", lambda: kc.node_system(12, 3, 53, diag=9.0, symmetric=True), 3, dict()),
}
# essential dofs inside blocks: one dof of a node, two of another, a whole node (nodes12x3)
ESSENTIAL = np.array([1, 12, 14, 21, 22, 23], dtype=np.int64)


def settings(name):
    method, _, _, given = CASES[name]
    base = kc.GMRES_DEFAULTS if method == "gmres" else kc.CG_DEFAULTS
    return {k: v for k, v in {**base, **given}.items() if k != "jacobi"}


@functools.lru_cache(maxsize=None)
def system(name):
    A, b = CASES[name][1]()
    b.setflags(write=False)
    return A, b


def blocks_of(A, vdim):
    """B[node, i, j] of a scipy matrix, zeros where the pattern has no entry"""
    D = sp.csr_matrix(A).toarray()
    n_nodes = D.shape[0] // vdim
    return np.stack([D[a * vdim:(a + 1) * vdim, a * vdim:(a + 1) * vdim] for a in range(n_nodes)])


def eliminated(A, ess):
    """EliminateRowCol(ess, DIAG_ONE) on the matrix' own pattern (explicit zeros stay stored)"""
    A = sp.csr_matrix(A).copy()
    is_ess = np.zeros(A.shape[0], dtype=bool)
    is_ess[ess] = True
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    gone = is_ess[rows] | is_ess[A.indices]
    A.data[gone] = 0.0
    A.data[gone & (rows == A.indices)] = 1.0
    return A


def block_inverse(A, vdim):
    """M = blockdiag(B_A^-1) in fp64, dense"""
    B = blocks_of(A, vdim)
    M = np.zeros((A.shape[0], A.shape[0]))
    for a, Ba in enumerate(B):
        M[a * vdim:(a + 1) * vdim, a * vdim:(a + 1) * vdim] = np.linalg.inv(Ba)
    return M


def block_cholesky_factor(A, vdim):
    """C = blockdiag(L_A^-T) in fp64, dense: M = C C^T"""
    B = blocks_of(A, vdim)
    C = np.zeros((A.shape[0], A.shape[0]))
    for a, Ba in enumerate(B):
        C[a * vdim:(a + 1) * vdim, a * vdim:(a + 1) * vdim] = np.linalg.inv(np.linalg.cholesky(Ba)).T
    return C


def _round(M):
    return np.asarray(M, dtype=np.float64)


def transformed(name, ess=None):
    """what the 120-digit reference solves, and how its answer maps back: (matrix, right-hand side, back) with
    x = back @ x_reference.  GMRES: (M A, M b, I); CG: (C^T A C, C^T b, C).  ess: the system eliminated first (the matrix
    by EliminateRowCol(DIAG_ONE), b[ess] = 0)"""
    A, b = system(name)
    method, _, vdim, _ = CASES[name]
    if ess is not None:
        A = eliminated(A, ess)
        b = b.copy()
        b[ess] = 0.0
    Ad = sp.csr_matrix(A).toarray().astype(LD)
    if method == "gmres":
        M = block_inverse(A, vdim).astype(LD)
        return _round(M @ Ad), _round(M @ b.astype(LD)), np.eye(len(b))
    C = block_cholesky_factor(A, vdim)
    Cl = C.astype(LD)
    return _round(Cl.T @ Ad @ Cl), _round(Cl.T @ b.astype(LD)), C


@functools.lru_cache(maxsize=None)
def reference(name, with_essential=False):
    """(the 120-digit solve of the transformed system, x of the original one as fp64)"""
    T, tb, back = transformed(name, ESSENTIAL if with_essential else None)
    solve = getattr(kref, CASES[name][0])(T.tolist(), tb.tolist(), jacobi=False, **settings(name))
    x = back.astype(LD) @ np.array([LD(kref.mp.nstr(v, 30)) for v in solve.x])
    return solve, np.asarray(x, dtype=np.float64)


def block_callable(A, vdim):
    """z = M r with the fp64 block inverse: the preconditioner of the fp64 restatement"""
    M = sp.csr_matrix(block_inverse(A, vdim))
    return lambda r: M @ r


def block_solve_extended(A, vdim, r):
    """z_A = B_A^-1 r_A by a long-double solve per node"""
    B = blocks_of(A, vdim).astype(LD)
    r = np.asarray(r, dtype=LD).reshape(-1, vdim)
    z = np.zeros_like(r)
    for a in range(len(B)):
        # Gaussian elimination with partial pivoting in long double (numpy.linalg has no long double)
        M = np.concatenate([B[a], r[a][:, None]], axis=1)
        for k in range(vdim):
            p = k + int(np.argmax(np.abs(M[k:, k])))
            M[[k, p]] = M[[p, k]]
            for i in range(k + 1, vdim):
                M[i] -= M[i, k] / M[k, k] * M[k]
        for k in reversed(range(vdim)):
            z[a, k] = (M[k, vdim] - M[k, k + 1:vdim] @ z[a, k + 1:]) / M[k, k]
    return np.asarray(z.reshape(-1), dtype=np.float64)


def apply_bar(A, vdim):
    """the bar of one application z = M r, relative to max|z|: the closed-form inverse (adjugate over determinant) and the
    product commit a few dozen roundings, each amplified by at most the condition number of the block: 64 eps max cond(B_A)"""
    return 64 * np.finfo(float).eps * max(np.linalg.cond(Ba) for Ba in blocks_of(A, vdim))
