"""The fixed systems on which the Krylov solvers are held to tests/_krylov_reference.py: one table, used by
test_krylov_reference_cpu.py (the fp64 restatement oracle/krylov.py) and by test_krylov_gpu.py (csrc/krylov.hip).

DEV_X and DEV_NORM are MEASURED, on the CPU, by test_krylov_reference_cpu.py::test_restatement_equals_reference: the
worst deviation of the fp64 restatement from the 120-digit reference over the whole table,

    DEV_X    = max over cases of  max|x - x_ref| / max|x_ref|     measured 2.48e-15 (ns36_k50), recorded as 2.5e-15
    DEV_NORM = max over cases of  |final_norm - norm_ref| / goal    measured 4.71e-08 (ns36_k5_cut7), recorded as 4.8e-8

(the norm of an unconverged solve is about 1e8 goals, so its fp64 rounding, eps ||M b||, is about 1e-8 goals; the rotated
right-hand side of a converged one carries the same.)

The bars of both tests are BAR = 20 times these: they come from the rounding of
an fp64 solve of these systems and never from what the device returns."""
import functools

import numpy as np
import scipy.sparse as sp

import _krylov_reference as ref

DEV_X = 2.5e-15
DEV_NORM = 4.8e-8
BAR = 20.0


def _csr(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def random_system(n, density, diag, seed, symmetric=False):
    """sp.random(n, n, density, seed) + diag(diag + U[0, 1)), and a standard normal right-hand side"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=density, random_state=seed, format="csr")
    if symmetric:
        A = 0.5 * (A + A.T)
    A = _csr(A + sp.diags(diag + rng.random(n)))
    return A, rng.standard_normal(n)


def node_system(n_nodes, vdim, seed, diag=6.0, drop_middle=False, symmetric=False):
    """a vdim-vector field on a ring of nodes, every node coupled to itself and two neighbours on either side, byVDIM
    numbering: the vdim rows of a node share their column list (drop_middle: without the middle dof of the other nodes,
    so the list is not made of node triples)"""
    rng = np.random.default_rng(seed)
    n = n_nodes * vdim
    rows, cols = [], []
    for a in range(n_nodes):
        nb = sorted({(a + s) % n_nodes for s in (-2, -1, 0, 1, 2)})
        for c in range(vdim):
            for bnode in nb:
                for e in range(vdim):
                    if drop_middle and e == 1 and bnode != a:
                        continue
                    rows.append(a * vdim + c)
                    cols.append(bnode * vdim + e)
    vals = rng.standard_normal(len(rows))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    if symmetric:
        A = 0.5 * (A + A.T)
    A = _csr(A + sp.diags(diag + rng.random(n)))
    return A, rng.standard_normal(n)


def _ns36(diag):
    return lambda: random_system(36, 0.25, diag, 7)


def _scaled(build, factor):
    def f():
        A, b = build()
        return A, b * factor
    return f


def _indefinite():
    A, b = random_system(36, 0.2, 3.0, 11, symmetric=True)
    A = A.tolil()
    A[20, 20] = -A[20, 20]
    return _csr(A), b


# name: (method, builder, solver settings, (RowGroup, NodeColumns) of the pattern)
CASES = {
    # non-symmetric, Jacobi: >= 20 restart cycles that converge; stagnation to max_iter; no restart
    "ns36_k5": ("gmres", _ns36(1.5), dict(kdim=5), (1, False)),
    "ns36_k5_stagnates": ("gmres", _ns36(1.2), dict(kdim=5), (1, False)),
    "ns36_k50": ("gmres", _ns36(1.2), dict(kdim=50), (1, False)),
    "ns36_k7_plain": ("gmres", _ns36(1.5), dict(kdim=7, jacobi=False), (1, False)),
    "ns36_k1": ("gmres", _ns36(3.0), dict(kdim=1), (1, False)),
    "ns36_k1_plain": ("gmres", _ns36(3.0), dict(kdim=1, jacobi=False), (1, False)),
    # max_iter: in the middle of the second cycle; at the end of a cycle; none at all
    "ns36_k5_cut7": ("gmres", _ns36(1.5), dict(kdim=5, max_iter=7), (1, False)),
    "ns36_k5_cut10": ("gmres", _ns36(1.5), dict(kdim=5, max_iter=10), (1, False)),
    "ns36_k7_cut3": ("gmres", _ns36(1.5), dict(kdim=7, max_iter=3), (1, False)),
    "ns36_maxiter0": ("gmres", _ns36(1.5), dict(kdim=5, max_iter=0), (1, False)),
    # n below a wave and below kdim
    "n1": ("gmres", lambda: random_system(1, 1.0, 1.5, 21), dict(), (1, False)),
    "n1_plain": ("gmres", lambda: random_system(1, 1.0, 1.5, 21), dict(jacobi=False), (1, False)),
    "n3": ("gmres", lambda: random_system(3, 1.0, 1.5, 22), dict(), (3, True)),      # (full: one node)
    "n6": ("gmres", lambda: random_system(6, 0.8, 1.5, 23), dict(), (1, False)),
    "n7": ("gmres", lambda: random_system(7, 0.7, 1.5, 24), dict(), (1, False)),
    "n7_k50_plain": ("gmres", lambda: random_system(7, 0.7, 1.5, 24), dict(jacobi=False), (1, False)),
    # the zero-iteration returns, and abs_tol as the goal of a solve that iterates
    "b_zero": ("gmres", _scaled(_ns36(1.5), 0.0), dict(kdim=5), (1, False)),
    "b_below_abs_tol": ("gmres", _scaled(_ns36(1.5), 1e-14), dict(kdim=5), (1, False)),
    "b_abs_tol_decides": ("gmres", _scaled(_ns36(1.5), 1e-9), dict(kdim=7), (1, False)),
    # symmetric
    "sym36_k50": ("gmres", lambda: random_system(36, 0.25, 2.5, 9, symmetric=True), dict(), (1, False)),
    "sym36_k5_plain": ("gmres", lambda: random_system(36, 0.25, 2.5, 9, symmetric=True), dict(kdim=5, jacobi=False), (1, False)),
    # the four product forms: n % 3 == 0 with node triples and without, n % 2 == 0, neither
    "nodes12x3": ("gmres", lambda: node_system(12, 3, 31), dict(kdim=7), (3, True)),
    "nodes12x3_dropped": ("gmres", lambda: node_system(12, 3, 32, drop_middle=True), dict(kdim=50), (3, False)),
    "nodes17x2": ("gmres", lambda: node_system(17, 2, 33), dict(kdim=5), (2, False)),
    "nodes18x2": ("gmres", lambda: node_system(18, 2, 34), dict(kdim=7, jacobi=False), (2, False)),
    "ragged35": ("gmres", lambda: random_system(35, 0.25, 1.5, 35), dict(kdim=7), (1, False)),
    # the replicated systems of the large-vector tests (n0 = 33, about 7 entries per row)
    "ns33_k5": ("gmres", lambda: random_system(33, 6.0 / 33, 2.0, 41), dict(kdim=5, abs_tol=0.0), (1, False)),
    "spd33_cg": ("cg", lambda: random_system(33, 6.0 / 33, 3.0, 42, symmetric=True), dict(abs_tol=0.0), (1, False)),
    # conjugate gradients
    "spd36_cg": ("cg", lambda: random_system(36, 0.25, 3.0, 51, symmetric=True), dict(), (1, False)),
    "spd35_cg_plain": ("cg", lambda: random_system(35, 0.25, 3.0, 52, symmetric=True), dict(jacobi=False), (1, False)),
    "nodes12x3_cg": ("cg", lambda: node_system(12, 3, 53, diag=9.0, symmetric=True), dict(), (3, True)),
    "spd36_cg_cut4": ("cg", lambda: random_system(36, 0.25, 3.0, 51, symmetric=True), dict(max_iter=4), (1, False)),
    "cg_b_zero": ("cg", _scaled(lambda: random_system(36, 0.25, 3.0, 51, symmetric=True), 0.0), dict(), (1, False)),
    "cg_n1": ("cg", lambda: random_system(1, 1.0, 1.5, 21), dict(), (1, False)),
    "cg_indefinite": ("cg", _indefinite, dict(jacobi=False), (1, False)),
}

GMRES_DEFAULTS = dict(rel_tol=1e-8, abs_tol=1e-12, max_iter=300, kdim=50, jacobi=True)
CG_DEFAULTS = dict(rel_tol=1e-8, abs_tol=1e-12, max_iter=1000, jacobi=True)


def settings(name):
    method, _, given, _ = CASES[name]
    return {**(GMRES_DEFAULTS if method == "gmres" else CG_DEFAULTS), **given}


@functools.lru_cache(maxsize=None)
def system(name):
    """(A as scipy CSR with sorted indices and a stored diagonal, b); shared, not to be written to"""
    A, b = CASES[name][1]()
    assert (A.diagonal() != 0).all()
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def reference(name):
    """the 120-digit solve of the case; x also as fp64 (`x64`)"""
    A, b = system(name)
    solve = getattr(ref, CASES[name][0])((A.indptr.tolist(), A.indices.tolist(), A.data.tolist()), b.tolist(), **settings(name))
    return solve, np.array([float(v) for v in solve.x])


def deviations(name, x, final_norm):
    """(max|x - x_ref| / max|x_ref|, |final_norm - norm_ref| / goal) of a solve of the case"""
    solve, x64 = reference(name)
    scale = np.abs(x64).max()
    dx = float(np.abs(np.asarray(x) - x64).max() / scale) if scale > 0 else float(np.abs(np.asarray(x)).max())
    dn = float(abs(ref.mpf(float(final_norm)) - solve.final_norm) / solve.goal)
    return dx, dn


def replicated(name, copies, seed=5):
    """A = I_copies (x) A0, b = c (x) b0 with |c_j| in [0.5, 2] of mixed sign: every Krylov quantity of (A, b) is that of
    (A0, b0) times c_j on block j, so the solvers take the iterations of (A0, b0) and return c (x) x0 and ||c|| norm0
    (as long as the relative tolerance decides).  (rowptr, col, val, b, c)"""
    A0, b0 = system(name)
    n0, nnz0 = A0.shape[0], A0.nnz
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.5, 2.0, copies) * rng.choice([-1.0, 1.0], copies)
    rowptr = (A0.indptr[None, :-1].astype(np.int64) + nnz0 * np.arange(copies, dtype=np.int64)[:, None]).ravel()
    rowptr = np.concatenate([rowptr, [nnz0 * copies]]).astype(np.int64)
    col = (A0.indices[None, :].astype(np.int64) + n0 * np.arange(copies, dtype=np.int64)[:, None]).ravel().astype(np.int32)
    val = np.tile(A0.data, copies)
    b = (c[:, None] * b0[None, :]).ravel()
    return rowptr, col, val, b, c
