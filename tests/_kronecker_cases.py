"""The patches, Dirichlet configurations and systems on which the Kronecker preconditioner is held to
tests/_kronecker_reference.py: one table, used by test_kronecker_cpu.py (mimi_amd/kronecker.py in numpy) and by
test_kronecker_gpu.py (csrc/kronecker.hpp through the C ABI).

The DEV_* constants are MEASURED, on the CPU, by test_kronecker_cpu.py (which holds them to what it measures, to the
variation between numpy builds); they are deviations of fp64 computations from the extended-precision references and never
come from what the device returns.  The bars of both tests are BAR = 20 times them (the convention of
tests/_krylov_cases.py).

    DEV_APPLY = max over GRIDS x DIRICHLET of  max|z - z_ref| / max|z_ref|  of the numpy application
                (KroneckerOperator.apply) against apply_extended                  measured 9.52e-13 (p3_10x6, component), recorded 9.6e-13
    DEV_SOLVE = max over SOLVES x FAC0 of  max|x - x_ref| / max|x_ref|  of the restated GMRES with the dense fp64
                preconditioner against solve_extended                            measured 2.79e-08 (p3_4x3x2, fac0 1e-2), recorded 2.8e-8
                (a converged solve stops at a preconditioned residual of 1e-8 of the start: x is no closer than that)
    MARGIN    = every residual of every SOLVES case stays at least this far from the goal, relatively (measured: 1.2e-2
                at the closest, p3_4x3x2 at fac0 1): the restated solve and the device disagree in a residual by rounding
                (DEV_APPLY-sized), orders of magnitude below it

The iteration counts the restatement gives (oracle tangent, Jacobi -> Kronecker) are recorded in ITERATIONS."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import _kronecker_reference as ref
import _patches

BAR = 20.0
DEV_APPLY = 9.6e-13
DEV_SOLVE = 2.8e-8
MARGIN = 1e-3

YOUNG, POISSON, RHO = 2100.0, 0.3, 1.0
LAMBDA = YOUNG * POISSON / ((1 + POISSON) * (1 - 2 * POISSON))
MU = YOUNG / (2 * (1 + POISSON))
# the coefficients of the application tests: rho, and fac0 e_cd + fac1 eta with fac0 = 1e-2 and fac1 eta = 3e-3
APPLY_FAC0, APPLY_DAMPING = 1e-2, 3e-3


def stiff(dim, fac0, damping=0.0):
    """[c][d]: fac0 (lambda + 2 mu if d == c else mu) + damping, written out from the definition"""
    return np.array([[fac0 * (LAMBDA + 2 * MU if d == c else MU) + damping for d in range(dim)] for c in range(dim)])


def _pair(P):
    import mimi_amd
    return P, mimi_amd.BSplinePatch(P.p, P.knots, np.asarray(P.ctrl, dtype=np.float64).reshape(P.n_nodes, -1))


def _block(n_el, p, lengths):
    from oracle import iga
    return lambda: _pair(iga.Patch.block(n_el, p, lengths))


# node grid -> builder of (oracle patch, product patch)
GRIDS = {
    "p2_5x4x3": _block((3, 2, 1), 2, [1.5, 1.0, 0.5]),
    "p2_35x4x4": _block((33, 2, 2), 2, [4.0, 1.0, 1.0]),      # one axis past two 16-wide tiles, in each position
    "p2_4x35x4": _block((2, 33, 2), 2, [1.0, 4.0, 1.0]),
    "p2_4x4x35": _block((2, 2, 33), 2, [1.0, 1.0, 4.0]),
    "p1_6x5x4": _block((5, 4, 3), 1, [2.0, 1.5, 1.0]),
    "p3_10x6": _block((7, 3), 3, [3.0, 1.0]),
    "rep3d_p2": lambda: _patches.patches("rep3d_p2"),          # repeated interior knots, non-uniform, bent net: 7 x 5 x 5
    "mix3d_322": lambda: _patches.patches("mix3d_322"),        # a different degree per axis: 5 x 4 x 4
}
NODES = {"p2_5x4x3": [5, 4, 3], "p2_35x4x4": [35, 4, 4], "p2_4x35x4": [4, 35, 4], "p2_4x4x35": [4, 4, 35], "p1_6x5x4": [6, 5, 4],
         "p3_10x6": [10, 6], "rep3d_p2": [7, 5, 5], "mix3d_322": [5, 4, 4]}
DIRICHLET = ("face", "component", "partial")


@functools.lru_cache(maxsize=None)
def grid(name):
    P, B = GRIDS[name]()
    assert list(P.n) == NODES[name] == list(B.n_ctrl)
    return P, B


def essential(P, kind):
    """face: every dof of the face axis 0 / side 0; component: component 1 of the face axis 1 / side 1; partial: every
    second node of the face axis 0 / side 0, all components -- which fills no face"""
    dim = P.dim
    if kind == "face":
        nodes = P.boundary_nodes(0, 0)
        return np.sort(np.concatenate([nodes * dim + c for c in range(dim)])).astype(np.int64)
    if kind == "component":
        return np.sort(P.boundary_nodes(1, 1) * dim + 1).astype(np.int64)
    if kind == "partial":
        nodes = P.boundary_nodes(0, 0)[::2]
        return np.sort(np.concatenate([nodes * dim + c for c in range(dim)])).astype(np.int64)
    if kind == "none":
        return np.zeros(0, dtype=np.int64)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def application(name, kind):
    """(r, z_ref): a standard normal right-hand side and the extended-precision application; shared, read-only"""
    P, _ = grid(name)
    dim = P.dim
    r = np.random.default_rng(17).standard_normal(P.n_nodes * dim)
    z = ref.apply_extended(P, essential(P, kind), dim, RHO, stiff(dim, APPLY_FAC0, APPLY_DAMPING), r)
    r.setflags(write=False)
    z.setflags(write=False)
    return r, z


# ---- the solves: J = M + fac0 K(u) on a bent block --------------------------------------------------------------------------
# name -> (elements, degree, lengths, clamped faces (axis, side))
SOLVES = {
    "p2_6x4x2": ((6, 4, 2), 2, [3.0, 2.0, 1.0], [(0, 0)]),
    "p3_4x3x2": ((4, 3, 2), 3, [2.0, 1.5, 1.0], [(0, 0), (1, 0)]),
    "2d_p3_8x4": ((8, 4), 3, [4.0, 2.0], [(0, 0)]),
}
FAC0 = (1e-2, 1.0)
# (case, fac0) -> iterations of the restated GMRES(50) on the oracle's tangent: (Jacobi, Kronecker)
ITERATIONS = {("p2_6x4x2", 1e-2): (442, 45), ("p2_6x4x2", 1.0): (346, 45),
              ("p3_4x3x2", 1e-2): (290, 30), ("p3_4x3x2", 1.0): (290, 31),
              ("2d_p3_8x4", 1e-2): (107, 26), ("2d_p3_8x4", 1.0): (160, 29)}
AMPLITUDE = 0.1     # of the longest side


@functools.lru_cache(maxsize=None)
def solve_patch(name):
    """(oracle patch, product patch) of a solve: the block with its control net bent (a smooth map, 8 % of the longest
    side), shared"""
    from oracle import iga
    n_el, p, lengths, _ = SOLVES[name]
    P0 = iga.Patch.block(n_el, p, lengths)
    X = np.asarray(P0.ctrl, dtype=np.float64).copy()
    L = max(lengths)
    s = X[:, 0] / lengths[0]
    X[:, 1] += 0.08 * L * np.sin(np.pi * s)
    X[:, 0] += 0.04 * L * s * (X[:, 1] / lengths[1] - 0.5)
    if len(n_el) == 3:
        X[:, 2] += 0.05 * L * s * s
    return _pair(iga.Patch(P0.p, P0.knots, X))


def solve_inputs(name):
    """(essential dofs, u, b): the clamped faces, a smooth displacement of AMPLITUDE x the longest side (zero on the face
    axis 0 / side 0), a standard normal right-hand side with zeros on the essential dofs"""
    P, _ = solve_patch(name)
    n_el, p, lengths, clamped = SOLVES[name]
    dim = P.dim
    ess = np.unique(np.concatenate([P.boundary_nodes(a, s)[:, None] * dim + np.arange(dim)[None, :] for a, s in clamped]).ravel())
    X0 = np.asarray(_pair_block(name).ctrl)
    s = X0[:, 0] / lengths[0]
    L = max(lengths)
    u = np.zeros((P.n_nodes, dim))
    u[:, 1] = AMPLITUDE * L * s * s
    u[:, 0] = -0.3 * AMPLITUDE * L * s * s * (X0[:, 1] / lengths[1] - 0.5)
    if dim == 3:
        u[:, 2] = 0.4 * AMPLITUDE * L * np.sin(0.5 * np.pi * s) * (X0[:, 1] / lengths[1])
    b = np.random.default_rng(23).standard_normal(P.n_nodes * dim)
    b[ess] = 0.0
    return ess.astype(np.int64), u.ravel(), b


@functools.lru_cache(maxsize=None)
def _pair_block(name):
    from oracle import iga
    n_el, p, lengths, _ = SOLVES[name]
    return iga.Patch.block(n_el, p, lengths)


@functools.lru_cache(maxsize=None)
def oracle_system(name, fac0):
    """J = M + fac0 K(u) from the oracle's exact neo-Hookean tangent, essential rows and columns eliminated (DIAG_ONE), as
    scipy CSR on the patch's own pattern; with the inputs"""
    from oracle import harness as hz, ref_path as rp
    from _cases import oracle_material
    P, _ = solve_patch(name)
    ess, u, b = solve_inputs(name)
    D = rp.DomainOracle(P, oracle_material("neohook"), n_threads=2)
    D.set_dt(1.0)
    vals = hz.assemble_mass(P, D.tables, RHO, D.rowptr, D.col)
    D.add_domain_residual_and_grad(u, fac0, np.zeros(P.n_vdofs), vals, rp.TANGENT_EXACT)
    hz.eliminate_row_col(D.rowptr, D.col, vals, ess)
    J = sp.csr_matrix((vals, D.col, D.rowptr), shape=(P.n_vdofs, P.n_vdofs))
    return types.SimpleNamespace(P=P, D=D, ess=ess, u=u, b=b, J=J)


def restated_solves(J, P, ess, b, fac0):
    """(GMRES + Jacobi, GMRES + the dense fp64 Kronecker operator) of the restatement"""
    dinv = 1.0 / J.diagonal()
    jac = ref.gmres(J, b, lambda v: dinv * v, max_iter=3000)
    kron = ref.gmres(J, b, ref.dense_preconditioner(P, ess, P.dim, RHO, stiff(P.dim, fac0)), max_iter=3000)
    return jac, kron
