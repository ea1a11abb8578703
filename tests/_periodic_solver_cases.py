"""The inputs on which periodic pairs on the Kronecker and matrix-free solver routes are held to references: one table, used by
test_periodic_kronecker_cpu.py (mimi_amd/kronecker.py with periodic_axes, in numpy) and by test_periodic_solvers_gpu.py (the
folded product of csrc/krylov.hip and the device application through the C ABI).  The references are those of
tests/_kronecker_reference.py, folded here by dense 0/1 maps written from the definition: a periodic axis identifies its last
node plane with its first, folded nodes are numbered lexicographically on the grid without the last planes.

The DEV_* constants are MEASURED on the CPU (the convention of tests/_kronecker_cases.py: deviations of fp64 numpy computations
from the 50-digit references, never of what a kernel returns); the bars of both tests are kc.BAR = 20 times them.

    DEV_APPLY_PERIODIC = max over GRIDS of  max|z - z_ref| / max|z_ref|  of KroneckerOperator.apply (periodic_axes) against
                         the 50-digit solve of the dense folded operator
                         measured 1.08e-14 (per12_p3), recorded 1.1e-14, printed by
                         python -m pytest tests/test_periodic_kronecker_cpu.py::test_recorded_deviation_of_the_application -s
    DEV_SOLVE_PERIODIC = max over SOLVES x kc.FAC0 of  max|x - x_ref| / max|x_ref|  of the restated GMRES(50) with
                         KroneckerOperator.apply against solve_extended of the folded, eliminated system
                         measured 3.25e-08 (p2_6x4x2 axis 1, fac0 1e-2), recorded 3.3e-8, printed by
                         python -m pytest tests/test_periodic_kronecker_cpu.py::test_restated_solves -s
    ITERATIONS         = (Jacobi, Kronecker) of the restated GMRES(50) on the folded oracle tangent, same command
    CG_ITERATIONS      = the restated CG with KroneckerOperator.apply on the folded mass matrix of CG_CASE, printed by
                         python -m pytest tests/test_periodic_kronecker_cpu.py::test_restated_cg_on_the_folded_mass -s"""
import functools
import types

import numpy as np
import scipy.sparse as sp

import _kronecker_cases as kc
import _kronecker_reference as ref

DEV_APPLY_PERIODIC = 1.1e-14
DEV_SOLVE_PERIODIC = 3.3e-8


# ---- the fold, from its definition -------------------------------------------------------------------------------------------
def p1(n):
    """the n x (n - 1) 0/1 map of one periodic axis: function i -> i, the last one -> 0"""
    P = np.zeros((n, n - 1))
    P[np.arange(n - 1), np.arange(n - 1)] = 1.0
    P[n - 1, 0] = 1.0
    return P


def node_map(n, axes):
    """folded node of every unwrapped node of a grid of n[d] nodes per axis (axis 0 fastest), by plain loops"""
    n = [int(v) for v in n]
    m = [v - 1 if d in axes else v for d, v in enumerate(n)]
    out = np.zeros(int(np.prod(n)), dtype=np.int64)
    for a in range(len(out)):
        rest, folded, stride = a, 0, 1
        for d in range(len(n)):
            i = rest % n[d]
            rest //= n[d]
            folded += (i % m[d] if d in axes else i) * stride
            stride *= m[d]
        out[a] = folded
    return out


def node_fold(n, axes):
    """P_nodes: dense n_nodes_u x n_nodes_f"""
    nm = node_map(n, axes)
    P = np.zeros((len(nm), int(nm.max()) + 1))
    P[np.arange(len(nm)), nm] = 1.0
    return P


def dof_fold(n, axes, dim):
    """P on the vdofs (byVDIM), sparse n_u x n_f"""
    nm = node_map(n, axes)
    rows = np.arange(len(nm) * dim)
    cols = np.repeat(nm, dim) * dim + np.tile(np.arange(dim), len(nm))
    return sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(len(rows), (int(nm.max()) + 1) * dim))


def folded_face_dofs(P, axes, faces, components=None):
    """the folded essential dofs of clamped faces [(axis, side)] (on non-periodic axes), sorted and unique"""
    nm = node_map(P.n, axes)
    comps = range(P.dim) if components is None else components
    dofs = [nm[P.boundary_nodes(a, s)] * P.dim + c for a, s in faces for c in comps]
    return np.unique(np.concatenate(dofs)).astype(np.int64)


# ---- 1. the 1-D matrices -----------------------------------------------------------------------------------------------------
def knots_1d(p, spans, repeated):
    """open knot vector of degree p on [0, 1] with `spans` spans, uniform; repeated: the first interior knot twice"""
    inner = list(np.arange(1, spans) / spans)
    if repeated:
        inner = sorted(inner + inner[:1])
    return np.array([0.0] * (p + 1) + inner + [1.0] * (p + 1))


# (degree, spans, one interior knot repeated): 1 span has no interior knot
AXES_1D = [(p, m, rep) for p in (2, 3) for m in (1, 2, 5) for rep in (False, True) if not (rep and m == 1)]
LENGTH_1D = 2.5      # of the periodic axis; the other axis of the carrier patch is one element of degree 1 and length 1


def patch_1d(p, spans, repeated):
    """(knots, product patch): a 2-D carrier patch whose axis 0 has the knot vector under test, Greville control points
    scaled to LENGTH_1D"""
    import mimi_amd
    kn = knots_1d(p, spans, repeated)
    g = np.array([kn[i + 1:i + p + 1].mean() for i in range(len(kn) - p - 1)]) * LENGTH_1D
    ctrl = np.array([[x, y] for y in (0.0, 1.0) for x in g])
    return kn, mimi_amd.BSplinePatch([p, 1], [kn, np.array([0.0, 0.0, 1.0, 1.0])], ctrl)


# ---- 2. the dense folded operator ----------------------------------------------------------------------------------------------
# name -> (elements, degree, lengths, periodic axes, clamped face on a non-periodic axis); folded node counts along the
# periodic axis 2, 16 and 17 (the first count and the two around the 16-wide tile of csrc/kronecker.hpp), in every position
GRIDS = {
    "per0_2": ((1, 2, 1), 2, [1.0, 1.5, 0.5], (0,), (1, 0)),
    "per0_16": ((15, 1, 1), 2, [4.0, 1.0, 0.5], (0,), (1, 1)),
    "per0_17": ((16, 1, 1), 2, [4.0, 1.0, 0.5], (0,), (2, 0)),
    "per1_2": ((2, 1, 1), 2, [1.5, 1.0, 0.5], (1,), (0, 0)),
    "per1_16": ((1, 15, 1), 2, [1.0, 4.0, 0.5], (1,), (0, 1)),
    "per1_17": ((1, 16, 1), 2, [1.0, 4.0, 0.5], (1,), (2, 1)),
    "per2_2": ((1, 2, 1), 2, [1.0, 1.5, 0.5], (2,), (1, 0)),
    "per2_16": ((1, 1, 15), 2, [1.0, 0.5, 4.0], (2,), (0, 0)),
    "per2_17": ((1, 1, 16), 2, [1.0, 0.5, 4.0], (2,), (1, 1)),
    "per02_16_2": ((15, 2, 1), 2, [4.0, 1.5, 0.5], (0, 2), (1, 0)),
    "per12_p3": ((2, 3, 2), 3, [1.0, 1.5, 1.0], (1, 2), (0, 1)),
    "2d_per1_p3": ((3, 4), 3, [1.5, 2.0], (1,), (0, 0)),
    "2d_per0_17": ((16, 2), 2, [4.0, 1.0], (0,), (1, 1)),
}


@functools.lru_cache(maxsize=None)
def grid(name):
    """(oracle patch, product patch, periodic axes, folded essential dofs, folded nodes per axis)"""
    from oracle import iga
    n_el, p, lengths, axes, face = GRIDS[name]
    P, B = kc._pair(iga.Patch.block(n_el, p, lengths))
    ess = folded_face_dofs(P, axes, [face])
    n_dir = [int(v) - (d in axes) for d, v in enumerate(P.n)]
    return P, B, axes, ess, n_dir


def folded_component_operator(P, axes, c, mass, stiff):
    """P_nodes^T P_c P_nodes, dense on all folded nodes (nothing removed)"""
    full = [[np.ones(P.n[d], dtype=bool) for d in range(P.dim)] for _ in range(P.dim)]
    Pc, nodes = ref.component_operator(P, c, mass, stiff, full)
    assert np.array_equal(nodes, np.arange(P.n_nodes))
    Pn = node_fold(P.n, axes)
    return Pn.T @ Pc @ Pn


@functools.lru_cache(maxsize=None)
def application(name):
    """(r, z_ref): a standard normal right-hand side of the folded size and the 50-digit application of the dense folded
    operator, z[ess] = r[ess]; shared, read-only"""
    P, _, axes, ess, n_dir = grid(name)
    dim = P.dim
    n_f = int(np.prod(n_dir))
    r = np.random.default_rng(17).standard_normal(n_f * dim)
    z = np.zeros(n_f * dim)
    is_ess = np.zeros(n_f * dim, dtype=bool)
    is_ess[ess] = True
    for c in range(dim):
        Pf = folded_component_operator(P, axes, c, kc.RHO, kc.stiff(dim, kc.APPLY_FAC0, kc.APPLY_DAMPING))
        free = np.nonzero(~is_ess[c::dim])[0]
        z[free * dim + c] = [float(v) for v in ref.solve_extended(Pf[np.ix_(free, free)], r[free * dim + c])]
    z[ess] = r[ess]
    r.setflags(write=False)
    z.setflags(write=False)
    return r, z


# ---- 4. the folded solves ----------------------------------------------------------------------------------------------------
# (case of kc.SOLVES, periodic axis) -- the clamped faces of the cases lie on other axes
SOLVES = [("p2_6x4x2", 1), ("p2_6x4x2", 2), ("p3_4x3x2", 2), ("2d_p3_8x4", 1)]
# (case, axis, fac0) -> iterations of the restated GMRES(50) on the folded oracle tangent: (Jacobi, Kronecker)
ITERATIONS = {("p2_6x4x2", 1, 1e-2): (128, 28), ("p2_6x4x2", 1, 1.0): (260, 32),
              ("p2_6x4x2", 2, 1e-2): (113, 25), ("p2_6x4x2", 2, 1.0): (167, 26),
              ("p3_4x3x2", 2, 1e-2): (283, 20), ("p3_4x3x2", 2, 1.0): (283, 20),
              ("2d_p3_8x4", 1, 1e-2): (82, 18), ("2d_p3_8x4", 1, 1.0): (85, 18)}
CG_CASE = ("p2_6x4x2", 2)
CG_ITERATIONS = 5


def eliminate(A, ess):
    """EliminateRowCol(ess, DIAG_ONE) on a scipy matrix"""
    A = sp.lil_matrix(A)
    keep = np.ones(A.shape[0])
    keep[ess] = 0.0
    D = sp.diags(keep)
    return sp.csr_matrix(D @ sp.csr_matrix(A) @ D + sp.diags(1.0 - keep))


@functools.lru_cache(maxsize=None)
def unwrapped_matrices(name, fac0):
    """(mass matrix rho M, tangent J_u = rho M + fac0 K(u)) of the oracle on the unwrapped patch, nothing eliminated"""
    from oracle import harness as hz, ref_path as rp
    from _cases import oracle_material
    P, _ = kc.solve_patch(name)
    _, u, _ = kc.solve_inputs(name)
    D = rp.DomainOracle(P, oracle_material("neohook"), n_threads=2)
    D.set_dt(1.0)
    mass = hz.assemble_mass(P, D.tables, kc.RHO, D.rowptr, D.col)
    vals = mass.copy()
    D.add_domain_residual_and_grad(u, fac0, np.zeros(P.n_vdofs), vals, rp.TANGENT_EXACT)
    shape = (P.n_vdofs, P.n_vdofs)
    return sp.csr_matrix((mass, D.col, D.rowptr), shape=shape), sp.csr_matrix((vals, D.col, D.rowptr), shape=shape)


@functools.lru_cache(maxsize=None)
def folded_system(name, axis, fac0):
    """J_f = P^T (rho M + fac0 K(u)) P of the oracle's tangent, the essential dofs eliminated AFTER the fold; the right-hand
    side default_rng(23) of the folded size, zero on them"""
    P, B = kc.solve_patch(name)
    clamped = kc.SOLVES[name][3]
    assert all(a != axis for a, _ in clamped)
    ess = folded_face_dofs(P, (axis,), clamped)
    Pm = dof_fold(P.n, (axis,), P.dim)
    M_u, J_u = unwrapped_matrices(name, fac0)
    b = np.random.default_rng(23).standard_normal(Pm.shape[1])
    b[ess] = 0.0
    _, u, _ = kc.solve_inputs(name)
    return types.SimpleNamespace(P=P, B=B, axes=(axis,), ess=ess, u=u, b=b, fold=Pm, J=eliminate(Pm.T @ J_u @ Pm, ess),
                                 M=eliminate(Pm.T @ M_u @ Pm, ess))


# ---- 11. the consistent-mass route with a pair: tests/_explicit_cases.py: cm_run, folded ----------------------------------------
# cube_p2 with the opposite faces of attributes 3 and 5 joined, the bottom clamped; the oracle's matrices folded by P, the
# reference solved by scipy's LU, the iteration counts from the restated CG with KroneckerOperator(periodic_axes).  Step, velocity
# scale and the derivation of the bars (a second run with every residual entry moved by its own bar and the restated CG; spread /
# MARGIN) are those of the unfolded runs.
CM_CASE, CM_PAIR = "cube_p2", (3, 5)


@functools.lru_cache(maxsize=None)
def _cm_setting():
    """(oracle patch, product patch, periodic axis, dof fold, fixed folded dofs as a mask)"""
    import _explicit_cases as ec
    nl = ec.facade(CM_CASE, "neohook", setup=False)
    (a0, s0), (a1, s1) = nl._faces[CM_PAIR[0]], nl._faces[CM_PAIR[1]]
    assert a0 == a1 and s0 != s1
    P = ec.oracle_patch(CM_CASE)
    Pm = dof_fold(P.n, (a0,), P.dim)
    fixed = (Pm.T @ ec.clamped_bottom(P).astype(float)) > 0
    return P, nl.patch(), a0, Pm, fixed


def cm_initial_velocity():
    """the unfolded runs' velocity at the lowest copy of every folded node"""
    import _explicit_cases as ec
    P, _, _, Pm, _ = _cm_setting()
    v_u = ec.cm_initial_velocity(P)
    first = np.full(Pm.shape[1], -1, dtype=np.int64)
    for i in range(Pm.shape[0] - 1, -1, -1):
        first[Pm.indices[i]] = i
    return v_u[first]


def cm_run(run, solver="lu", perturb=False):
    import scipy.sparse.linalg as spla
    import _explicit_cases as ec
    from mimi_amd.kronecker import KroneckerOperator, stiffness_coefficients
    from oracle import harness as hz, ref_path as rp
    matname, eta = ec.CM_RUNS[run]
    P, B, axis, Pm, fixed = _cm_setting()
    om, pm = ec.material_pair(matname)
    D = rp.DomainOracle(P, om)
    dt = ec.CM_DT
    D.set_dt(dt)
    n_u, dim = P.n_vdofs, P.dim
    ess = np.flatnonzero(fixed)
    csr = lambda vals: sp.csr_matrix((vals, D.col, D.rowptr), shape=(n_u, n_u))
    M = Pm.T @ csr(hz.assemble_mass(P, D.tables, ec.RHO, D.rowptr, D.col)) @ Pm
    C = Pm.T @ csr(hz.assemble_viscosity(P, D.tables, eta, D.rowptr, D.col)) @ Pm if eta else None
    keep = sp.diags((~fixed).astype(float))
    op = KroneckerOperator(B, ess, dim, periodic_axes=(axis,))
    rng = np.random.default_rng(77)
    iterations = []

    def solve(fac1, b):
        A = M + fac1 * C if eta else M
        A = (keep @ A @ keep + sp.diags(fixed.astype(float))).tocsc()
        b = np.where(fixed, 0.0, b)
        if solver == "lu":
            return spla.splu(A).solve(b)
        stiff = stiffness_coefficients(pm.lambda_, pm.mu, 0.0, fac1, eta or -1.0, dim)
        s = ref.cg(A.tocsr(), b, lambda v: op.apply(v, ec.RHO, stiff))
        assert s[3], "the restated CG did not converge"
        iterations.append(s[1])
        return s[0]

    def rhs(x, v):
        x_u = Pm @ x
        r = np.zeros(n_u)
        D.add_domain_residual(x_u, r)
        if perturb:
            r = r + ec._residual_perturbation(P, D, matname, r, x_u, rng)
        return -(Pm.T @ r) - (C @ v if eta else 0.0)

    x, v = np.zeros(Pm.shape[1]), np.where(fixed, 0.0, cm_initial_velocity())
    a = solve(0.0, rhs(x, v))
    for _ in range(ec.STEPS):
        v = v + (0.5 * dt) * a
        x = x + dt * v
        a = solve(0.5 * dt, rhs(x, v))
        v = v + (0.5 * dt) * a
        D.domain_post_time_advance(Pm @ x)
    return types.SimpleNamespace(x=x, v=v, a=a, eqps=D.eqps.copy(), iterations=iterations)


@functools.lru_cache(maxsize=None)
def cm_reference(run):
    """(the LU run, the restated-CG run with its iteration counts, bar of x, bar of v, bar of eqps), as ec.cm_reference"""
    import _explicit_cases as ec
    import _radial_return as rr
    lu, cg, moved = cm_run(run), cm_run(run, solver="cg"), cm_run(run, solver="cg", perturb=True)
    spread = lambda a, b: float(np.abs(a - b).max()) / ec.MARGIN
    return lu, cg, spread(lu.x, moved.x), spread(lu.v, moved.v), spread(lu.eqps, moved.eqps) + ec.STEPS * 2.0 * rr.SOLVER_XTOL
