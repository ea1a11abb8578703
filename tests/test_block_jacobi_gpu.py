"""Node-block Jacobi (preconditioner id 3) and Jacobi from the operator's diagonal (id 1, armed, no matrix values) of
csrc/krylov.hip through mimi_amd.linear.LinearSolver.

CSR route, on the systems of tests/_block_jacobi_cases.py:
(1) ApplyPreconditioner(3, values, r) against a long-double block solve per node, within bc.apply_bar;
(2) GMRES with id 3 against the 120-digit GMRES on (M A, M b), CG with id 3 against the 120-digit CG on (C^T A C, C^T b): equal
    iteration counts (every case keeps the margin: test_block_jacobi_cpu.py), x within BAR x DEV_X;
(3) essential dofs inside a block; the refusals.
Operator route, on the systems of test_matrix_free_gpu.py::_operator_system:
(4) "jacobi" armed with None values against "jacobi" with the values, "block_jacobi" with None against with the values:
    ApplyPreconditioner within dc.tangent_bar, equal iteration counts, x within kc.BAR x kc.DEV_SOLVE of the extended-precision
    solve, and the counts of the fp64 restatement with the preconditioner as a callable where its margin holds;
(5) a J2 system beyond yield (the record route); (6) a periodic system through SetOperatorFold against the folded assembled
    matrix; (7) unarmed, "jacobi" with None values still asks for the matrix values."""
import numpy as np
import pytest
import scipy.sparse as sp

import _block_jacobi_cases as bc
import _domain_cases as dc
import _kronecker_cases as kc
import _kronecker_reference as ref
import _periodic_solver_cases as pc
from _cases import product_material

pytestmark = pytest.mark.gpu


def _solver(A, essential=None, vdim=None):
    from mimi_amd.integrators import CSRPattern
    from mimi_amd.linear import LinearSolver
    S = LinearSolver(CSRPattern(A.indptr.astype(np.int64), A.indices.astype(np.int32), len(A.indices)), essential)
    if vdim:
        S.SetNodeBlock(vdim)
    S.preconditioner = "block_jacobi"
    return S


def _solve(S, name, val, b):
    st = bc.settings(name)
    x = np.full(len(b), np.nan)
    if bc.CASES[name][0] == "gmres":
        S.rel_tol, S.abs_tol, S.max_iter, S.kdim = st["rel_tol"], st["abs_tol"], st["max_iter"], st["kdim"]
        S.Mult(val, np.array(b), x)
    else:
        S.MultCG(val, np.array(b), x, rel_tol=st["rel_tol"], abs_tol=st["abs_tol"], max_iter=st["max_iter"])
    return x


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bc.CASES))
def test_application_against_a_long_double_block_solve(name):
    A, b = bc.system(name)
    vdim = bc.CASES[name][2]
    S = _solver(A, vdim=vdim)
    r = np.random.default_rng(2).standard_normal(len(b))
    z = S.ApplyPreconditioner("block_jacobi", np.array(A.data), np.array(r), np.full(len(b), np.nan))
    want = bc.block_solve_extended(A, vdim, r)
    dev = np.abs(z - want).max() / np.abs(want).max()
    print(f"\n{name}: z deviates {dev:.3g} (bar {bc.apply_bar(A, vdim):.3g})")
    assert dev <= bc.apply_bar(A, vdim)
    # in place, and by number
    z2 = np.array(r)
    S.ApplyPreconditioner(3, np.array(A.data), z2, z2)
    assert z2.tobytes() == z.tobytes()


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bc.CASES))
def test_device_solver_equals_reference(name):
    A, b = bc.system(name)
    S = _solver(A, vdim=bc.CASES[name][2])
    x = _solve(S, name, np.array(A.data), b)
    s, x64 = bc.reference(name)
    dx = float(np.abs(x - x64).max() / np.abs(x64).max())
    print(f"\n{name}: iterations {S.final_iter_} (reference {s.iterations}), x deviates {dx:.3g} (bar {bc.BAR * bc.DEV_X:.3g}), "
          f"final norm {S.final_norm_:.6e} (reference {float(s.final_norm):.6e})")
    assert S.converged_ and s.converged and np.isfinite(x).all()
    assert S.final_iter_ == s.iterations
    assert dx <= bc.BAR * bc.DEV_X
    assert abs(S.final_norm_ - float(s.final_norm)) <= 1e-6 * float(s.goal)


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
def test_essential_dofs_inside_a_block():
    name = "nodes12x3"
    A, b = bc.system(name)
    S = _solver(A, essential=bc.ESSENTIAL, vdim=3)
    vals = np.array(A.data)
    S.Eliminate(None, vals)
    Ae = bc.eliminated(A, bc.ESSENTIAL)
    assert vals.tobytes() == Ae.data.tobytes()
    r = np.random.default_rng(2).standard_normal(len(b))
    z = S.ApplyPreconditioner("block_jacobi", vals, np.array(r), np.full(len(b), np.nan))
    want = bc.block_solve_extended(Ae, 3, r)
    assert np.abs(z - want).max() <= bc.apply_bar(Ae, 3) * np.abs(want).max()
    assert (z[bc.ESSENTIAL] == r[bc.ESSENTIAL]).all()
    # the blocks are eliminated like the matrix, whether the caller's values already are or not
    assert S.ApplyPreconditioner("block_jacobi", np.array(A.data), np.array(r), np.full(len(b), np.nan)).tobytes() == z.tobytes()
    be = np.array(b)
    be[bc.ESSENTIAL] = 0.0
    x = _solve(S, name, vals, be)
    s, x64 = bc.reference(name, with_essential=True)
    dx = float(np.abs(x - x64).max() / np.abs(x64).max())
    print(f"\n{name} with essential dofs: iterations {S.final_iter_} (reference {s.iterations}), x deviates {dx:.3g}")
    assert S.converged_ and S.final_iter_ == s.iterations and dx <= bc.BAR * bc.DEV_X
    assert not x[bc.ESSENTIAL].any()


def test_refusals():
    A, b = bc.system("nodes12x3")
    nan = lambda: np.full(len(b), np.nan)
    S = _solver(A)
    with pytest.raises(RuntimeError, match="set_node_block"):
        S.Mult(np.array(A.data), np.array(b), nan())
    with pytest.raises(RuntimeError, match="set_node_block"):
        S.MultCG(np.array(A.data), np.array(b), nan())
    with pytest.raises(RuntimeError, match="set_node_block"):
        S.ApplyPreconditioner("block_jacobi", np.array(A.data), np.array(b), nan())
    A2, b2 = bc.system("nodes17x2")
    with pytest.raises(RuntimeError, match="no multiple of dim 3"):
        _solver(A2).SetNodeBlock(3)
    with pytest.raises(RuntimeError, match="dim 4"):
        S.SetNodeBlock(4)
    # a singular block: the error names the node
    S.SetNodeBlock(3)
    vals = np.array(A.data)
    D = sp.csr_matrix((np.arange(len(vals), dtype=np.float64), A.indices, A.indptr), shape=A.shape).toarray().astype(np.int64)
    vals[D[15:18, 15:18].ravel()] = 0.0
    for solve in (lambda: S.Mult(vals, np.array(b), nan()), lambda: S.MultCG(vals, np.array(b), nan()),
                  lambda: S.ApplyPreconditioner("block_jacobi", vals, np.array(b), nan())):
        with pytest.raises(RuntimeError, match="block of node 5 is singular"):
            solve()
    vals[D[6:9, 6:9].ravel()] = np.nan
    with pytest.raises(RuntimeError, match="block of node 2 is singular or not finite"):
        S.Mult(vals, np.array(b), nan())
    # without values and without an operator
    with pytest.raises(RuntimeError, match="no operator is set"):
        S.Mult(None, np.array(b), nan())
    # the handle still solves
    x = _solve(S, "nodes12x3", np.array(A.data), b)
    assert S.converged_ and np.abs(A @ x - b).max() <= 1e-6 * np.abs(b).max()


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
def _callables(J, dim):
    dinv = 1.0 / J.diagonal()
    return {"jacobi": lambda v: dinv * v, "block_jacobi": bc.block_callable(J, dim)}


def _compare_routes(S, J, vals, b, dim, bar_apply, bar_x, label, restated=True):
    """both preconditioners with None values against with the values, on a solver whose operator is set and linearised"""
    S.SetNodeBlock(dim)
    S.SetOperatorDiagonal(True)
    S.max_iter = 3000
    x_ref = np.array([float(v) for v in ref.solve_extended(J, b)])
    r = np.random.default_rng(4).standard_normal(len(b))
    nan = lambda: np.full(len(b), np.nan)
    for kind, precond in _callables(J, dim).items():
        S.preconditioner = kind
        z_op = S.ApplyPreconditioner(kind, None, np.array(r), nan())
        z_csr = S.ApplyPreconditioner(kind, vals, np.array(r), nan())
        dz = np.abs(z_op - z_csr).max() / np.abs(z_csr).max()
        x_op = S.Mult(None, np.array(b), nan())
        it_op, conv_op = S.final_iter_, S.converged_
        x_csr = S.Mult(vals, np.array(b), nan())
        it_csr, conv_csr = S.final_iter_, S.converged_
        dev_op = np.abs(x_op - x_ref).max() / np.abs(x_ref).max()
        dev_csr = np.abs(x_csr - x_ref).max() / np.abs(x_ref).max()
        line = (f"\n{label} {kind}: application deviates {dz:.2e} (bar {bar_apply:.2e}); iterations operator {it_op}, values {it_csr}"
                f"; x deviates {dev_op:.3g} / {dev_csr:.3g} (bar {bar_x:.3g})")
        if restated:
            s = ref.gmres(J, b, precond, max_iter=3000)
            line += f"; restatement {s.iterations}, margin {ref.margin(s):.2e}"
        print(line)
        assert dz <= bar_apply
        assert conv_op and conv_csr and np.isfinite(x_op).all()
        assert it_op == it_csr
        assert dev_op <= bar_x and dev_csr <= bar_x
        if restated and s.converged and ref.margin(s) >= kc.MARGIN:
            assert it_op == s.iterations


@pytest.mark.parametrize("fac0", kc.FAC0)
@pytest.mark.parametrize("name", list(kc.SOLVES))
def test_operator_route_against_the_values(name, fac0):
    from test_matrix_free_gpu import _operator_system
    G, S, J, vals, P, ess, u, b = _operator_system(name, fac0)
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(np.array(u))
    _compare_routes(S, J, vals, b, P.dim, dc.tangent_bar("neohook"), kc.BAR * kc.DEV_SOLVE, f"{name} fac0 {fac0:g}")


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
def test_j2_beyond_yield():
    """the record route: J2 committed beyond yield at 0.5 u (half of the points plastic), linearised further along at 0.7 u; the
    coefficient of a time step (fac0 1e-2): at fac0 1 the small-strain law's tangent is indefinite under these rotations and the
    restated GMRES(50) stalls with either preconditioner"""
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from mimi_amd.linear import LinearSolver
    name, fac0 = "p2_6x4x2", 1e-2
    P, B = kc.solve_patch(name)
    ess, u, b = kc.solve_inputs(name)
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("j2"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    G.DomainPostTimeAdvance(0.5 * u)
    eqps = np.asarray(G.State("accumulated_plastic_strain"))
    share = float((eqps > 0).mean())
    print(f"\nplastic share of the commit {share:.2f}")
    assert 0.25 < share < 0.75
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    G.AddDomainResidualAndGrad(0.7 * u, fac0, np.zeros(P.n_vdofs), vals)
    S = LinearSolver(pattern, ess)
    S.Eliminate(None, vals)
    J = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs))
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(0.7 * u)
    assert G.LinearizationBytes() > 0
    _compare_routes(S, J, vals, b, P.dim, dc.tangent_bar("j2"), kc.BAR * kc.DEV_SOLVE, "j2 beyond yield")


# ---- (6) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, axis", [("p2_6x4x2", 1), ("2d_p3_8x4", 1)])
def test_periodic_system_through_the_fold(name, axis):
    """at least two knot spans on the periodic axis (4): no element holds both copies of a node, and the sum over the copies is
    the diagonal of P^T A P"""
    import torch
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from mimi_amd.linear import LinearSolver
    from test_periodic_solvers_gpu import _fold
    fac0 = kc.FAC0[0]
    assert kc.SOLVES[name][0][axis] >= 2
    sysm = pc.folded_system(name, axis, fac0)
    P, B = sysm.P, sysm.B
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    fold = _fold(pattern, P.n, sysm.axes, P.dim)
    folded = fold.Pattern()
    S = LinearSolver(folded, sysm.ess)
    S.SetOperatorFold(fold)
    # the folded assembled matrix: the device assembly on the unwrapped pattern, folded and eliminated on the device
    dev = torch.device("cuda", 0)
    vals_u = torch.zeros(len(col), dtype=torch.float64, device=dev)
    G.AddMass(kc.RHO, vals_u)
    G.AddDomainResidualAndGrad(torch.from_numpy(np.array(sysm.u)).to(dev), fac0, torch.zeros(P.n_vdofs, dtype=torch.float64, device=dev), vals_u)
    vals_f = torch.zeros(folded.nnz, dtype=torch.float64, device=dev)
    fold.Add(None, None, vals_u, None, vals_f)
    S.Eliminate(None, vals_f)
    G.Synchronize()
    vals = vals_f.cpu().numpy()
    J = sp.csr_matrix((vals, np.asarray(folded.col), np.asarray(folded.rowptr)), shape=(len(sysm.b), len(sysm.b)))
    assert abs(J - sysm.J).max() <= 1e-9 * abs(sysm.J).max()
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(np.array(sysm.u))
    _compare_routes(S, J, vals, sysm.b, P.dim, dc.tangent_bar("neohook"), kc.BAR * pc.DEV_SOLVE_PERIODIC, f"{name} axis {axis} folded")


# ---- (7) ---------------------------------------------------------------------------------------------------------------------
def test_unarmed_jacobi_still_needs_the_values():
    from test_matrix_free_gpu import _operator_system
    name, fac0 = "2d_p3_8x4", 1e-2
    G, S, J, vals, P, ess, u, b = _operator_system(name, fac0)
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(np.array(u))
    nan = lambda: np.full(len(b), np.nan)
    S.preconditioner = "jacobi"
    for _ in range(2):
        with pytest.raises(RuntimeError, match="matrix values"):
            S.Mult(None, b, nan())
        with pytest.raises(RuntimeError, match="matrix values"):
            S.MultCG(None, b, nan())
        with pytest.raises(RuntimeError, match="matrix values"):
            S.ApplyPreconditioner("jacobi", None, np.array(b), nan())
        S.SetOperatorDiagonal(True)
        x = S.Mult(None, b, nan())
        assert S.converged_ and np.abs(J @ x - b).max() <= 1e-6 * np.abs(b).max()
        S.SetOperatorDiagonal(False)
    # armed, but before a Linearize: the refusal of the action
    G2, S2, *_ = _operator_system(name, fac0)
    S2.SetOperator(G2, kc.RHO, fac0, 0.0)
    S2.SetOperatorDiagonal(True)
    S2.preconditioner = "jacobi"
    with pytest.raises(RuntimeError, match="before any mimi_hip_domain_linearize"):
        S2.Mult(None, b, nan())
    # armed, on an operator without a diagonal (every coefficient zero): the error names the first free dof (0 and 1 are clamped)
    assert ess[0] == 0 and ess[1] == 1 and 2 not in ess
    S.SetOperatorDiagonal(True)
    S.SetOperator(G, 0.0, 0.0, 0.0)
    for solve in (lambda: S.Mult(None, b, nan()), lambda: S.ApplyPreconditioner("jacobi", None, np.array(b), nan())):
        with pytest.raises(RuntimeError, match="diagonal entry of dof 2 is zero or not finite"):
            solve()
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    S.SetOperatorDiagonal(False)
    # armed, with values: the bits of a solve that never saw the setting
    S.SetOperatorDiagonal(True)
    S.max_iter = 300
    armed = S.Mult(vals, b, nan())
    S.SetOperatorDiagonal(False)
    assert S.Mult(vals, b, nan()).tobytes() == armed.tobytes()
