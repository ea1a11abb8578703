"""csrc/kronecker.hpp through the C ABI (mimi_amd.linear.LinearSolver) on the table of tests/_kronecker_cases.py:

(a) one application z = P^-1 r, z[ess] = r[ess] against the extended-precision dense inverse of tests/_kronecker_reference.py
    on every node grid and Dirichlet configuration, within BAR x DEV_APPLY (the deviation the fp64 numpy application shows
    on the CPU, test_kronecker_cpu.py), and equal bits from two applications;
(b) solves of J = M + fac0 K(u), assembled by the device domain integrator on a bent block: GMRES with preconditioner id 2
    against the extended-precision direct solve within BAR x DEV_SOLVE, the iteration count of the numpy restatement, fewer
    iterations than the same handle's Jacobi solve; CG with id 2 on a mass matrix; ids 0 and 1 bit for bit what a handle
    without the operator gives;
(c) the reference's golden beams through the facade with "use_kronecker_preconditioner";
(d) the refusals."""
import numpy as np
import pytest
import scipy.sparse as sp

import _kronecker_cases as kc
import _kronecker_reference as ref
from _cases import product_material

pytestmark = pytest.mark.gpu


def _diagonal_pattern(n):
    from mimi_amd.integrators import CSRPattern
    return CSRPattern(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), n)


def _kronecker_solver(pattern, B, ess, dim, mass, stiff):
    from mimi_amd.kronecker import KroneckerOperator
    from mimi_amd.linear import LinearSolver
    S = LinearSolver(pattern, ess)
    S.SetKronecker(KroneckerOperator(B, ess, dim))
    S.SetKroneckerCoefficients(mass, stiff)
    return S


@pytest.mark.parametrize("kind", kc.DIRICHLET)
@pytest.mark.parametrize("name", list(kc.GRIDS))
def test_application_equals_the_extended_precision_inverse(name, kind):
    P, B = kc.grid(name)
    dim = P.dim
    ess = kc.essential(P, kind)
    r, z_ref = kc.application(name, kind)
    S = _kronecker_solver(_diagonal_pattern(P.n_nodes * dim), B, ess, dim, kc.RHO, kc.stiff(dim, kc.APPLY_FAC0, kc.APPLY_DAMPING))
    z = S.ApplyPreconditioner("kronecker", None, np.array(r), np.full(len(r), np.nan))
    again = S.ApplyPreconditioner(2, None, np.array(r), np.full(len(r), np.nan))
    dev = np.abs(z - z_ref).max() / np.abs(z_ref).max()
    print(f"\n{name} [{kind}]: z deviates {dev:.3g} (bar {kc.BAR * kc.DEV_APPLY:.3g})")
    assert np.isfinite(z).all()
    assert dev <= kc.BAR * kc.DEV_APPLY
    assert np.array_equal(z[ess], r[ess])
    assert z.tobytes() == again.tobytes()


def test_application_in_place_on_device_tensors():
    """z == r, both in HBM: the bits of the staged host call"""
    import torch
    name, kind = "p2_35x4x4", "face"
    P, B = kc.grid(name)
    ess = kc.essential(P, kind)
    r, _ = kc.application(name, kind)
    S = _kronecker_solver(_diagonal_pattern(len(r)), B, ess, P.dim, kc.RHO, kc.stiff(P.dim, kc.APPLY_FAC0, kc.APPLY_DAMPING))
    z = S.ApplyPreconditioner(2, None, np.array(r), np.zeros(len(r)))
    d = torch.from_numpy(np.array(r)).to(torch.device("cuda", 0))
    S.ApplyPreconditioner(2, None, d, d)
    assert d.cpu().numpy().tobytes() == z.tobytes()


def test_jacobi_application():
    """kind 1: z = r / diag(A)"""
    from mimi_amd.linear import LinearSolver
    n = 1000
    rng = np.random.default_rng(3)
    diag, r = 1.0 + rng.random(n), rng.standard_normal(n)
    S = LinearSolver(_diagonal_pattern(n))
    z = S.ApplyPreconditioner("jacobi", diag, r, np.zeros(n))
    assert np.array_equal(z, (1.0 / diag) * r)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def _device_system(name, fac0):
    """J = M + fac0 K(u) of the case assembled by the device integrator and eliminated by the solver handle; (handle with
    the Kronecker operator, J as scipy CSR, values, inputs)"""
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    P, B = kc.solve_patch(name)
    ess, u, b = kc.solve_inputs(name)
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    G.AddDomainResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    S = _kronecker_solver(pattern, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))
    S.Eliminate(None, vals)
    J = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs))
    return S, J, vals, P, ess, b


@pytest.mark.parametrize("fac0", kc.FAC0)
@pytest.mark.parametrize("name", list(kc.SOLVES))
def test_gmres_with_the_kronecker_preconditioner(name, fac0):
    S, J, vals, P, ess, b = _device_system(name, fac0)
    S.max_iter = 3000
    restated = ref.gmres(J, b, ref.dense_preconditioner(P, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0)), max_iter=3000)
    assert restated.converged and ref.margin(restated) >= kc.MARGIN
    S.preconditioner = "kronecker"
    x = S.Mult(vals, b, np.full(len(b), np.nan))
    it, converged = S.final_iter_, S.converged_
    S.preconditioner = "jacobi"
    S.Mult(vals, b, np.full(len(b), np.nan))
    it_jacobi = S.final_iter_
    x_ref = np.array([float(v) for v in ref.solve_extended(J, b)])
    dev = np.abs(x - x_ref).max() / np.abs(x_ref).max()
    print(f"\n{name} fac0 {fac0:g}: iterations Jacobi {it_jacobi} -> Kronecker {it} (restatement {restated.iterations}, on the oracle's "
          f"tangent {kc.ITERATIONS[(name, fac0)]}), margin {ref.margin(restated):.3g}, x deviates {dev:.3g} "
          f"(bar {kc.BAR * kc.DEV_SOLVE:.3g})")
    assert converged and np.isfinite(x).all()
    assert dev <= kc.BAR * kc.DEV_SOLVE
    assert it == restated.iterations
    assert it < it_jacobi


def test_ids_0_and_1_are_untouched_by_the_operator():
    """a handle that holds the operator solves with "none" and "jacobi" to the bits of a handle that never saw it; and one
    handle taken through changing matrix values and the ids 1, 2, 0, 2, 1 gives, at every solve, the bits of a fresh one"""
    from mimi_amd.linear import LinearSolver
    name, fac0 = "2d_p3_8x4", 1e-2
    S, J, vals, P, ess, b = _device_system(name, fac0)
    plain = LinearSolver(S.pattern_, ess)
    for preconditioner in ("jacobi", "none"):
        got = []
        for handle in (S, plain):
            handle.preconditioner = preconditioner
            x = handle.Mult(vals, b, np.full(len(b), np.nan))
            got.append((x.tobytes(), handle.final_iter_, handle.final_norm_, handle.converged_))
            x = handle.MultCG(vals, b, np.full(len(b), np.nan))
            got.append((x.tobytes(), handle.final_iter_, handle.final_norm_, handle.converged_))
        assert got[0] == got[2] and got[1] == got[3]
        assert got[0][1] > 1
    S.use_jacobi = False                       # the alias of old
    assert S.preconditioner == "none" and not S.use_jacobi
    # one handle through changing matrix values (rows scaled, so the diagonal moves) and alternating ids, 2 among them:
    # every solve gives the bytes of a handle made for it
    _, B = kc.solve_patch(name)
    rng = np.random.default_rng(73)
    rows = np.repeat(np.arange(P.n_vdofs), np.diff(np.asarray(S.pattern_.rowptr)))
    for preconditioner in ("jacobi", "kronecker", "none", "kronecker", "jacobi"):
        vals = vals * rng.uniform(0.5, 2.0, P.n_vdofs)[rows]
        got = []
        for handle in (S, _kronecker_solver(S.pattern_, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))):
            handle.preconditioner = preconditioner
            x = handle.Mult(vals, b, np.full(len(b), np.nan))
            got.append((x.tobytes(), handle.final_iter_, np.float64(handle.final_norm_).tobytes(), handle.converged_))
            x = handle.MultCG(vals, b, np.full(len(b), np.nan), max_iter=60)      # (no longer symmetric: a short leash)
            got.append((x.tobytes(), handle.final_iter_, np.float64(handle.final_norm_).tobytes(), handle.converged_))
        assert got[0] == got[2] and got[1] == got[3]
        assert got[0][1] > 1


@pytest.mark.parametrize("kind", ["face", "none"])
def test_cg_on_the_mass_matrix_of_an_affine_block(kind):
    """P with fac0 = 0 is the mass matrix of an affine block itself: conjugate gradients end after at most 2 iterations"""
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    P, B = kc.grid("p2_5x4x3")
    dim = P.dim
    ess = kc.essential(P, kind)
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    S = _kronecker_solver(pattern, B, ess, dim, kc.RHO, np.zeros(dim * dim))
    S.Eliminate(None, vals)
    b = np.random.default_rng(5).standard_normal(P.n_vdofs)
    b[ess] = 0.0
    S.preconditioner = "kronecker"
    x = S.MultCG(vals, b, np.full(len(b), np.nan))
    it = S.final_iter_
    S.preconditioner = "jacobi"
    S.MultCG(vals, b, np.full(len(b), np.nan))
    print(f"\nmass solve [{kind}]: CG iterations Jacobi {S.final_iter_} -> Kronecker {it}")
    assert it <= 2 and it < S.final_iter_
    M = sp.csr_matrix((vals, col, rowptr), shape=(len(b), len(b)))
    assert np.abs(M @ x - b).max() <= 1e-8 * np.abs(b).max()


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def _golden_steps(case, golden_dir, kronecker, steps=3):
    """the first `steps` steps of a golden beam on the iterative route; the GMRES iterations they took"""
    import os
    from oracle import harness as hz
    from test_nonlinear_solid import GOLDEN_CASES, beam
    runtime = [("use_iterative_solver", 1)] + ([("use_kronecker_preconditioner", 1)] if kronecker else [])
    nl = beam(case, runtime=runtime)
    assert nl.use_iterative_solver_ and nl.use_kronecker_ == kronecker
    assert nl.linear_.preconditioner == ("kronecker" if kronecker else "jacobi")
    total = [0]
    mult = nl.linear_.Mult

    def counted(*args):
        out = mult(*args)
        assert nl.linear_.converged_
        total[0] += nl.linear_.final_iter_
        return out
    nl.linear_.Mult = counted
    u = nl.solution_view("displacement", "x").ravel()
    for i in range(steps):
        nl.step_time2()
        golden = hz.golden_to_lexicographic(np.genfromtxt(os.path.join(golden_dir, "ref", GOLDEN_CASES[case]["refdir"], f"x_{i}.txt")))
        assert np.allclose(u, golden)                  # test_nonlinear_solid.py's criterion on the iterative route
    return total[0]


@pytest.mark.parametrize("case", ["neohook", "j2"])
def test_golden_beams_with_the_flag(golden_dir, case):
    with_flag = _golden_steps(case, golden_dir, True)
    without = _golden_steps(case, golden_dir, False)
    print(f"\n{case}: GMRES iterations of three steps, Jacobi {without} -> Kronecker {with_flag}")
    assert 0 < with_flag < without


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mimi_amd.kronecker import KroneckerOperator
    from mimi_amd.linear import LinearSolver
    P, B = kc.grid("p2_5x4x3")
    n = P.n_nodes * P.dim
    S = LinearSolver(_diagonal_pattern(n))
    S.preconditioner = "kronecker"
    ones = np.ones(n)
    with pytest.raises(RuntimeError, match="set_kronecker"):
        S.Mult(ones, ones, np.zeros(n))
    with pytest.raises(RuntimeError, match="set_kronecker"):
        S.MultCG(ones, ones, np.zeros(n))
    with pytest.raises(RuntimeError, match="set_kronecker"):
        S.ApplyPreconditioner(2, None, ones, np.zeros(n))
    with pytest.raises(RuntimeError, match="set_kronecker"):
        S.SetKroneckerCoefficients(1.0, np.zeros(9))
    other = LinearSolver(_diagonal_pattern(n + 3))
    with pytest.raises(RuntimeError, match="5 x 4 x 3 nodes"):
        other.SetKronecker(KroneckerOperator(B, [], P.dim))
    S.SetKronecker(KroneckerOperator(B, [], P.dim))
    with pytest.raises(RuntimeError, match="set_kronecker_coefficients"):
        S.Mult(ones, ones, np.zeros(n))
    S.preconditioner = "ilu"
    with pytest.raises(ValueError, match="ilu"):
        S.Mult(ones, ones, np.zeros(n))
