"""mimi_amd/kronecker.py (host side of the Kronecker preconditioner) against the oracle's assemblies and the
references of tests/_kronecker_reference.py, without a device; measures the DEV_* constants of tests/_kronecker_cases.py."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _kronecker_cases as kc
import _kronecker_reference as ref
import _patches

# affine blocks: (elements, degree, lengths); rounding bar of tests 1 and 2: 1e-12 x the largest entry -- the entries are sums of
# at most 27 x 125 products of O(1) factors, each off by a few ulp (about 4e-13 in all at the worst), and the assemblies
# measure 2e-14 apart
AFFINE = [((3, 2, 1), 2, [1.5, 1.0, 0.5]), ((4, 3, 2), 3, [2.0, 3.0, 1.0]), ((3, 2, 2), 1, [1.0, 1.0, 1.0]), ((5, 3), 3, [5.0, 1.0]),
          ((4, 3), 2, [1.0, 2.0])]
ROUNDING = 1e-12


def _product(P):
    return kc._pair(P)[1]


def _component_blocks(P, vals, rowptr, col):
    """the diagonal blocks (component c against component c) of a matrix on the vdof pattern, dense"""
    A = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs)).toarray()
    return [A[c::P.dim, c::P.dim] for c in range(P.dim)]


@pytest.mark.parametrize("n_el, p, lengths", AFFINE)
def test_mass_term_equals_the_assembled_mass_matrix(n_el, p, lengths):
    from mimi_amd.kronecker import KroneckerOperator
    from oracle import harness as hz, iga
    P = iga.Patch.block(n_el, p, lengths)
    op = KroneckerOperator(_product(P), [], P.dim)
    assert np.allclose(op.lengths, lengths, rtol=1e-14)
    rowptr, col = P.sparsity()
    blocks = _component_blocks(P, hz.assemble_mass(P, P.tables(), 1.0, rowptr, col), rowptr, col)
    kron = ref._kron(op.M)
    for c in range(P.dim):
        assert np.abs(kron - blocks[c]).max() <= ROUNDING * np.abs(blocks[c]).max()


@pytest.mark.parametrize("n_el, p, lengths", AFFINE)
def test_stiffness_term_equals_the_tangent_at_rest(n_el, p, lengths):
    """at u = 0 the exact neo-Hookean tangent is linear elasticity: its (c, c) block is sum_d e_cd K_d (x) M..."""
    from mimi_amd.kronecker import KroneckerOperator, stiffness_coefficients
    from oracle import iga, ref_path as rp
    from _cases import oracle_material
    P = iga.Patch.block(n_el, p, lengths)
    dim = P.dim
    D = rp.DomainOracle(P, oracle_material("neohook"), n_threads=2)
    D.set_dt(1.0)
    vals = np.zeros(D.nnz)
    D.add_domain_residual_and_grad(np.zeros(P.n_vdofs), 1.0, np.zeros(P.n_vdofs), vals, rp.TANGENT_EXACT)
    blocks = _component_blocks(P, vals, D.rowptr, D.col)
    op = KroneckerOperator(_product(P), [], dim)
    lam, mu = rp.lame(kc.YOUNG, kc.POISSON)[:2]
    e = stiffness_coefficients(lam, mu, 1.0, dim=dim).reshape(dim, dim)
    assert np.array_equal(e, kc.stiff(dim, 1.0))
    for c in range(dim):
        kron = sum(e[c, d] * ref._kron([op.K[a] if a == d else op.M[a] for a in range(dim)]) for d in range(dim))
        assert np.abs(kron - blocks[c]).max() <= ROUNDING * np.abs(blocks[c]).max()


@pytest.mark.parametrize("case", ["rep2d_p2", "rep3d_p2", "rep3d_p3", "nonuni3d_p2", "nonuni3d_p3", "mix2d_31", "mix3d_231", "mix3d_322"])
def test_eigenvectors_are_orthonormal_and_diagonalise(case):
    """U^T M U = I and U^T K U = diag(lam) on repeated interior knots, non-uniform knots and mixed degrees; the 1-D
    matrices equal the reference's own Gauss loop"""
    from mimi_amd.kronecker import KroneckerOperator
    P, B = _patches.patches(case)
    op = KroneckerOperator(B, kc.essential(P, "face"), P.dim)
    for d, (M, K) in enumerate(ref.scaled_matrices(P)):
        assert np.abs(op.M[d] - M).max() <= 1e-13 * np.abs(M).max() and np.abs(op.K[d] - K).max() <= 1e-13 * np.abs(K).max()
    for c in range(P.dim):
        for d in range(P.dim):
            U, lam, keep = op.U_cd[c][d], op.lam_cd[c][d], op.kept[c][d]
            nk = int(keep.sum())
            assert nk == P.n[d] - (1 if d == 0 else 0)
            assert not U[~keep].any() and not U[:, nk:].any() and (lam[nk:] == -1.0).all() and (lam[:nk] >= 0.0).all()
            I = U.T @ op.M[d] @ U
            assert np.abs(I[:nk, :nk] - np.eye(nk)).max() <= 1e-12
            L = U.T @ op.K[d] @ U
            assert np.abs(L[:nk, :nk] - np.diag(lam[:nk])).max() <= 1e-12 * max(lam[:nk].max(), 1.0)


def test_face_rule():
    from mimi_amd.kronecker import KroneckerOperator
    P, B = kc.grid("p2_5x4x3")
    removed = lambda kind: [[np.nonzero(~k)[0].tolist() for k in kk] for kk in KroneckerOperator(B, kc.essential(P, kind), 3).kept]
    assert removed("face") == [[[0], [], []]] * 3                        # a whole face: its function goes for every component
    assert removed("component") == [[[], [], []], [[], [3], []], [[], [], []]]   # one component of the face axis 1 / side 1
    assert removed("partial") == [[[], [], []]] * 3                      # a partial set of a face removes nothing
    assert removed("none") == [[[], [], []]] * 3
    for kind in ("face", "component", "partial", "none"):
        assert [[np.nonzero(~k)[0].tolist() for k in kk] for kk in ref.kept_functions(P, kc.essential(P, kind), 3)] == removed(kind)
    both = np.concatenate([kc.essential(P, "face"), kc.essential(P, "component")])
    assert removed("face")[1] == [[0], [], []] and \
        [np.nonzero(~k)[0].tolist() for k in KroneckerOperator(B, both, 3).kept[1]] == [[0], [3], []]


@functools.lru_cache(maxsize=None)
def _applied(name, kind):
    """(operator, z of the numpy application, its deviation from the extended-precision inverse)"""
    from mimi_amd.kronecker import KroneckerOperator
    P, B = kc.grid(name)
    r, z_ref = kc.application(name, kind)
    op = KroneckerOperator(B, kc.essential(P, kind), P.dim)
    z = op.apply(r, kc.RHO, kc.stiff(P.dim, kc.APPLY_FAC0, kc.APPLY_DAMPING))
    return op, z, float(np.abs(z - z_ref).max() / np.abs(z_ref).max())


@pytest.mark.parametrize("kind", kc.DIRICHLET)
@pytest.mark.parametrize("name", list(kc.GRIDS))
def test_numpy_application_equals_the_extended_precision_inverse(name, kind):
    """the bar of the device test, held by the numpy application too; the flattened U and lam are what the device gets"""
    P, B = kc.grid(name)
    op, z, dev = _applied(name, kind)
    ess, (r, _) = kc.essential(P, kind), kc.application(name, kind)
    assert op.n_dir == kc.NODES[name] and op.U.size == P.dim * sum(n * n for n in op.n_dir) and op.lam.size == P.dim * sum(op.n_dir)
    print(f"\n{name} [{kind}]: the numpy application deviates {dev:.3g} (DEV_APPLY {kc.DEV_APPLY:.3g})")
    assert dev <= kc.BAR * kc.DEV_APPLY
    assert np.array_equal(z[ess], r[ess])


def test_recorded_deviation_of_the_application():
    """DEV_APPLY of _kronecker_cases.py is what the numpy application shows here, to the variation between numpy builds"""
    measured = {(name, kind): _applied(name, kind)[2] for name in kc.GRIDS for kind in kc.DIRICHLET}
    worst = max(measured, key=measured.get)
    print(f"\nmeasured DEV_APPLY = {measured[worst]:.3g} {worst}")
    assert kc.DEV_APPLY / 5 <= measured[worst] <= 5 * kc.DEV_APPLY


@pytest.mark.parametrize("fac0", kc.FAC0)
@pytest.mark.parametrize("name", list(kc.SOLVES))
def test_restated_solves(name, fac0):
    """DEV_SOLVE, the margins and the recorded iteration counts (the Jacobi count, with a dozen restarts behind it, to a few
    per cent: it is recorded for the reader); the preconditioned solve with the product's own numpy application takes the
    iterations of the dense one"""
    from mimi_amd.kronecker import KroneckerOperator
    S = kc.oracle_system(name, fac0)
    jacobi, kron = kc.restated_solves(S.J, S.P, S.ess, S.b, fac0)
    x_ref = np.array([float(v) for v in ref.solve_extended(S.J, S.b)])
    dev = np.abs(kron.x - x_ref).max() / np.abs(x_ref).max()
    print(f"\n{name} fac0 {fac0:g}: iterations Jacobi {jacobi.iterations} -> Kronecker {kron.iterations}, margin "
          f"{ref.margin(kron):.3g}, x deviates {dev:.3g} (DEV_SOLVE {kc.DEV_SOLVE:.3g})")
    assert jacobi.converged and kron.converged
    assert kron.iterations == kc.ITERATIONS[(name, fac0)][1]
    assert abs(jacobi.iterations - kc.ITERATIONS[(name, fac0)][0]) <= 0.05 * kc.ITERATIONS[(name, fac0)][0]
    assert kron.iterations < jacobi.iterations
    assert ref.margin(kron) >= kc.MARGIN
    assert kc.DEV_SOLVE / 50 <= dev <= kc.BAR * kc.DEV_SOLVE
    op = KroneckerOperator(kc.solve_patch(name)[1], S.ess, S.P.dim)
    own = ref.gmres(S.J, S.b, lambda v: op.apply(v, kc.RHO, kc.stiff(S.P.dim, fac0)), max_iter=3000)
    assert own.iterations == kron.iterations and np.abs(own.x - x_ref).max() <= kc.BAR * kc.DEV_SOLVE * np.abs(x_ref).max()


def test_cg_restatement_on_an_affine_mass_matrix():
    """P at fac0 = 0 is the mass matrix of an affine block: preconditioned conjugate gradients end at once"""
    from mimi_amd.kronecker import KroneckerOperator
    from oracle import harness as hz
    P, B = kc.grid("p2_5x4x3")
    ess = kc.essential(P, "face")
    rowptr, col = P.sparsity()
    vals = hz.assemble_mass(P, P.tables(), kc.RHO, rowptr, col)
    hz.eliminate_row_col(rowptr, col, vals, ess)
    M = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs))
    b = np.random.default_rng(5).standard_normal(P.n_vdofs)
    b[ess] = 0.0
    op = KroneckerOperator(B, ess, P.dim)
    s = ref.cg(M, b, lambda v: op.apply(v, kc.RHO, np.zeros(9)))
    assert s.converged and s.iterations <= 2
    assert np.abs(M @ s.x - b).max() <= 1e-8 * np.abs(b).max()


def test_linear_solver_preconditioner_names():
    """the attribute and its boolean alias, without a handle"""
    from mimi_amd.linear import LinearSolver
    S = LinearSolver.__new__(LinearSolver)
    assert S.preconditioner == "jacobi" and S.use_jacobi and S._preconditioner_id() == 1
    S.use_jacobi = False
    assert S.preconditioner == "none" and S._preconditioner_id() == 0
    S.preconditioner = "kronecker"
    assert not S.use_jacobi and S._preconditioner_id() == 2
    S.preconditioner = "ilu"
    with pytest.raises(ValueError, match="ilu"):
        S._preconditioner_id()


def test_flag_is_refused_with_a_periodic_pair():
    """before any device work, like the other refusals of the periodic route: the test needs no GPU.  (Without the iterative
    solver the flag is inert and nothing is refused.)"""
    import mimi_amd as mimi
    from test_nonlinear_solid import beam
    nl = beam("neohook", runtime=[("use_iterative_solver", 1), ("use_kronecker_preconditioner", 1)], finish=False)
    faces = {f: a for a, f in nl._faces.items()}
    bc = mimi.BoundaryConditions()
    bc.initial.periodic(faces[(1, 0)], faces[(1, 1)])
    nl.boundary_condition = bc
    with pytest.raises(RuntimeError) as err:
        nl.setup(1)
    assert "use_kronecker_preconditioner" in str(err.value) and "periodic" in str(err.value)
