"""mimi_amd/kronecker.py with periodic axes against the references of tests/_kronecker_reference.py folded by
the dense maps of tests/_periodic_solver_cases.py, without a device; measures the constants of that file.

(1) the folded 1-D matrices P1^T M P1, P1^T K P1, their kernel, their mass and the orthonormality of the eigenvectors;
(2) the dense folded operator is the Kronecker product of the folded 1-D matrices, and KroneckerOperator.apply is its 50-digit
    inverse within kc.BAR x DEV_APPLY_PERIODIC;
(3) periodic_axes=() gives the arrays of the class without the argument, byte for byte;
(4) the restated solves on the folded oracle tangents: iteration counts, margins, DEV_SOLVE_PERIODIC; CG on a folded mass;
(5) the rules of the "periodic_iterative" flag, before any device work."""
import functools
import os

import numpy as np
import pytest

import _kronecker_cases as kc
import _kronecker_reference as ref
import _periodic_solver_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -53


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, spans, repeated", pc.AXES_1D)
def test_folded_1d_matrices(p, spans, repeated):
    from mimi_amd.kronecker import KroneckerOperator
    kn, B = pc.patch_1d(p, spans, repeated)
    n = len(kn) - p - 1
    op = KroneckerOperator(B, [], 2, periodic_axes=(0,))
    assert op.n_dir == [n - 1, 2] and op.periodic_axes == [0]
    L = op.lengths[0]
    assert abs(L - pc.LENGTH_1D) <= 4 * n * ULP * pc.LENGTH_1D         # the whole unwrapped polygon: the period
    M, K = ref.matrices_1d(kn, p)
    P1 = pc.p1(n)
    Mf, Kf = P1.T @ (L * M) @ P1, P1.T @ (K / L) @ P1
    assert op.M[0].shape == (n - 1, n - 1) and op.K[0].shape == (n - 1, n - 1)
    assert np.abs(op.M[0] - Mf).max() <= 1e-14 * np.abs(Mf).max()
    assert np.abs(op.K[0] - Kf).max() <= 1e-14 * np.abs(Kf).max()
    if spans == 1 and p == 2:
        assert n - 1 == 2 and (op.M[0] > 0).all()                        # every function overlaps every other
    # the constant is in the kernel of K and carries the whole mass: to rounding (sums of at most n entries, each a sum of
    # (p + 1) Gauss terms)
    ones = np.ones(n - 1)
    assert np.abs(op.K[0] @ ones).max() <= 16 * n * (p + 1) * ULP * np.abs(op.K[0]).max()
    assert abs(ones @ op.M[0] @ ones - L) <= 16 * n * (p + 1) * ULP * L
    # no face on the periodic axis; the eigenvectors are M-orthonormal within test_kronecker_cpu.py's bar
    for c in range(2):
        U, lam, keep = op.U_cd[c][0], op.lam_cd[c][0], op.kept[c][0]
        assert keep.all() and len(keep) == n - 1 and (lam >= 0.0).all()
        assert np.abs(U.T @ op.M[0] @ U - np.eye(n - 1)).max() <= 1e-12
        assert np.abs(U.T @ op.K[0] @ U - np.diag(lam)).max() <= 1e-12 * max(lam.max(), 1.0)
        assert lam.min() <= 1e-12 * max(lam.max(), 1.0)                  # the constant's eigenvalue


def test_the_node_map_of_the_cases_is_the_products():
    from mimi_amd.integrators import periodic_node_map
    for n, axes in (([4, 3, 5], (1,)), ([3, 4, 3], (0, 2)), ([5, 4], (0,)), ([3, 3, 3], (0, 1, 2))):
        assert np.array_equal(pc.node_map(n, axes), periodic_node_map(n, axes))


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.GRIDS))
def test_dense_folded_operator_is_the_kronecker_product_of_the_folded_matrices(name):
    """entries are sums of at most 2^(periodic axes) x (1 + dim) products of dim factors, each factor off by a few ulp of the
    two independent Gauss loops (1e-14 relative, test (1)): 1e-13 x the largest entry covers them"""
    from mimi_amd.kronecker import KroneckerOperator
    P, B, axes, ess, n_dir = pc.grid(name)
    dim = P.dim
    op = KroneckerOperator(B, ess, dim, periodic_axes=axes)
    assert op.n_dir == n_dir and op.n == int(np.prod(n_dir)) * dim
    assert op.U.size == dim * sum(n * n for n in n_dir) and op.lam.size == dim * sum(n_dir)
    stiff = kc.stiff(dim, kc.APPLY_FAC0, kc.APPLY_DAMPING)
    for c in range(dim):
        dense = pc.folded_component_operator(P, axes, c, kc.RHO, stiff)
        kron = kc.RHO * ref._kron(op.M)
        for d in range(dim):
            kron = kron + stiff[c, d] * ref._kron([op.K[a] if a == d else op.M[a] for a in range(dim)])
        assert np.abs(kron - dense).max() <= 1e-13 * np.abs(dense).max()
    # the face rule through the node map: the clamped face's function goes for every component, nothing on a periodic axis
    face_axis, side = pc.GRIDS[name][4]
    for c in range(dim):
        for d in range(dim):
            gone = np.nonzero(~op.kept[c][d])[0].tolist()
            assert gone == ([0 if side == 0 else n_dir[d] - 1] if d == face_axis else [])


@functools.lru_cache(maxsize=None)
def _applied(name):
    from mimi_amd.kronecker import KroneckerOperator
    P, B, axes, ess, _ = pc.grid(name)
    r, z_ref = pc.application(name)
    op = KroneckerOperator(B, ess, P.dim, periodic_axes=axes)
    z = op.apply(r, kc.RHO, kc.stiff(P.dim, kc.APPLY_FAC0, kc.APPLY_DAMPING))
    return z, float(np.abs(z - z_ref).max() / np.abs(z_ref).max())


@pytest.mark.parametrize("name", list(pc.GRIDS))
def test_numpy_application_equals_the_extended_precision_inverse(name):
    _, _, _, ess, _ = pc.grid(name)
    r, _ = pc.application(name)
    z, dev = _applied(name)
    print(f"\n{name}: the numpy application deviates {dev:.3g} (DEV_APPLY_PERIODIC {pc.DEV_APPLY_PERIODIC:.3g})")
    assert dev <= kc.BAR * pc.DEV_APPLY_PERIODIC
    assert np.array_equal(z[ess], r[ess])


def test_recorded_deviation_of_the_application():
    measured = {name: _applied(name)[1] for name in pc.GRIDS}
    worst = max(measured, key=measured.get)
    print(f"\nmeasured DEV_APPLY_PERIODIC = {measured[worst]:.3g} ({worst})")
    assert pc.DEV_APPLY_PERIODIC / 5 <= measured[worst] <= 5 * pc.DEV_APPLY_PERIODIC


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, kind", [("p2_5x4x3", "face"), ("p3_10x6", "component"), ("rep3d_p2", "partial"), ("mix3d_322", "none")])
def test_without_periodic_axes_nothing_changes(name, kind):
    """the arrays of the class as it was before the argument existed, restated here from its definition: the same calls of
    scipy on the same matrices, so the same bytes"""
    import scipy.linalg
    from mimi_amd import kronecker
    from mimi_amd.kronecker import KroneckerOperator
    P, B = kc.grid(name)
    dim = P.dim
    ess = kc.essential(P, kind)
    op = KroneckerOperator(B, ess, dim, periodic_axes=())
    plain = KroneckerOperator(B, ess, dim)
    assert op.n_dir == kc.NODES[name] and op.n == P.n_nodes * dim and op.periodic_axes == []
    L = kronecker.axis_lengths(B)
    kept = ref.kept_functions(P, ess, dim)
    Us, lams = [], []
    for c in range(dim):
        for d in range(dim):
            M, K = kronecker.matrices_1d(B.knots[d], B.degrees[d])
            M, K = L[d] * M, K / L[d]
            keep = np.nonzero(kept[c][d])[0]
            n = P.n[d]
            U, lam = np.zeros((n, n)), np.full(n, -1.0)
            w, V = scipy.linalg.eigh(K[np.ix_(keep, keep)], M[np.ix_(keep, keep)])
            U[np.ix_(keep, np.arange(len(keep)))] = V
            lam[:len(keep)] = np.maximum(w, 0.0)
            Us.append(U.ravel())
            lams.append(lam)
    assert op.U.tobytes() == np.concatenate(Us).tobytes() == plain.U.tobytes()
    assert op.lam.tobytes() == np.concatenate(lams).tobytes() == plain.lam.tobytes()
    stiff = kc.stiff(dim, kc.APPLY_FAC0, kc.APPLY_DAMPING)
    assert op.scaling(kc.RHO, stiff).tobytes() == plain.scaling(kc.RHO, stiff).tobytes()
    r, _ = kc.application(name, kind)
    assert op.apply(r, kc.RHO, stiff).tobytes() == plain.apply(r, kc.RHO, stiff).tobytes()


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fac0", kc.FAC0)
@pytest.mark.parametrize("name, axis", pc.SOLVES)
def test_restated_solves(name, axis, fac0):
    from mimi_amd.kronecker import KroneckerOperator
    S = pc.folded_system(name, axis, fac0)
    dim = S.P.dim
    op = KroneckerOperator(S.B, S.ess, dim, periodic_axes=S.axes)
    assert op.n == len(S.b)
    dinv = 1.0 / S.J.diagonal()
    jacobi = ref.gmres(S.J, S.b, lambda v: dinv * v, max_iter=3000)
    kron = ref.gmres(S.J, S.b, lambda v: op.apply(v, kc.RHO, kc.stiff(dim, fac0)), max_iter=3000)
    x_ref = np.array([float(v) for v in ref.solve_extended(S.J, S.b)])
    dev = np.abs(kron.x - x_ref).max() / np.abs(x_ref).max()
    print(f"\n{name} axis {axis} fac0 {fac0:g}: iterations Jacobi {jacobi.iterations} -> Kronecker {kron.iterations}, margin "
          f"{ref.margin(kron):.3g}, x deviates {dev:.3g} (DEV_SOLVE_PERIODIC {pc.DEV_SOLVE_PERIODIC:.3g})")
    assert jacobi.converged and kron.converged
    want = pc.ITERATIONS[(name, axis, fac0)]
    assert kron.iterations == want[1]
    assert abs(jacobi.iterations - want[0]) <= 0.05 * want[0]
    assert kron.iterations < jacobi.iterations
    assert ref.margin(kron) >= kc.MARGIN
    assert dev <= kc.BAR * pc.DEV_SOLVE_PERIODIC


def test_restated_cg_on_the_folded_mass():
    from mimi_amd.kronecker import KroneckerOperator
    name, axis = pc.CG_CASE
    S = pc.folded_system(name, axis, kc.FAC0[0])
    op = KroneckerOperator(S.B, S.ess, S.P.dim, periodic_axes=S.axes)
    s = ref.cg(S.M, S.b, lambda v: op.apply(v, kc.RHO, np.zeros(S.P.dim ** 2)))
    print(f"\n{name} axis {axis}: CG iterations on the folded mass {s.iterations}, margin {ref.margin(s):.3g}")
    assert s.converged and s.iterations == pc.CG_ITERATIONS
    assert ref.margin(s) >= kc.MARGIN
    assert np.abs(S.M @ s.x - S.b).max() <= 1e-7 * np.abs(S.b).max()


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
MESH = os.path.join(ROOT, "tests", "golden", "meshes", "square-nurbs.mesh")
KRONECKER = (("use_iterative_solver", 1), ("use_kronecker_preconditioner", 1))
MATRIX_FREE = KRONECKER + (("matrix_free", 1),)
CONSISTENT = (("explicit_dynamics", 1), ("explicit_consistent_mass", 1))


def _prepared(flags, mark=None):
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(MESH)
    rc = mimi.RuntimeCommunication()
    for k, v in flags:
        rc.set_int(k, v)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.periodic(3, 4)
    if mark:
        mark(bc)
    nl.boundary_condition = bc
    return nl


@pytest.mark.parametrize("flags, match", [(KRONECKER, "the folded numbering needs periodic 1-D matrices"),
                                          (MATRIX_FREE, "the folded numbering needs periodic 1-D matrices"),
                                          (CONSISTENT, "explicit_consistent_mass cannot be combined with a periodic boundary")])
def test_without_the_flag_the_refusals_hold(flags, match):
    for extra in ((), (("periodic_iterative", 0),)):
        with pytest.raises(RuntimeError, match=match):
            _prepared(flags + extra).setup(1)


def test_matrix_free_refusal_without_the_flag_word_for_word(monkeypatch):
    """the matrix_free refusal stands behind the Kronecker one in setup(); reached alone here"""
    import mimi_amd.solid as solid
    nl = _prepared(MATRIX_FREE)
    seen = []
    real = nl.runtime_communication.get_int

    def get_int(key, default):
        # (the Kronecker refusal asks for this key first: answer 0 there once, so that the next refusal is reached)
        if key == "use_kronecker_preconditioner" and not seen:
            seen.append(key)
            return 0
        return real(key, default)
    monkeypatch.setattr(nl.runtime_communication, "get_int", get_int)
    with pytest.raises(RuntimeError) as err:
        nl.setup(1)
    assert str(err.value) == "matrix_free cannot be combined with a periodic boundary: the action runs in the unwrapped numbering"
    assert solid.NonlinearSolid is type(nl)


@pytest.mark.parametrize("flags", [KRONECKER, MATRIX_FREE + (("matrix_free_boundary", 1),)])
def test_with_the_flag_a_marker_on_a_joined_face_is_refused_as_ever(flags):
    # boundary 2 is attribute 3, which the pair (3, 4) makes interior
    with pytest.raises(RuntimeError, match=r"periodic boundary: pressure marker on boundary 2 \(attribute 3\), which the periodic pair makes interior"):
        _prepared(flags + (("periodic_iterative", 1),), lambda bc: bc.initial.pressure(2, 1.0)).setup(1)
