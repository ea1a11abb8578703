"""csrc/krylov.hip through mimi_amd.linear.LinearSolver against the 120-digit minimal-residual / Galerkin reference
(tests/_krylov_reference.py) on the case table of tests/_krylov_cases.py: equal iteration counts and `converged_`, x and
`final_norm_` within 20 times the deviation an fp64 solve of these systems shows on the CPU (DEV_X, DEV_NORM: measured
by test_krylov_reference_cpu.py on oracle/krylov.py, never on the device).  Then what the table cannot reach: x being
overwritten, one handle reused across kdim and methods, vectors long enough for every trip of kr_mgs_kernel (replicated
systems: test_krylov_reference_cpu.py::test_replicated_system_solves_like_one_copy), rows long enough for the second
and later trips of kr_row_products in all four product forms, and the essential-dof list given unsorted."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import _krylov_cases as kc

pytestmark = pytest.mark.gpu


def _solver(A, where, essential=None):
    """(LinearSolver, to_device) for the pattern of A; where == "device": the pattern and every vector are torch tensors"""
    from mimi_amd.integrators import CSRPattern
    from mimi_amd.linear import LinearSolver
    rowptr, col = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    if where == "host":
        return LinearSolver(CSRPattern(rowptr, col, len(col)), essential), lambda a: np.array(a, dtype=np.float64)
    import torch
    dev = torch.device("cuda", 0)
    S = LinearSolver(CSRPattern(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), len(col)), essential)
    return S, lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _run(S, method, st, val, b, x):
    """the solve of the settings `st`; (x on the host, iterations, final norm, converged)"""
    S.use_jacobi = st["jacobi"]
    if method == "gmres":
        S.rel_tol, S.abs_tol, S.max_iter, S.kdim = st["rel_tol"], st["abs_tol"], st["max_iter"], st["kdim"]
        S.Mult(val, b, x)
    else:
        S.MultCG(val, b, x, rel_tol=st["rel_tol"], abs_tol=st["abs_tol"], max_iter=st["max_iter"])
    return _host(x).copy(), S.final_iter_, S.final_norm_, S.converged_


def _solve_case(name, where, fill=0.0, S=None, **changed):
    A, b = kc.system(name)
    to = None
    if S is None:
        S, to = _solver(A, where)
    else:
        S, to = S
    return _run(S, kc.CASES[name][0], {**kc.settings(name), **changed}, to(A.data), to(b), to(np.full(len(b), fill)))


def _stopping_norm(name, x):
    """||M (b - A x)|| (GMRES) or sqrt|(r, M r)| (CG) of a returned x, in long double"""
    A, b = kc.system(name)
    L = np.longdouble
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    Ax = np.zeros(A.shape[0], dtype=L)
    np.add.at(Ax, rows, A.data.astype(L) * x.astype(L)[A.indices])
    r = b.astype(L) - Ax
    m = 1 / A.diagonal().astype(L) if kc.settings(name)["jacobi"] else np.ones(len(b), dtype=L)
    if kc.CASES[name][0] == "gmres":
        return np.sqrt(np.sum((m * r) ** 2))
    return np.sqrt(np.abs(np.sum(m * r * r)))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", list(kc.CASES))
def test_device_solver_equals_reference(name, where):
    A, b = kc.system(name)
    S, to = _solver(A, where)
    assert (S.RowGroup(), S.NodeColumns()) == kc.CASES[name][3]
    x, it, nrm, conv = _solve_case(name, where, S=(S, to))
    s, x64 = kc.reference(name)
    dx, dn = kc.deviations(name, x, nrm)
    print(f"\n{name} [{where}]: iterations {it} (reference {s.iterations}), x deviates {dx:.3g} (bar {kc.BAR * kc.DEV_X:.3g}), "
          f"final norm {dn:.3g} of the goal (bar {kc.BAR * kc.DEV_NORM:.3g})")
    assert np.isfinite(x).all() and np.isfinite(nrm)
    assert it == s.iterations and conv == s.converged
    assert dx <= kc.BAR * kc.DEV_X
    assert dn <= kc.BAR * kc.DEV_NORM
    if not s.converged:
        # what was returned as the norm is the norm of what was returned as x
        assert abs(np.longdouble(nrm) - _stopping_norm(name, x)) <= kc.BAR * kc.DEV_NORM * float(s.goal)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["ns36_k5", "ns36_k5_cut7", "ns36_maxiter0", "b_zero", "b_below_abs_tol", "n1", "spd36_cg",
                                  "cg_b_zero", "cg_indefinite"])
def test_x_is_overwritten(name, where):
    """iterative_mode false: what x holds on entry is not read"""
    zeros = _solve_case(name, where, fill=0.0)
    nans = _solve_case(name, where, fill=np.nan)
    assert nans[0].tobytes() == zeros[0].tobytes() and nans[1:] == zeros[1:]
    if not kc.system(name)[1].any():
        assert not nans[0].any() and not np.signbit(nans[0]).any()
        assert nans[1:] == (0, 0.0, True)


@pytest.mark.parametrize("where", ["host", "device"])
def test_one_handle_reused_across_kdim_and_methods(where):
    """V, the partial sums and the pinned Hessenberg columns grow with kdim, and CG takes V as d, z, q: every solve of the
    sequence gives the bytes of a fresh handle -- also when the matrix values change between solves and the preconditioner id
    alternates 1, 0, 1 (the Jacobi scaling belongs to one solve)"""
    name = "spd36_cg"                  # symmetric positive definite: GMRES and CG both solve it
    A, b = kc.system(name)
    sequence = [("gmres", dict(kdim=7)), ("gmres", dict(kdim=50)), ("gmres", dict(kdim=1)), ("cg", dict()), ("gmres", dict(kdim=50))]
    shared = _solver(A, where)
    for method, changed in sequence:
        st = {**(kc.GMRES_DEFAULTS if method == "gmres" else kc.CG_DEFAULTS), **changed}
        got = []
        for S, to in (shared, _solver(A, where)):
            got.append(_run(S, method, st, to(A.data), to(b), to(np.full(len(b), np.nan))))
        assert got[0][2] > 0 and got[0][3]
        assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1:] == got[1][1:]
    # the matrix values change between solves (rows scaled, so the diagonal moves) and the preconditioner id alternates:
    # nothing of one solve's Jacobi scaling may reach the next
    rng = np.random.default_rng(71)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    val = A.data.copy()
    for jacobi in (True, False, True):
        val = val * rng.uniform(0.5, 2.0, A.shape[0])[rows]
        for method in ("gmres", "cg"):
            # (rows scaled: no longer symmetric, so conjugate gradients get a short leash; their bytes are compared all the same)
            st = {**(kc.GMRES_DEFAULTS if method == "gmres" else {**kc.CG_DEFAULTS, "max_iter": 60}), "jacobi": jacobi}
            got = []
            for S, to in (shared, _solver(A, where)):
                x, it, nrm, conv = _run(S, method, st, to(val), to(b), to(np.full(len(b), np.nan)))
                got.append((x.tobytes(), it, np.float64(nrm).tobytes(), conv))
            assert got[0] == got[1]
            assert method == "cg" or (got[0][1] > 1 and got[0][3])


@pytest.mark.parametrize("copies", [3972, 31776])
@pytest.mark.parametrize("name", ["ns33_k5", "spd33_cg"])
def test_large_vectors(name, copies):
    """n = 33 * 3972 = 131 076 = 512 * 256 + 4: four threads of kr_mgs_kernel have an entry at their second position;
    n = 33 * 31 776 = 1 048 608 = 8 * 512 * 256 + 32: part of one wave makes the second trip of its loop.  The system is
    `copies` scaled copies of a case of the table, so the reference is that of the one copy."""
    from mimi_amd.integrators import CSRPattern
    from mimi_amd.linear import LinearSolver
    rowptr, col, val, b, c = kc.replicated(name, copies)
    n = len(b)
    assert n in (512 * 256 + 4, 8 * 512 * 256 + 32)
    st = kc.settings(name)
    assert st["abs_tol"] == 0.0
    S = LinearSolver(CSRPattern(rowptr, col, len(col)))
    assert S.RowGroup() == 1
    x, it, nrm, conv = _run(S, kc.CASES[name][0], st, val, b, np.full(n, np.nan))
    s, x64 = kc.reference(name)
    expected = np.kron(c, x64)
    norm_c = np.sqrt(np.sum(c.astype(np.longdouble) ** 2))
    dx = np.abs(x - expected).max() / np.abs(expected).max()
    dn = float(abs(nrm - norm_c * np.longdouble(float(s.final_norm))) / (norm_c * float(s.goal)))
    print(f"\n{name} x {copies}: iterations {it} (one copy: {s.iterations}), x deviates {dx:.3g}, final norm {dn:.3g} of the goal")
    assert np.isfinite(x).all()
    assert it == s.iterations and conv == s.converged
    assert dx <= kc.BAR * kc.DEV_X
    assert dn <= kc.BAR * kc.DEV_NORM


def _grid_pattern(dims, vdim, radius, drop_middle=False):
    """a vdim-vector field on a node grid, every node coupled to the nodes within `radius` in the maximum norm, byVDIM
    numbering (drop_middle: without the middle dof of the other nodes)"""
    nodes = np.arange(int(np.prod(dims))).reshape(dims)
    rows = []
    for idx in itertools.product(*[range(d) for d in dims]):
        sl = tuple(slice(max(i - radius, 0), min(i + radius + 1, d)) for i, d in zip(idx, dims))
        nb = np.sort(nodes[sl].ravel())
        cols = (nb[:, None] * vdim + np.arange(vdim)[None, :]).ravel()
        if drop_middle:
            cols = cols[(cols % vdim != 1) | (cols // vdim == nodes[idx])]
        rows.extend([cols] * vdim)
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32)


def _long_row_pattern(kind):
    """(rowptr, col, RowGroup, NodeColumns, longest row)"""
    if kind == "3d_radius2":
        return _grid_pattern((7, 7, 7), 3, 2) + (3, True, 375)
    if kind == "3d_radius3":
        return _grid_pattern((7, 7, 7), 3, 3) + (3, True, 1029)
    if kind == "3d_radius2_dropped":
        return _grid_pattern((7, 7, 7), 3, 2, drop_middle=True) + (3, False, 251)
    if kind == "3d_radius3_dropped":
        return _grid_pattern((7, 7, 7), 3, 3, drop_middle=True) + (3, False, 687)
    if kind == "2d_radius6":
        return _grid_pattern((15, 14), 2, 6) + (2, False, 338)
    A = sp.random(601, 601, density=0.6, random_state=5, format="csr") + sp.eye(601, format="csr")
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), 1, False, int(np.diff(A.indptr).max())


@pytest.mark.parametrize("alpha", [1.0, -0.75])
@pytest.mark.parametrize("kind", ["3d_radius2", "3d_radius3", "3d_radius2_dropped", "3d_radius3_dropped", "2d_radius6", "ragged"])
def test_add_mult_on_long_rows(kind, alpha):
    """a lane of kr_row_products takes 4 entries per trip: rows of more than 256 entries (degree 2: 375, degree 3: 1029)
    make the later trips, the rows at the boundary of the grid the mixed tails.  Against the row sums in long double; a
    row may miss them by the rounding of its own len + 4 operations, (len + 4) 2^-53 (|y0| + |alpha| sum |a_k x_k|)."""
    from mimi_amd.integrators import CSRPattern
    from mimi_amd.linear import LinearSolver
    rowptr, col, group, triples, longest = _long_row_pattern(kind)
    n, lens = len(rowptr) - 1, np.diff(rowptr)
    assert lens.max() == longest and lens.min() < longest
    rng = np.random.default_rng(29)
    val, x, y0 = rng.standard_normal(len(col)), rng.standard_normal(n), rng.standard_normal(n)
    S = LinearSolver(CSRPattern(rowptr, col, len(col)))
    assert S.RowGroup() == group and S.NodeColumns() == triples
    y = S.AddMult(val, x, y0.copy(), alpha=alpha)
    L = np.longdouble
    products = val.astype(L) * x.astype(L)[col]
    sums = np.add.reduceat(products, rowptr[:-1])
    magnitudes = np.add.reduceat(np.abs(products), rowptr[:-1])
    expected = y0.astype(L) + L(alpha) * sums
    bar = (lens + 4) * L(2.0) ** -53 * (np.abs(y0) + abs(alpha) * magnitudes)
    excess = np.abs(y.astype(L) - expected) / bar
    print(f"\n{kind}: rows of {lens.min()} .. {lens.max()} entries, worst |y - y_ref| / bar = {float(excess.max()):.3g}")
    assert (excess <= 1).all()


@pytest.mark.parametrize("where", ["host", "device"])
def test_cg_exits(where):
    """max_iter below what the solve needs, and a matrix that is not positive definite ((d, A d) <= 0): not converged,
    the reference's iteration and iterate, finite values"""
    for name in ("spd36_cg_cut4", "cg_indefinite"):
        s, x64 = kc.reference(name)
        assert not s.converged and s.indefinite == (name == "cg_indefinite") and s.iterations >= 1
        x, it, nrm, conv = _solve_case(name, where, fill=np.nan)
        assert np.isfinite(x).all() and np.isfinite(nrm)
        assert (it, conv) == (s.iterations, False)
        dx, dn = kc.deviations(name, x, nrm)
        assert dx <= kc.BAR * kc.DEV_X and dn <= kc.BAR * kc.DEV_NORM
    # the same matrix without the cut converges
    x, it, nrm, conv = _solve_case("spd36_cg_cut4", where, max_iter=1000)
    assert conv and it == kc.reference("spd36_cg")[0].iterations


@pytest.mark.parametrize("where", ["host", "device"])
def test_eliminate_with_an_unsorted_list_with_duplicates(where):
    A, b = kc.system("nodes12x3")
    rng = np.random.default_rng(61)
    unique = np.sort(rng.choice(A.shape[0], 11, replace=False)).astype(np.int64)
    shuffled = rng.permutation(np.concatenate([unique, unique[::3], unique[:2]])).astype(np.int64)
    assert len(shuffled) > len(unique) and not np.array_equal(np.sort(shuffled), shuffled)
    results = []
    for ess in (unique, shuffled):
        S, to = _solver(A, where, ess)
        r, vals = to(b), to(A.data)
        S.Eliminate(r, vals)
        results.append((_host(r).copy(), _host(vals).copy()))
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
    # and it is the elimination: rows and columns of the list are gone, their diagonal is one
    mask = np.zeros(A.shape[0], dtype=bool)
    mask[unique] = True
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    kill = mask[rows] | mask[A.indices]
    expected = np.where(kill, np.where(rows == A.indices, 1.0, 0.0), A.data)
    assert np.array_equal(results[0][1], expected) and np.array_equal(results[0][0], np.where(mask, 0.0, b))
