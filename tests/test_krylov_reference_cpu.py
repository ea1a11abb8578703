"""The 120-digit minimal-residual / Galerkin reference (tests/_krylov_reference.py) against facts that need no solver,
the condition that makes the iteration counts of the case table (tests/_krylov_cases.py) a property of the problems, and
the fp64 restatement oracle/krylov.py held to the reference on every case: equal iteration counts and `converged`, x and
the final norm within 20 times the deviations measured here and recorded in _krylov_cases.py (DEV_X = 2.5e-15 of max|x|,
DEV_NORM = 4.8e-8 of the goal; `pytest -s` prints what this run measures)."""
import numpy as np
import pytest
import scipy.sparse as sp
from mpmath import mp, mpf

import _krylov_cases as kc
import _krylov_reference as ref

GMRES_CASES = [name for name, case in kc.CASES.items() if case[0] == "gmres"]
CG_CASES = [name for name, case in kc.CASES.items() if case[0] == "cg"]


def _plain(A):
    return A.indptr.tolist(), A.indices.tolist(), A.data.tolist()


@pytest.mark.parametrize("jacobi", [True, False])
@pytest.mark.parametrize("n,density,seed", [(12, 0.4, 3), (23, 0.3, 4)])
def test_reference_gmres_reaches_the_direct_solve_after_n_steps(n, density, seed, jacobi):
    """K_n is the whole space: with kdim >= n and a tolerance out of reach the n-th iterate is A^-1 b; sparse and
    dense input give the same; the residuals of the cycle do not increase"""
    A, b = kc.random_system(n, density, 1.5, seed)
    exact = ref.solve_direct(_plain(A), b.tolist())
    for matrix in (_plain(A), A.toarray().tolist()):
        s = ref.gmres(matrix, b.tolist(), rel_tol=1e-200, abs_tol=0.0, max_iter=n, kdim=n + 3, jacobi=jacobi)
        assert s.iterations == n and not s.converged and len(s.history) == n + 1
        with mp.workdps(ref.DPS):
            scale = max(abs(v) for v in exact)
            assert max(abs(a - e) for a, e in zip(s.x, exact)) <= mpf(10) ** -80 * scale
            assert all(later <= earlier for earlier, later in zip(s.history, s.history[1:]))


@pytest.mark.parametrize("name", GMRES_CASES)
def test_reference_gmres_residuals_do_not_increase_within_a_cycle(name):
    s, _ = kc.reference(name)
    kdim = kc.settings(name)["kdim"]
    steps = s.history[1:]
    with mp.workdps(ref.DPS):
        for start in range(0, len(steps), kdim):
            cycle = ([s.history[0]] if start == 0 else [s.restarts[start // kdim - 1]]) + steps[start:start + kdim]
            assert all(later <= earlier * (1 + mpf(10) ** -90) for earlier, later in zip(cycle, cycle[1:]))
        # a restart residual is the last minimum of its cycle
        for c, restart in enumerate(s.restarts):
            last = steps[min((c + 1) * kdim, len(steps)) - 1]
            assert abs(restart - last) <= mpf(10) ** -80 * s.history[0]


@pytest.mark.parametrize("name", ["spd33_cg", "spd36_cg", "spd35_cg_plain", "nodes12x3_cg"])
def test_reference_cg_error_decreases_in_the_energy_norm(name):
    A, b = kc.system(name)
    s, _ = kc.reference(name)
    exact = ref.solve_direct(_plain(A), b.tolist())
    op = ref._Matrix(_plain(A), len(b))
    with mp.workdps(ref.DPS):
        errors = []
        for x in s.iterates:
            e = [a - t for a, t in zip(x, exact)]
            errors.append(mp.fdot(e, op.mult(e)))
        assert len(errors) == s.iterations + 1
        assert all(later < earlier for earlier, later in zip(errors, errors[1:]))


def test_reference_on_a_diagonal_matrix_takes_one_iteration():
    rng = np.random.default_rng(8)
    d, b = 0.5 + rng.random(9), rng.standard_normal(9)
    A = sp.diags(d).tocsr()
    for method in (ref.gmres, ref.cg):
        s = method(_plain(A), b.tolist(), jacobi=True)
        assert s.iterations == 1 and s.converged
        with mp.workdps(ref.DPS):
            assert max(abs(x - mpf(float(bi)) / mpf(float(di))) for x, bi, di in zip(s.x, b, d)) <= mpf(10) ** -100


def test_case_table_covers_what_it_has_to():
    its = {name: kc.reference(name)[0] for name in kc.CASES}
    st = {name: kc.settings(name) for name in kc.CASES}
    gm = GMRES_CASES
    assert {st[n]["kdim"] for n in gm} >= {1, 5, 7, 50}
    assert {True, False} == {st[n]["jacobi"] for n in gm}
    assert any(its[n].converged and its[n].iterations >= 20 * st[n]["kdim"] for n in gm)               # >= 20 cycles
    assert any(not its[n].converged and its[n].iterations == 300 for n in gm)                         # stagnation
    assert any(not its[n].converged and 0 < its[n].iterations % st[n]["kdim"] for n in gm)            # cut mid-cycle
    assert any(st[n]["max_iter"] == 0 and its[n].iterations == 0 and not its[n].converged for n in gm)
    assert {kc.system(n)[0].shape[0] for n in gm if st[n]["kdim"] == 50} >= {1, 3, 6, 7}
    assert any(its[n].iterations == 0 and its[n].converged and not kc.system(n)[1].any() for n in gm)
    assert any(its[n].iterations == 0 and its[n].converged and kc.system(n)[1].any() for n in gm)
    assert {kc.CASES[n][3] for n in gm} == {(3, True), (3, False), (2, False), (1, False)}
    assert all(kc.system(n)[0].shape[0] <= 60 for n in kc.CASES)
    assert any(its[n].indefinite and its[n].iterations >= 1 for n in CG_CASES)
    assert any(not its[n].converged and not its[n].indefinite for n in CG_CASES)


@pytest.mark.parametrize("name", list(kc.CASES))
def test_no_residual_of_a_case_sits_on_the_goal(name):
    """|residual_k / goal - 1| >= 1e-3 at every step of the reference: the iteration count belongs to the problem, not to
    the rounding of whoever solves it.  (A case that fails this is replaced.)"""
    s, _ = kc.reference(name)
    assert ref.margin(s) >= 1e-3


def _row_group(A):
    """what mimi_hip_linear_create finds: (rows sharing a column list, the list is made of node triples)"""
    n = A.shape[0]
    lists = [tuple(A.indices[A.indptr[i]:A.indptr[i + 1]]) for i in range(n)]
    for g in (3, 2):
        if n % g == 0 and all(lists[i] == lists[i - i % g] for i in range(n)):
            triples = g == 3 and all(len(c) % 3 == 0 and all(c[k] % 3 == 0 and c[k + 1] == c[k] + 1 and c[k + 2] == c[k] + 2
                                                             for k in range(0, len(c), 3)) for c in lists)
            return g, triples
    return 1, False


@pytest.mark.parametrize("name", list(kc.CASES))
def test_case_patterns_have_the_row_grouping_they_claim(name):
    assert _row_group(kc.system(name)[0]) == kc.CASES[name][3]


_measured = {}


@pytest.mark.parametrize("name", list(kc.CASES))
def test_restatement_equals_reference(name):
    from oracle import krylov
    A, b = kc.system(name)
    s, _ = kc.reference(name)
    with np.errstate(invalid="ignore"):      # (n = 1: the unused v_1 of the restatement is 0 / 0)
        x, it, nrm, conv = getattr(krylov, kc.CASES[name][0])(A, b.copy(), **kc.settings(name))
    dx, dn = kc.deviations(name, x, nrm)
    _measured[name] = (dx, dn)
    print(f"\n{name}: iterations {it} (reference {s.iterations}), x deviates {dx:.3g}, final norm {dn:.3g} of the goal")
    assert it == s.iterations and bool(conv) == s.converged
    assert np.isfinite(x).all()
    assert dx <= kc.BAR * kc.DEV_X
    assert dn <= kc.BAR * kc.DEV_NORM


def test_recorded_deviations_are_the_measured_ones():
    """DEV_X and DEV_NORM of _krylov_cases.py are what the restatement shows here, to the variation between numpy builds"""
    from oracle import krylov
    for name in kc.CASES:
        if name not in _measured:
            A, b = kc.system(name)
            with np.errstate(invalid="ignore"):
                x, it, nrm, conv = getattr(krylov, kc.CASES[name][0])(A, b.copy(), **kc.settings(name))
            _measured[name] = kc.deviations(name, x, nrm)
    worst_x = max(_measured, key=lambda n: _measured[n][0])
    worst_n = max(_measured, key=lambda n: _measured[n][1])
    print(f"\nmeasured DEV_X = {_measured[worst_x][0]:.3g} ({worst_x}), DEV_NORM = {_measured[worst_n][1]:.3g} ({worst_n})")
    assert kc.DEV_X / 5 <= _measured[worst_x][0] <= 5 * kc.DEV_X
    assert kc.DEV_NORM / 5 <= _measured[worst_n][1] <= 5 * kc.DEV_NORM


@pytest.mark.parametrize("name", ["ns33_k5", "spd33_cg"])
def test_replicated_system_solves_like_one_copy(name):
    """A = I_m (x) A0, b = c (x) b0: the iterations of (A0, b0), x = c (x) x0, norm = ||c|| norm0 -- what the large-vector
    tests of the device solver rest on, asserted here on the restatement at m = 400"""
    from oracle import krylov
    m = 400
    rowptr, col, val, b, c = kc.replicated(name, m)
    n = len(b)
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    A0, b0 = kc.system(name)
    assert (A != sp.kron(sp.eye(m), A0, format="csr")).nnz == 0 and np.array_equal(b, np.kron(c, b0))
    assert np.abs(c).min() >= 0.5 and np.abs(c).max() <= 2.0 and (c > 0).any() and (c < 0).any()
    s, x64 = kc.reference(name)
    x, it, nrm, conv = getattr(krylov, kc.CASES[name][0])(A, b.copy(), **kc.settings(name))
    norm_c = np.linalg.norm(c)
    dx = np.abs(x - np.kron(c, x64)).max() / np.abs(np.kron(c, x64)).max()
    dn = abs(nrm - norm_c * float(s.final_norm)) / (norm_c * float(s.goal))
    print(f"\n{name} x {m}: iterations {it} (one copy: {s.iterations}), x deviates {dx:.3g}, final norm {dn:.3g} of the goal")
    assert it == s.iterations and bool(conv) == s.converged
    assert dx <= kc.BAR * kc.DEV_X and dn <= kc.BAR * kc.DEV_NORM
