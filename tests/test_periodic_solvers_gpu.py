"""Periodic pairs on the Kronecker and matrix-free solver routes, on the device: the Kronecker application on the reduced grid,
the folded product of csrc/krylov.hip (LinearSolver.SetOperatorFold / OperatorMult), solves with both, and the facade's
"periodic_iterative" flag.  Inputs, references and measured constants: tests/_periodic_solver_cases.py.

(6)  the device application against the 50-digit inverse of the dense folded operator, within kc.BAR x DEV_APPLY_PERIODIC;
(7)  the folded product alone against mask(P^T (K v_u)) of the long-double reference, the mass and viscosity terms, a contact
     and a pressure term, and its bytes: those of PeriodicFold.Add of the unfolded action;
(8)  the rules of the seam;
(9)  GMRES and CG with the folded operator and the periodic Kronecker operator: the restatement's iteration counts;
(10) the facade: iterative + Kronecker, additionally matrix-free, against the periodic direct route;
(11) explicit_consistent_mass with a pair, against the folded restatement."""
import functools

import numpy as np
import pytest

import _domain_cases as dc
import _domain_reference as dr
import _explicit_cases as ec
import _face_reference as fr
import _kronecker_cases as kc
import _kronecker_reference as ref
import _periodic_solver_cases as pc
from _cases import product_material
from _domain_cases import DT, f64

pytestmark = pytest.mark.gpu


def _diagonal_pattern(n):
    from mimi_amd.integrators import CSRPattern
    return CSRPattern(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), n)


def _fold(pattern_u, n_ctrl, axes, dim):
    from mimi_amd.integrators import PeriodicFold
    return PeriodicFold(pattern_u, pc.node_map(n_ctrl, axes), dim).Prepare()


# ---- (6) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.GRIDS))
def test_device_application_on_the_reduced_grid(name):
    from mimi_amd.kronecker import KroneckerOperator
    from mimi_amd.linear import LinearSolver
    P, B, axes, ess, n_dir = pc.grid(name)
    r, z_ref = pc.application(name)
    S = LinearSolver(_diagonal_pattern(len(r)), ess)
    S.SetKronecker(KroneckerOperator(B, ess, P.dim, periodic_axes=axes))
    S.SetKroneckerCoefficients(kc.RHO, kc.stiff(P.dim, kc.APPLY_FAC0, kc.APPLY_DAMPING))
    z = S.ApplyPreconditioner("kronecker", None, np.array(r), np.full(len(r), np.nan))
    again = S.ApplyPreconditioner(2, None, np.array(r), np.full(len(r), np.nan))
    dev = np.abs(z - z_ref).max() / np.abs(z_ref).max()
    print(f"\n{name} {n_dir}: z deviates {dev:.3g} (bar {kc.BAR * pc.DEV_APPLY_PERIODIC:.3g})")
    assert np.isfinite(z).all()
    assert dev <= kc.BAR * pc.DEV_APPLY_PERIODIC
    assert np.array_equal(z[ess], r[ess])
    assert z.tobytes() == again.tobytes()


# ---- (7) ---------------------------------------------------------------------------------------------------------------------
# (case of tests/_domain_cases.py, periodic axis, clamped face on another axis): col8_p2 along its 8 spans and along an axis of
# 2 spans (4 nodes -> 3: the window wraps onto itself), col5_p3 along its single span (4 nodes -> 3), a 2-D case with repeated
# knots, a general-family case
PRODUCTS = [("col8_p2", 2, (0, 0)), ("col8_p2", 0, (1, 1)), ("col5_p3", 1, (0, 0)), ("rep2d_p3", 1, (0, 1)), ("mix3d_231", 0, (2, 0))]


@functools.lru_cache(maxsize=None)
def _product_inputs(case, axis, face):
    """(dof fold P as scipy, folded essential dofs, x_f, v_u = P mask(x_f)); shared, read-only"""
    a = dc.arrays(case)
    nm = pc.node_map(a.n_ctrl, (axis,))
    nodes = np.unique(nm[fr.face_node_ids(a.n_ctrl, *face)])
    ess = np.sort(np.concatenate([nodes * a.dim + c for c in range(a.dim)])).astype(np.int64)
    Pm = pc.dof_fold(a.n_ctrl, (axis,), a.dim)
    x = np.random.default_rng(29).standard_normal(Pm.shape[1])
    xm = x.copy()
    xm[ess] = 0.0
    v_u = Pm @ xm
    for arr in (ess, x, v_u):
        arr.setflags(write=False)
    return Pm, ess, x, v_u


@functools.lru_cache(maxsize=None)
def _reference_product(case, axis, face, matname):
    """K v_u of the long-double reference at the case's own u (u0 committed first for the stateful laws)"""
    r = dc.reference(case, matname)
    v_u = _product_inputs(case, axis, face)[3]
    return f64(dr.assemble(r.geo, r.mat, r.u, r.state, DT, [v_u]).Kv[0])


def _restore(Pm, ess, x, y_u):
    """mask(P^T y_u) + x[ess], the copies of a folded node added in ascending order from zero"""
    y = np.zeros(Pm.shape[1])
    np.add.at(y, Pm.indices, y_u)            # (row i of P has its single entry in column indices[i]: ascending i)
    y[ess] = x[ess]
    return y


def _folded_solver(case, axis, face):
    from mimi_amd.linear import LinearSolver
    a = dc.arrays(case)
    fold = _fold(_pattern_of(case), a.n_ctrl, (axis,), a.dim)
    _, ess, _, _ = _product_inputs(case, axis, face)
    S = LinearSolver(fold.Pattern(), ess)
    S.SetOperatorFold(fold)
    return S, fold


def _pattern_of(case):
    from mimi_amd.integrators import CSRPattern
    rowptr, col, _ = dc.pattern(case)
    return CSRPattern(np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), len(col))


@pytest.mark.parametrize("matname", ["neohook", "j2"])
@pytest.mark.parametrize("case, axis, face", PRODUCTS, ids=lambda v: str(v))
def test_folded_product_against_the_reference(case, axis, face, matname):
    import torch
    from mimi_amd.integrators import PeriodicFold
    from mimi_amd.linear import LinearSolver
    from test_matrix_free_gpu import linearized
    a = dc.arrays(case)
    Pm, ess, x, v_u = _product_inputs(case, axis, face)
    G, r = linearized(case, matname)
    fold = PeriodicFold(_pattern_of(case), pc.node_map(a.n_ctrl, (axis,)), a.dim).Prepare()
    assert fold.n_f_ == Pm.shape[1] and fold.n_u_ == Pm.shape[0]
    S = LinearSolver(fold.Pattern(), ess)
    S.SetOperatorFold(fold)
    S.SetOperator(G, 0.0, 1.0, 0.0)
    y = S.OperatorMult(np.array(x), np.full(len(x), np.nan))
    Kv = _reference_product(case, axis, face, matname)
    want = _restore(Pm, ess, x, Kv)
    free = np.setdiff1d(np.arange(len(x)), ess)
    dev = np.abs(y - want)[free].max() / np.abs(Kv).max()
    print(f"\n{case} axis {axis} {matname}: the folded product deviates {dev:.2e} (bar {dc.tangent_bar(matname):.2e})")
    assert np.isfinite(y).all() and dev <= dc.tangent_bar(matname)
    assert np.array_equal(y[ess], x[ess])
    # the bytes: PeriodicFold.Add of the unfolded action on the expanded masked vector, then the restore step in numpy
    y_u = np.zeros(len(v_u))
    G.ApplyTangent(np.array(v_u), y_u)
    folded = np.zeros(len(x))
    fold.Add(y_u, folded)
    folded[ess] = x[ess]
    assert y.tobytes() == folded.tobytes() == _restore(Pm, ess, x, y_u).tobytes()
    # twice, and with device arguments
    assert S.OperatorMult(np.array(x), np.full(len(x), np.nan)).tobytes() == y.tobytes()
    dev0 = torch.device("cuda", 0)
    d_y = torch.full((len(x),), float("nan"), dtype=torch.float64, device=dev0)
    S.OperatorMult(torch.from_numpy(np.array(x)).to(dev0), d_y)
    assert d_y.cpu().numpy().tobytes() == y.tobytes()


def test_folded_mass_and_viscosity_terms():
    from test_matrix_free_gpu import handle
    case, axis, face = PRODUCTS[0]
    Pm, ess, x, v_u = _product_inputs(case, axis, face)
    geo = dc.geometry(case)
    G = handle(case, "neohook")
    S, fold = _folded_solver(case, axis, face)
    free = np.setdiff1d(np.arange(len(x)), ess)
    for name, coefficients, times in (("mass", (dc.RHO, 0.0, 0.0), dr.mass_times(geo, dc.RHO, v_u)),
                                      ("viscosity", (0.0, 0.0, dc.NU), dr.diffusion_times(geo, dc.NU, v_u))):
        S.SetOperator(G, *coefficients)                       # (stiffness 0: no Linearize needed)
        y = S.OperatorMult(np.array(x), np.full(len(x), np.nan))
        want = _restore(Pm, ess, x, f64(times))
        dev = np.abs(y - want)[free].max() / np.abs(f64(times)).max()
        print(f"\n{case} axis {axis}: folded {name} term deviates {dev:.2e} (bar {dc.FORMS_BAR:.2e})")
        assert dev <= dc.FORMS_BAR and np.array_equal(y[ess], x[ess])


def test_folded_product_with_a_contact_and_a_pressure_term():
    """the faces of test_boundary_action_gpu.py's system (contact on axis 2 / side 1, pressure on axis 1 / side 1) on the bent
    block p2_6x4x2 made periodic along axis 0: the folded product is the fold of the handles' own unfolded actions"""
    from mimi_amd.integrators import CSRPattern, FollowerPressure, MortarContact, NonlinearSolid, RigidPlane
    from mimi_amd.linear import LinearSolver
    name, fac0, axes = "p2_6x4x2", 1e-2, (0,)
    P, B = kc.solve_patch(name)
    _, u, _ = kc.solve_inputs(name)
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    X = np.asarray(P.ctrl, dtype=np.float64) + u.reshape(-1, P.dim)
    top = X[:, 2] >= X[:, 2].max() - 0.35 * (X[:, 2].max() - X[:, 2].min())
    contact = MortarContact(RigidPlane([0.0, 0.0, float(X[top, 2].mean())], [0.0, 0.0, -1.0], 1e4), "contact", pattern, B, 2, 1).Prepare()
    pressure = FollowerPressure("pressure", pattern, B, 1, 1).Prepare()
    pressure.SetPressure(25.0)
    for h in (G, contact, pressure):
        h.Linearize(u)
    fold = _fold(pattern, P.n, axes, P.dim)
    ess = pc.folded_face_dofs(P, axes, [(1, 0)])
    Pm = pc.dof_fold(P.n, axes, P.dim)
    S = LinearSolver(fold.Pattern(), ess)
    S.SetOperatorFold(fold)
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    x = np.random.default_rng(31).standard_normal(Pm.shape[1])
    y_domain = S.OperatorMult(np.array(x), np.full(len(x), np.nan))
    S.AddBoundaryOperator(contact, fac0)
    S.AddBoundaryOperator(pressure, fac0)
    y = S.OperatorMult(np.array(x), np.full(len(x), np.nan))
    xm = x.copy()
    xm[ess] = 0.0
    v_u = Pm @ xm
    y_u = np.zeros(len(v_u))
    G.ApplyTangent(np.array(v_u), y_u, stiffness=fac0, density=kc.RHO)
    only_domain = y_u.copy()
    contact.ApplyTangent(np.array(v_u), y_u, fac0)
    after_contact = y_u.copy()
    pressure.ApplyTangent(np.array(v_u), y_u, fac0)
    assert np.abs(after_contact - only_domain).max() > 0 and np.abs(y_u - after_contact).max() > 0
    assert y.tobytes() == _restore(Pm, ess, x, y_u).tobytes()
    assert y_domain.tobytes() == _restore(Pm, ess, x, only_domain).tobytes()


# ---- (8) ---------------------------------------------------------------------------------------------------------------------
def test_rules_of_the_seam():
    import torch
    from mimi_amd.integrators import PeriodicFold
    from mimi_amd.linear import LinearSolver
    from test_matrix_free_gpu import handle, linearized
    case, axis, face = PRODUCTS[2]
    a = dc.arrays(case)
    Pm, ess, x, v_u = _product_inputs(case, axis, face)
    G, r = linearized(case, "neohook")
    fold = PeriodicFold(_pattern_of(case), pc.node_map(a.n_ctrl, (axis,)), a.dim).Prepare()
    S = LinearSolver(fold.Pattern(), ess)
    nan = lambda n=len(x): np.full(n, np.nan)
    # a fold of another size
    other_axis = PRODUCTS[0]
    b = dc.arrays(other_axis[0])
    wrong = PeriodicFold(_pattern_of(other_axis[0]), pc.node_map(b.n_ctrl, (other_axis[1],)), b.dim).Prepare()
    with pytest.raises(RuntimeError, match="folded dofs"):
        S.SetOperatorFold(wrong)
    # a fold on another device
    if torch.cuda.device_count() > 1:
        elsewhere = PeriodicFold(_pattern_of(case), pc.node_map(a.n_ctrl, (axis,)), a.dim, device=1).Prepare()
        with pytest.raises(RuntimeError, match="on device 1, the solver on device 0"):
            S.SetOperatorFold(elsewhere)
    # without a fold the unwrapped domain does not fit the folded solver
    with pytest.raises(RuntimeError, match="dofs"):
        S.SetOperator(G, 0.0, 1.0, 0.0)
    # a fold, but no operator
    S.SetOperatorFold(fold)
    S.preconditioner = "none"
    for call in (lambda: S.Mult(None, np.zeros(len(x)), nan()), lambda: S.MultCG(None, np.zeros(len(x)), nan()),
                 lambda: S.OperatorMult(np.array(x), nan())):
        with pytest.raises(RuntimeError, match="no operator is set"):
            call()
    # with the fold a domain of the folded size is the wrong one
    with pytest.raises(RuntimeError, match="unwrapped side of the operator fold"):
        S.SetOperator(handle("one3d_p3", "neohook"), 0.0, 1.0, 0.0)
    S.SetOperator(G, 0.0, 1.0, 0.0)
    y = S.OperatorMult(np.array(x), nan())
    # SetOperator keeps the fold (and drops nothing else of it)
    S.SetOperator(G, 0.0, 1.0, 0.0)
    assert S.OperatorMult(np.array(x), nan()).tobytes() == y.tobytes()
    # the fold cleared under a set operator: the solve is refused, not run out of bounds
    S.SetOperatorFold(None)
    with pytest.raises(RuntimeError, match="dofs"):
        S.OperatorMult(np.array(x), nan())
    # on a solver of the unwrapped size: an identity fold and none give the unfolded product bit for bit
    identity = PeriodicFold(_pattern_of(case), np.arange(a.n_nodes), a.dim).Prepare()
    ess_u = np.sort(np.concatenate([fr.face_node_ids(a.n_ctrl, *face) * a.dim + c for c in range(a.dim)])).astype(np.int64)
    U = LinearSolver(_pattern_of(case), ess_u)
    U.SetOperator(G, 0.0, 1.0, 0.0)
    xu = np.random.default_rng(37).standard_normal(a.n_vdofs)
    plain = U.OperatorMult(np.array(xu), nan(a.n_vdofs))
    U.SetOperatorFold(identity)
    through = U.OperatorMult(np.array(xu), nan(a.n_vdofs))
    assert np.array_equal(through, plain)             # (equal values: a sum of one copy from zero turns -0.0 into 0.0)
    U.SetOperatorFold(None)
    assert U.OperatorMult(np.array(xu), nan(a.n_vdofs)).tobytes() == plain.tobytes()
    fresh = LinearSolver(_pattern_of(case), ess_u)
    fresh.SetOperator(G, 0.0, 1.0, 0.0)
    assert fresh.OperatorMult(np.array(xu), nan(a.n_vdofs)).tobytes() == plain.tobytes()


# ---- (9) ---------------------------------------------------------------------------------------------------------------------
def _folded_operator_solver(name, axis, fac0):
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from mimi_amd.kronecker import KroneckerOperator
    from mimi_amd.linear import LinearSolver
    sysm = pc.folded_system(name, axis, fac0)
    P, B = sysm.P, sysm.B
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    fold = _fold(pattern, P.n, sysm.axes, P.dim)
    S = LinearSolver(fold.Pattern(), sysm.ess)
    S.SetKronecker(KroneckerOperator(B, sysm.ess, P.dim, periodic_axes=sysm.axes))
    S.SetKroneckerCoefficients(kc.RHO, kc.stiff(P.dim, fac0))
    S.SetOperatorFold(fold)
    S.preconditioner = "kronecker"
    return sysm, G, S


@pytest.mark.parametrize("fac0", kc.FAC0)
@pytest.mark.parametrize("name, axis", pc.SOLVES)
def test_gmres_with_the_folded_operator(name, axis, fac0):
    sysm, G, S = _folded_operator_solver(name, axis, fac0)
    S.max_iter = 3000
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(np.array(sysm.u))
    x = S.Mult(None, sysm.b, np.full(len(sysm.b), np.nan))
    x_ref = np.array([float(v) for v in ref.solve_extended(sysm.J, sysm.b)])
    dev = np.abs(x - x_ref).max() / np.abs(x_ref).max()
    want = pc.ITERATIONS[(name, axis, fac0)][1]
    print(f"\n{name} axis {axis} fac0 {fac0:g}: iterations {S.final_iter_} (restatement {want}), x deviates {dev:.3g} "
          f"(bar {kc.BAR * pc.DEV_SOLVE_PERIODIC:.3g})")
    assert S.converged_ and np.isfinite(x).all()
    assert S.final_iter_ == want
    assert dev <= kc.BAR * pc.DEV_SOLVE_PERIODIC


def test_cg_with_the_folded_mass_operator():
    name, axis = pc.CG_CASE
    sysm, G, S = _folded_operator_solver(name, axis, kc.FAC0[0])
    S.SetKroneckerCoefficients(kc.RHO, np.zeros(sysm.P.dim ** 2))
    S.SetOperator(G, kc.RHO, 0.0, 0.0)
    x = S.MultCG(None, sysm.b, np.full(len(sysm.b), np.nan))
    print(f"\n{name} axis {axis}: CG iterations on the folded mass operator {S.final_iter_} (restatement {pc.CG_ITERATIONS})")
    assert S.converged_ and S.final_iter_ == pc.CG_ITERATIONS
    assert np.abs(sysm.M @ x - sysm.b).max() <= 1e-7 * np.abs(sysm.b).max()


# ---- (10) --------------------------------------------------------------------------------------------------------------------
KRONECKER = (("use_iterative_solver", 1), ("use_kronecker_preconditioner", 1), ("periodic_iterative", 1))
MATRIX_FREE = KRONECKER + (("matrix_free", 1),)
BODY = -40.0


def _periodic_cube(matname, flags, mark=None):
    """cube_p2 clamped at boundary 0, attributes 3 and 5 joined, under a body force (the set-up of test_periodic_gpu.py and
    test_explicit_gpu.py); three implicit steps: (facade, x after each step, GMRES iterations)"""
    def configure(bc):
        for c in range(3):
            bc.initial.dirichlet(0, c)
        bc.initial.body_force(2, BODY)
        bc.initial.periodic(3, 5)
        if mark:
            mark(bc)
    nl = ec.facade("cube_p2", matname, flags=flags, configure=configure)
    nl.configure_newton("nonlinear_solid", 1e-12, 1e-10, 20, False)
    nl.time_step_size = 0.05
    total = [0]
    mult = nl.linear_.Mult

    def counted(A, *args):
        assert (A is None) == nl.matrix_free_
        out = mult(A, *args)
        assert nl.linear_.converged_
        total[0] += nl.linear_.final_iter_
        return out
    nl.linear_.Mult = counted
    x = nl.solution_view("displacement", "x")
    xs = []
    for _ in range(3):
        nl.step_time2()
        assert nl.newton_history[-1]["converged"]
        xs.append(x.copy())
    return nl, xs, total[0]


@pytest.mark.parametrize("matname", ["neohook", "j2"])
def test_facade_routes_against_the_periodic_direct_route(matname):
    direct, x_direct, _ = _periodic_cube(matname, ())
    assert direct.fold_ is not None and not direct.use_iterative_solver_ and hasattr(direct, "d_Au_")
    assembled, x_a, it_a = _periodic_cube(matname, KRONECKER)
    assert assembled.use_kronecker_ and assembled.linear_.preconditioner == "kronecker" and hasattr(assembled, "d_jac_")
    free, x_b, it_b = _periodic_cube(matname, MATRIX_FREE)
    assert free.matrix_free_ and not hasattr(free, "d_Au_") and not hasattr(free, "d_jac_")
    print(f"\n{matname}: GMRES iterations of three periodic steps, assembled {it_a}, matrix-free {it_b}")
    assert np.abs(x_direct[-1]).max() > 1e-6
    for xa, xb, xc in zip(x_a, x_b, x_direct):
        assert np.allclose(xa, xc) and np.allclose(xb, xc)
    assert it_a == it_b > 0


def test_facade_matrix_free_boundary_with_a_pressure_on_an_exterior_face():
    """a follower pressure on boundary 1 (the top, which the pair (3, 5) leaves exterior): matrix-free with its action against
    the assembled periodic route"""
    mark = lambda bc: bc.initial.pressure(1, 30.0)
    assembled, x_a, _ = _periodic_cube("neohook", KRONECKER, mark)
    free, x_b, it = _periodic_cube("neohook", MATRIX_FREE + (("matrix_free_boundary", 1),), mark)
    assert len(free.pressures_) == 1 and not free.pressures_[0].HoldsTangentBlocks() and assembled.pressures_[0].HoldsTangentBlocks()
    assert not hasattr(free, "d_Au_") and not hasattr(free, "d_jac_") and it > 0
    plain, x_c, _ = _periodic_cube("neohook", KRONECKER)
    assert np.abs(x_a[-1] - x_c[-1]).max() > 1e-3 * np.abs(x_c[-1]).max()       # the pressure acts
    for xa, xb in zip(x_a, x_b):
        assert np.allclose(xb, xa)


def test_without_the_flag_the_facade_refuses_the_pair_on_the_device_too():
    with pytest.raises(RuntimeError, match="periodic 1-D matrices"):
        _periodic_cube("neohook", KRONECKER[:2])


# ---- (11) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(ec.CM_RUNS))
def test_consistent_mass_with_a_pair(run):
    lu, cg, bar_x, bar_v, bar_e = pc.cm_reference(run)
    matname, eta = ec.CM_RUNS[run]

    def configure(bc):
        for c in range(3):
            bc.initial.dirichlet(0, c)
        bc.initial.periodic(*pc.CM_PAIR)
    nl = ec.facade(pc.CM_CASE, matname, flags=(("explicit_dynamics", 1), ("explicit_consistent_mass", 1), ("periodic_iterative", 1)),
                   configure=configure, viscosity=eta)
    assert nl.fold_ is not None and nl.explicit_consistent_
    nl.time_step_size = ec.CM_DT
    nl.solution_view("displacement", "x_dot")[:] = pc.cm_initial_velocity()
    nl.explicit_steps(ec.STEPS)
    ex, ev = np.abs(nl.x - lu.x).max(), np.abs(nl.x_dot - lu.v).max()
    print(f"{run}: x {ex:.2e} of bar {bar_x:.2e}, v {ev:.2e} of bar {bar_v:.2e}, CG iterations {nl.explicit_cg_iterations_} / {cg.iterations}")
    assert np.abs(lu.x).max() > 1e-3
    assert ex <= bar_x and ev <= bar_v
    assert nl.explicit_cg_iterations_ == cg.iterations
    if matname == "j2":
        assert lu.eqps.max() > 1e-3
        assert np.abs(nl.domain_.State("accumulated_plastic_strain") - lu.eqps).max() <= bar_e
    with pytest.raises(RuntimeError, match="ledger belongs to the lumped-mass step"):
        nl.explicit_energies()
    assert getattr(nl, "d_jac_", None) is None and nl.d_mass_ is None and getattr(nl, "d_Au_", None) is None
