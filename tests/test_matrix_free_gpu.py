"""The matrix-free tangent action (csrc/kernels_apply.hpp) through the C ABI: NonlinearSolid.Linearize / ApplyTangent,
LinearSolver.SetOperator and the facade's "matrix_free" flag.

(1) the stiffness action on every (case, material) of tests/_domain_cases.py -- J2Log and J2Simo with their three laws among
    them (dc.FINITE_PAIRS) -- against the long-double reference's K v, within the bar the assembled tangent is held to
    (dc.tangent_bar, relative to max |K v|); the kernel family and the bytes of record;
(2) the mass and viscosity terms against dr.mass_times / dr.diffusion_times within dc.FORMS_BAR, and their sum in one call;
(3) J2Simo and J2Log against the handle's own assembled tangent within dc.TANGENT_BAR, and on the same cases against the
    reference's K v within dc.tangent_bar: a tangent record that is wrong in the assembly and the action alike fails the second;
(4) element boxes: the sum of the boxes' actions is the whole;
(5) semantics: equal bytes, the snapshot, the refusal, host and device arguments, symmetry;
(6) solves with the operator on the systems of test_kronecker_gpu.py: the iteration count of the restated GMRES, the solution
    of the extended-precision direct solve; CG on a mass operator;
(7) the rules of the seam;
(8) the golden beams through the facade with the flag, and its refusals;
(9) the order of first use on a handle does not matter: assembly, nodal field, mass form and action in either order."""
import numpy as np
import pytest
import scipy.sparse as sp

import _domain_cases as dc
import _domain_reference as dr
import _kronecker_cases as kc
import _kronecker_reference as ref
from _cases import product_material
from _domain_cases import DT, f64

pytestmark = pytest.mark.gpu


def relmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max() / max(np.abs(f64(b)).max(), 1e-300))


def handle(case, material, element_box=None):
    """the product handle of a case of _domain_cases (material: a name of dc, or a product material)"""
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    a = dc.arrays(case)
    rowptr, col, _ = dc.pattern(case)
    pattern = CSRPattern(np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), len(col))
    mat = dc.product_material(material) if isinstance(material, str) else material
    if a.flat:
        G = NonlinearSolid("domain", mat, pattern, tables=dict(dc.flat_tables(case))).Prepare()
    else:
        G = NonlinearSolid("domain", mat, pattern, patch=dc.product_patch(case), quadrature_order=a.order,
                           element_box=element_box).Prepare()
    G.dt_ = DT
    return G


def info(G, what):
    from mimi_amd import _capi
    return int(_capi.lib().mimi_hip_domain_info(G._handle(), what))


FAMILY_CODES = {"tensor_p2_two_phase": 1, "tensor_p3_two_phase": 2, "tensor_small": 3, "general": 4}


def action(G, v, **coefficients):
    """the increment of ApplyTangent in accumulate form on a random y0"""
    y0 = np.random.default_rng(11).standard_normal(len(v))
    y = y0.copy()
    G.ApplyTangent(np.array(v), y, **coefficients)
    return y - y0


def linearized(case, matname, element_box=None):
    r = dc.reference(case, matname)
    G = handle(case, matname, element_box)
    if r.mat.stateful:
        G.DomainPostTimeAdvance(r.u0)
    G.Linearize(np.array(r.u))
    return G, r


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", dc.PAIRS, ids=lambda v: v)
def test_stiffness_action_against_the_reference(case, matname):
    a = dc.arrays(case)
    G, r = linearized(case, matname)
    worst = 0.0
    for v, Kv in zip(r.vectors, r.asm.Kv):
        worst = max(worst, relmax(action(G, v), Kv))
        assert info(G, 9) == FAMILY_CODES[a.family]
    print(f"\n{case} {matname} [{a.family}]: K v deviates {worst:.2e} (bar {dc.tangent_bar(matname):.2e})")
    assert worst <= dc.tangent_bar(matname)
    assert G.LastActionFamily() == a.family
    if not a.flat and a.family != "general":
        assert info(G, 8) == 0
    n_pts = G.n_elements_ * G.n_quad_
    assert info(G, 10) == (0 if matname == "neohook" else n_pts * a.dim ** 4 * 8)
    assert G.LinearizationBytes() == info(G, 10)


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.FORMS_CASES)
def test_mass_and_viscosity_terms(case):
    geo = dc.geometry(case)
    G = handle(case, "neohook")
    fig = dict(mass=0.0, viscosity=0.0)
    for v in dc.probes(case):
        m = action(G, v, stiffness=0.0, density=dc.RHO)            # (no Linearize: stiffness 0 needs none)
        c = action(G, v, stiffness=0.0, viscosity=dc.NU)
        fig["mass"] = max(fig["mass"], relmax(m, dr.mass_times(geo, dc.RHO, v)))
        fig["viscosity"] = max(fig["viscosity"], relmax(c, dr.diffusion_times(geo, dc.NU, v)))
    print(f"\n{case}: " + ", ".join(f"{k} {x:.2e}" for k, x in fig.items()))
    assert fig["mass"] <= dc.FORMS_BAR and fig["viscosity"] <= dc.FORMS_BAR
    r = dc.reference(case, "neohook")
    G.Linearize(np.array(r.u))
    for v, Kv in zip(dc.probes(case), r.asm.Kv):
        parts = (action(G, v, stiffness=0.0, density=dc.RHO), action(G, v, stiffness=0.0, viscosity=dc.NU), action(G, v))
        whole = action(G, v, stiffness=1.0, density=dc.RHO, viscosity=dc.NU)
        # the sum of the three single-coefficient calls, each term within its own bar
        bar = dc.FORMS_BAR * (np.abs(parts[0]).max() + np.abs(parts[1]).max()) + dc.tangent_bar("neohook") * np.abs(parts[2]).max()
        assert np.abs(whole - (parts[0] + parts[1] + parts[2])).max() <= bar
        want = f64(dr.mass_times(geo, dc.RHO, v)) + f64(dr.diffusion_times(geo, dc.NU, v)) + f64(Kv)
        assert np.abs(whole - want).max() <= bar


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["j2simo", "j2log"])
@pytest.mark.parametrize("case", list(dc.EXTRA.values()))
def test_finite_strain_laws_against_the_assembled_tangent(case, model):
    a = dc.arrays(case)
    u0, u = dc.inputs(case, "j2")
    G = handle(case, product_material(model))
    G.DomainPostTimeAdvance(u0)
    rowptr, col, _ = dc.pattern(case)
    vals = np.zeros(len(col))
    G.AddDomainResidualAndGrad(np.array(u), 1.0, np.zeros(a.n_vdofs), vals)
    K = sp.csr_matrix((vals, col, rowptr), shape=(a.n_vdofs, a.n_vdofs))
    G.Linearize(np.array(u))
    worst = max(relmax(action(G, v), K @ v) for v in dc.probes(case))
    print(f"\n{case} {model} [{a.family}]: action deviates {worst:.2e} from K v (bar {dc.TANGENT_BAR:.2e})")
    assert worst <= dc.TANGENT_BAR
    assert info(G, 9) == FAMILY_CODES[a.family]
    assert info(G, 10) == G.n_elements_ * G.n_quad_ * a.dim ** 4 * 8
    # independently: the same model at its own inputs (dc.SEEDS) against the long-double reference's K v
    G, r = linearized(case, model)
    worst = max(relmax(action(G, v), Kv) for v, Kv in zip(r.vectors, r.asm.Kv))
    print(f"{case} {model} [{a.family}]: action deviates {worst:.2e} from the reference's K v (bar {dc.tangent_bar(model):.2e})")
    assert worst <= dc.tangent_bar(model)
    assert info(G, 9) == FAMILY_CODES[a.family]


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", ["neohook", "j2"])
def test_element_boxes_add_up(matname):
    case = dc.BOX_CASE
    boxes = [linearized(case, matname, element_box=box) for box in dc.BOXES]
    r = boxes[0][1]
    for v, Kv in zip(r.vectors, r.asm.Kv):
        total = sum(action(G, v) for G, _ in boxes)
        assert relmax(total, Kv) <= dc.tangent_bar(matname)


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", [("col8_p2", "neohook"), ("col8_p2", "j2"), ("rep2d_p3", "j2"), ("mix3d_231", "stvk")])
def test_snapshot_and_equal_bytes(case, matname):
    import torch
    G, r = linearized(case, matname)
    v = r.vectors[0]
    first = action(G, v, density=dc.RHO, viscosity=dc.NU)
    assert action(G, v, density=dc.RHO, viscosity=dc.NU).tobytes() == first.tobytes()
    # the snapshot: the caller's u overwritten, another dt, a commit at another displacement
    G2 = handle(case, matname)
    if r.mat.stateful:
        G2.DomainPostTimeAdvance(r.u0)
    u = np.array(r.u)
    G2.Linearize(u)
    u[:] = np.nan
    G2.dt_ = 0.25 * DT
    G2._push_dt()
    G2.DomainPostTimeAdvance(np.array(r.u))
    assert action(G2, v, density=dc.RHO, viscosity=dc.NU).tobytes() == first.tobytes()
    # device arguments: the bytes of the host call
    dev = torch.device("cuda", 0)
    y0 = np.random.default_rng(11).standard_normal(len(v))
    d_y = torch.from_numpy(y0.copy()).to(dev)
    G.ApplyTangent(torch.from_numpy(np.array(v)).to(dev), d_y, density=dc.RHO, viscosity=dc.NU)
    G.Synchronize()
    assert (d_y.cpu().numpy() - y0).tobytes() == first.tobytes()
    # a linearisation from a device tensor: the same record
    G3 = handle(case, matname)
    if r.mat.stateful:
        G3.DomainPostTimeAdvance(r.u0)
    G3.Linearize(torch.from_numpy(np.array(r.u)).to(dev))
    assert action(G3, v, density=dc.RHO, viscosity=dc.NU).tobytes() == first.tobytes()


def test_stiffness_before_linearize_is_refused():
    G = handle("rep2d_p2", "neohook")
    v = dc.probes("rep2d_p2")[0]
    with pytest.raises(RuntimeError, match="before any mimi_hip_domain_linearize"):
        G.ApplyTangent(np.array(v), np.zeros(len(v)))
    G.ApplyTangent(np.array(v), np.zeros(len(v)), stiffness=0.0, density=1.0)


def test_mass_term_on_flat_tables_needs_shape_values():
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    case = "flat2d_p4"
    rowptr, col, _ = dc.pattern(case)
    tables = dict(dc.flat_tables(case))
    tables.pop("N")
    G = NonlinearSolid("domain", dc.product_material("neohook"), CSRPattern(np.array(rowptr), np.array(col, dtype=np.int32), len(col)),
                       tables=tables).Prepare()
    v = dc.probes(case)[0]
    with pytest.raises(RuntimeError, match="set_shape_values"):
        G.ApplyTangent(np.array(v), np.zeros(len(v)), stiffness=0.0, density=1.0)
    G.ApplyTangent(np.array(v), np.zeros(len(v)), stiffness=0.0, viscosity=1.0)


@pytest.mark.parametrize("matname", ["neohook", "stvk"])
@pytest.mark.parametrize("case", ["rep2d_p2", "col8_p2", "col5_p3", "mix3d_231"])
def test_hyperelastic_action_is_symmetric(case, matname):
    G, r = linearized(case, matname)
    v, w = r.vectors[0], r.vectors[1]
    Kv, Kw = action(G, v), action(G, w)
    a, b = float(w @ Kv), float(v @ Kw)
    size = float(np.abs(w) @ np.abs(Kv))
    print(f"\n{case} {matname}: w.Kv {a:.6e}, v.Kw {b:.6e}, asymmetry {abs(a - b) / size:.2e}")
    assert abs(a - b) <= dc.SYMMETRY_BAR * size


# ---- (6) ---------------------------------------------------------------------------------------------------------------------
def _operator_system(name, fac0):
    """test_kronecker_gpu.py::_device_system, keeping the domain handle: (domain, solver with the Kronecker operator, the
    device-assembled eliminated J as the reference matrix, values, patch, essential dofs, u, b)"""
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from test_kronecker_gpu import _kronecker_solver
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
    return G, S, J, vals, P, ess, u, b


@pytest.mark.parametrize("fac0", kc.FAC0)
@pytest.mark.parametrize("name", list(kc.SOLVES))
def test_gmres_with_the_operator(name, fac0):
    G, S, J, vals, P, ess, u, b = _operator_system(name, fac0)
    S.max_iter = 3000
    restated = ref.gmres(J, b, ref.dense_preconditioner(P, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0)), max_iter=3000)
    assert restated.converged and ref.margin(restated) >= kc.MARGIN
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    G.Linearize(np.array(u))
    S.preconditioner = "kronecker"
    x = S.Mult(None, b, np.full(len(b), np.nan))
    x_ref = np.array([float(v) for v in ref.solve_extended(J, b)])
    dev = np.abs(x - x_ref).max() / np.abs(x_ref).max()
    print(f"\n{name} fac0 {fac0:g}: iterations {S.final_iter_} (restatement {restated.iterations}), x deviates {dev:.3g} "
          f"(bar {kc.BAR * kc.DEV_SOLVE:.3g})")
    assert S.converged_ and np.isfinite(x).all()
    assert S.final_iter_ == restated.iterations
    assert dev <= kc.BAR * kc.DEV_SOLVE


@pytest.mark.parametrize("kind", ["face", "none"])
def test_cg_with_the_mass_operator_of_an_affine_block(kind):
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from test_kronecker_gpu import _kronecker_solver
    P, B = kc.grid("p2_5x4x3")
    ess = kc.essential(P, kind)
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    S = _kronecker_solver(pattern, B, ess, P.dim, kc.RHO, np.zeros(P.dim * P.dim))
    S.Eliminate(None, vals)
    b = np.random.default_rng(5).standard_normal(P.n_vdofs)
    b[ess] = 0.0
    S.SetOperator(G, kc.RHO, 0.0, 0.0)
    S.preconditioner = "kronecker"
    x = S.MultCG(None, b, np.full(len(b), np.nan))
    print(f"\nmass operator [{kind}]: CG iterations {S.final_iter_}")
    assert S.converged_ and S.final_iter_ <= 2
    M = sp.csr_matrix((vals, col, rowptr), shape=(len(b), len(b)))
    assert np.abs(M @ x - b).max() <= 1e-8 * np.abs(b).max()


# ---- (7) ---------------------------------------------------------------------------------------------------------------------
def test_rules_of_the_seam():
    from mimi_amd.linear import LinearSolver
    from test_kronecker_gpu import _kronecker_solver
    name, fac0 = "2d_p3_8x4", 1e-2
    G, S, J, vals, P, ess, u, b = _operator_system(name, fac0)
    nan = lambda: np.full(len(b), np.nan)
    S.preconditioner = "kronecker"
    with pytest.raises(RuntimeError, match="no operator is set"):
        S.Mult(None, b, nan())
    with pytest.raises(RuntimeError, match="no operator is set"):
        S.MultCG(None, b, nan())
    S.SetOperator(G, kc.RHO, fac0, 0.0)
    with pytest.raises(RuntimeError, match="before any mimi_hip_domain_linearize"):
        S.Mult(None, b, nan())
    G.Linearize(np.array(u))
    S.preconditioner = "jacobi"
    with pytest.raises(RuntimeError, match="matrix values"):
        S.Mult(None, b, nan())
    with pytest.raises(RuntimeError, match="matrix values"):
        S.MultCG(None, b, nan())
    S.preconditioner = "none"
    S.max_iter = 3000
    x = S.Mult(None, b, nan())
    assert S.converged_ and np.abs(J @ x - b).max() <= 1e-6 * np.abs(b).max()
    # with the operator set, solves that pass the values give the bits of a handle that never saw an operator
    _, B = kc.solve_patch(name)
    for preconditioner in ("none", "jacobi", "kronecker"):
        got = []
        for solver in (S, _kronecker_solver(S.pattern_, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))):
            solver.preconditioner = preconditioner
            solver.max_iter = 300
            x = solver.Mult(vals, b, nan())
            got.append((x.tobytes(), solver.final_iter_, np.float64(solver.final_norm_).tobytes(), solver.converged_))
            x = solver.MultCG(vals, b, nan(), max_iter=60)
            got.append((x.tobytes(), solver.final_iter_, np.float64(solver.final_norm_).tobytes(), solver.converged_))
        assert got[0] == got[2] and got[1] == got[3]
        assert got[0][1] > 1
    # cleared: None is an error again
    S.ClearOperator()
    S.preconditioner = "kronecker"
    with pytest.raises(RuntimeError, match="no operator is set"):
        S.Mult(None, b, nan())
    # a domain of another size
    other = handle("rep2d_p2", "neohook")
    with pytest.raises(RuntimeError, match="dofs"):
        S.SetOperator(other, 1.0, 1.0, 0.0)
    assert isinstance(S, LinearSolver)


# ---- (8) ---------------------------------------------------------------------------------------------------------------------
FLAGS = [("use_iterative_solver", 1), ("use_kronecker_preconditioner", 1), ("matrix_free", 1)]


@pytest.mark.parametrize("case", ["neohook", "j2"])
def test_golden_beams_with_the_flag(golden_dir, case):
    import os
    from oracle import harness as hz
    from test_nonlinear_solid import GOLDEN_CASES, beam
    nl = beam(case, runtime=FLAGS)
    assert nl.matrix_free_ and nl.use_kronecker_ and not hasattr(nl, "d_jac_")
    total = [0]
    mult = nl.linear_.Mult

    def counted(A, *args):
        assert A is None
        out = mult(A, *args)
        assert nl.linear_.converged_
        total[0] += nl.linear_.final_iter_
        return out
    nl.linear_.Mult = counted
    u = nl.solution_view("displacement", "x").ravel()
    for i in range(3):
        nl.step_time2()
        golden = hz.golden_to_lexicographic(np.genfromtxt(os.path.join(golden_dir, "ref", GOLDEN_CASES[case]["refdir"], f"x_{i}.txt")))
        assert np.allclose(u, golden)
    print(f"\n{case}: GMRES iterations of three matrix-free steps {total[0]}")
    assert total[0] > 0 and not hasattr(nl, "d_jac_")


def test_the_flag_is_refused_where_the_action_does_not_reach():
    from mimi_amd.integrators import RigidPlane
    from test_nonlinear_solid import beam

    def prepared(runtime, mark=None):
        nl = beam("neohook", runtime=runtime, finish=False)
        if mark:
            mark(nl.boundary_condition)
        return nl

    with pytest.raises(RuntimeError, match="use_kronecker_preconditioner"):
        prepared([("use_iterative_solver", 1), ("matrix_free", 1)]).setup(1)
    with pytest.raises(RuntimeError, match="use_iterative_solver"):
        prepared([("matrix_free", 1)]).setup(1)
    with pytest.raises(RuntimeError, match="contact"):
        prepared(FLAGS, lambda bc: bc.current.contact(3, RigidPlane([0.0, -1.0], [0.0, 1.0]))).setup(1)
    with pytest.raises(RuntimeError, match="pressure"):
        prepared(FLAGS, lambda bc: bc.initial.pressure(3, 1.0)).setup(1)
    with pytest.raises(RuntimeError, match="periodic"):
        prepared(FLAGS, lambda bc: bc.initial.periodic(1, 2)).setup(1)



# ---- (9) ---------------------------------------------------------------------------------------------------------------------
# What a handle builds at first use (the node adjacency, the longest-row scan, the general tables, the scratch of the
# two-phase route) is shared by its assemblies, fields, forms and actions: whichever comes first, every call takes the same
# route and gives the same bytes.
FIRST_USE = {"small 4x3 p2 neohook": ((4, 3), 2, "neohook", None),
             "general 3x2x2 p2 j2": ((3, 2, 2), 2, "j2", {"MIMI_HIP_FORCE_GENERAL": "1"}),
             "tables 2x2 p3 j2": ((2, 2), 3, "j2", "tables")}


@pytest.mark.parametrize("name", list(FIRST_USE))
def test_order_of_first_use_does_not_matter(name, monkeypatch):
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    n_el, p, matname, how = FIRST_USE[name]
    dim = len(n_el)
    if how == "tables":
        from _cases import oracle_material
        from oracle import iga, ref_path as rp
        P = iga.Patch.block(n_el, p)
        D = rp.DomainOracle(P, oracle_material(matname), n_threads=1)
        n_nodes, nnz = P.n_nodes, D.nnz
        tables = dict(dim=dim, n_nodes=n_nodes, dofs=D.conn, dN_dX=D.dN_dX, weight_det=D.weight * D.det, N=np.ascontiguousarray(D.tables["N"]))
        create = lambda: NonlinearSolid("domain", product_material(matname), CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), nnz),
                                        tables=tables)
    else:
        patch = mimi_amd.BSplinePatch.block(n_el, p)
        n_nodes, nnz = patch.n_nodes, CSRPattern.of_bspline_patch(patch).nnz
        create = lambda: NonlinearSolid("domain", product_material(matname), CSRPattern.of_bspline_patch(patch), patch=patch)
    for k, v in (how if isinstance(how, dict) else {}).items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(97)
    u, x = 0.02 * rng.standard_normal(n_nodes * dim), rng.standard_normal(n_nodes * dim)
    r0, A0, M0, y0 = (rng.standard_normal(n) for n in (n_nodes * dim, nnz, nnz, n_nodes * dim))
    s0, w0 = rng.standard_normal((n_nodes, dim * dim)), rng.standard_normal(n_nodes)

    def assembly(G):
        r, A = r0.copy(), A0.copy()
        G.AddDomainResidualAndGrad(u, 0.37, r, A)
        return dict(r=r, A=A, family=np.array(info(G, 7)))

    def field(G):
        s, w = s0.copy(), w0.copy()
        G.NodalField("cauchy_stress", u, s, w)
        return dict(s=s, w=w)

    def mass(G):
        return dict(M=G.AddMass(1.3, M0.copy()))

    def act(G):
        G.Linearize(u)
        return dict(y=G.ApplyTangent(x, y0.copy(), stiffness=0.37, density=0.7, viscosity=0.11))

    steps = [assembly, field, mass, act]
    results = []
    for order in (steps, steps[::-1]):
        G = create().Prepare()
        G.dt_ = DT
        got = {}
        for step in order:
            got.update(step(G))
        results.append(got)
    first, second = results
    assert sorted(first) == ["A", "M", "family", "r", "s", "w", "y"]
    for key in first:
        assert np.isfinite(first[key]).all() and first[key].tobytes() == second[key].tobytes(), key
    assert int(first["family"]) == (FAMILY_CODES["tensor_small"] if how is None else FAMILY_CODES["general"])
