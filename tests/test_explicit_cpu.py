"""The explicit central-difference step without a GPU: the C surface (header, exports, ABI), the numpy restatement of the
scheme (tests/_explicit_reference.py) on its two exact properties -- E* is conserved, free fall is reproduced -- the power
iteration of stable_time_step against a dense eigenvalue, and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import _explicit_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mimi_hip_explicit_create", "mimi_hip_explicit_destroy", "mimi_hip_explicit_set_stream", "mimi_hip_explicit_synchronize",
           "mimi_hip_explicit_info", "mimi_hip_explicit_set_mass", "mimi_hip_explicit_start", "mimi_hip_explicit_predict",
           "mimi_hip_explicit_correct", "mimi_hip_explicit_acceleration", "mimi_hip_explicit_energies"]


def test_header_declares_and_library_exports_the_explicit_entries():
    from mimi_amd import build, _capi, explicit
    raw = open(os.path.join(ROOT, "include", "mimi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mimi_hip_explicit_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRIES)
    assert set(declared) <= set(_capi.EXPORTS)
    everything = sorted(set(re.findall(r"\b(mimi_hip_[a-z0-9_]+)\s*\(", text)))
    assert sorted(_capi.EXPORTS) == everything
    assert "#define MIMI_HIP_ABI_VERSION 12" in text
    assert "explicit.hip" in build.SOURCES
    # what the step stands in for is cited with the entries
    section = raw[raw.index("explicit central-difference step"):]
    assert section.count("ode.cpp:229-250") >= 6
    import torch  # noqa: F401  (torch's HIP runtime first, as _capi.lib() loads it)
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in declared)
    lib.mimi_hip_abi_version.restype = ctypes.c_int
    assert lib.mimi_hip_abi_version() == 12
    # the shape of the sums: the library's constants are the ones the tests import
    lib.mimi_hip_explicit_info.restype = ctypes.c_int64
    lib.mimi_hip_explicit_info.argtypes = [ctypes.c_void_p, ctypes.c_int]
    shape = [lib.mimi_hip_explicit_info(None, k) for k in (4, 5, 6, 7)]
    assert shape == [explicit.SUM_BLOCK, explicit.SUM_GRID_CAP, explicit.SUM_FINAL_RUN, explicit.SUM_TREE_DEPTH]
    assert explicit.SUM_FINAL_RUN * explicit.SUM_BLOCK == explicit.SUM_GRID_CAP
    assert explicit.SUM_TREE_DEPTH == 2 * int(np.log2(explicit.SUM_BLOCK))
    assert lib.mimi_hip_explicit_info(None, 0) == -1
    # a null handle is an error status with a message, not a crash
    lib.mimi_hip_last_error.restype = ctypes.c_char_p
    assert lib.mimi_hip_explicit_predict(None, ctypes.c_double(0.1), None, None) != 0
    assert b"null" in lib.mimi_hip_last_error()


def test_sum_shape_helpers():
    from mimi_amd import explicit
    cap = explicit.SUM_GRID_CAP * explicit.SUM_BLOCK
    assert explicit.sum_grid(1) == 1 and explicit.sum_grid(257) == 2 and explicit.sum_grid(cap + 1) == explicit.SUM_GRID_CAP
    assert explicit.sum_run_length(1) == 1 + explicit.SUM_FINAL_RUN
    assert explicit.sum_run_length(cap) == 1 + explicit.SUM_FINAL_RUN
    assert explicit.sum_run_length(cap + 1) == 2 + explicit.SUM_FINAL_RUN


def nonlinear_system(T):
    """12 dofs: a chain of cubic springs with a contact-like one-sided spring, two constant-velocity dofs, one fixed dof,
    a load and a (symmetric positive semi-definite) damping matrix"""
    n = 12
    rng = np.random.default_rng(11)
    m = T(1) + np.asarray(rng.uniform(0, 1, n), dtype=T)
    k1, k3 = np.asarray(rng.uniform(20, 40, n - 1), dtype=T), np.asarray(rng.uniform(100, 300, n - 1), dtype=T)
    L = np.zeros((n - 1, n))
    for i in range(n - 1):
        L[i, i], L[i, i + 1] = -1, 1
    L = np.asarray(L, dtype=T)
    C = T(0.3) * (L.T @ L)

    def force(x):
        e = L @ x
        wall = np.where(x[-1] > T(0.05), T(500) * (x[-1] - T(0.05)), T(0))       # one-sided: not a potential of a smooth kind
        r = L.T @ (k1 * e + k3 * e ** 3)
        r[-1] = r[-1] + wall
        return r

    fixed, pres = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    fixed[0] = True
    pres[[3, 7]] = True
    vbar = np.zeros(n, dtype=T)
    vbar[3], vbar[7] = T(0.2), T(-0.15)
    f = np.asarray(rng.uniform(-1, 1, n), dtype=T)
    v0 = np.asarray(rng.uniform(-0.5, 0.5, n), dtype=T)
    return m, fixed, pres, vbar, f, v0, force, (lambda v: C @ v)


def test_restatement_conserves_e_star_in_long_double():
    """E* = KE - Q + W_int + W_damp - W_ext is conserved exactly by the scheme, for a nonlinear non-smooth force, with the
    lagged damping, a load, a fixed and two constant-velocity dofs: 400 steps in long double stay within 1e-17 of the energy
    scale (long double carries 2^-64 = 5.4e-20 per operation)"""
    T = np.longdouble
    assert np.finfo(T).eps < 2e-19, "this platform's long double is no wider than double"
    m, fixed, pres, vbar, f, v0, force, damping = nonlinear_system(T)
    s = er.Stepper(m, fixed, pres, vbar, dtype=T).start(np.zeros(12, dtype=T), v0, f, force, damping)
    dt = 0.004
    e0 = s.energies(dt)
    scale, worst = abs(e0["KE"]), T(0)
    for _ in range(400):
        s.step(dt)
        e = s.energies(dt)
        scale = max(scale, abs(e["KE"]), abs(e["W_int"]), abs(e["W_ext"]), abs(e["W_damp"]))
        worst = max(worst, abs(e["E_star"] - e0["E_star"]))
    # the run did something: plastic-like dissipation through the damping, work by the prescribed dofs, the wall was hit
    assert e["W_damp"] > 1e-4 * scale and abs(e["W_ext"]) > 1e-3 * scale and s.x[-1] != 0
    print(f"E* deviation {float(worst):.2e} of scale {float(scale):.2e}")
    assert worst <= 1e-17 * scale
    # the same system in doubles: the drift is rounding (the bar of the device runs is taken from figures like this one)
    m, fixed, pres, vbar, f, v0, force, damping = nonlinear_system(np.float64)
    s = er.Stepper(m, fixed, pres, vbar).start(np.zeros(12), v0, f, force, damping)
    e0 = s.energies(dt)
    for _ in range(400):
        s.step(dt)
    assert abs(s.energies(dt)["E_star"] - e0["E_star"]) <= 400 * 40 * 2.0 ** -53 * float(scale)


def test_restatement_reproduces_free_fall_exactly():
    """a body force and no fixed dof: a = g from the start, so x = 1/2 g t^2 and v = g t with no truncation error; with
    dt and g powers of two the doubles are exact too"""
    n, g, dt = 7, -8.0, 2.0 ** -6
    m = np.linspace(1.0, 2.5, n)
    s = er.Stepper(m).start(np.zeros(n), np.zeros(n), m * g, lambda x: np.zeros(n))
    for _ in range(50):
        s.step(dt)
    t = 50 * dt
    assert np.array_equal(s.x, np.full(n, 0.5 * g * t * t)) and np.array_equal(s.v, np.full(n, g * t))
    e = s.energies(dt)
    assert e["W_int"] == 0.0 and e["W_damp"] == 0.0
    assert e["KE"] == 0.5 * m.sum() * (g * t) ** 2
    # the ledger: KE - Q - W_ext is what it was at the start (-Q_0; Q is constant here)
    assert abs(e["E_star"] + e["Q"]) <= 1e-15 * e["KE"]


@pytest.mark.parametrize("case", ["sq_p2", "cube_p2"])
def test_power_iteration_reaches_the_dense_eigenvalue(case):
    """lambda_max(M_l^-1 K) at rest on the two meshes tests/test_explicit_gpu.py asks stable_time_step about, the bottom
    clamped: the iteration of stable_time_step (numpy here, the oracle's tangent and the row sums of its mass matrix)
    against scipy.linalg.eigh, within 1e-6 in at most 500 iterations from the fixed start vector, and from below"""
    from oracle import ref_path as rp
    from mimi_amd import explicit
    import _explicit_cases as ec
    P = ec.oracle_patch(case)
    D = rp.DomainOracle(P, ec.material_pair("neohook")[0])
    n = P.n_vdofs
    r, A = np.zeros(n), np.zeros(D.nnz)
    D.add_domain_residual_and_grad(np.zeros(n), 1.0, r, A, rp.TANGENT_EXACT)
    K = sp.csr_matrix((A, D.col, D.rowptr), shape=(n, n))
    m = ec.lumped_mass(P, D)
    assert m.min() > 0
    free = 1.0 - ec.clamped_bottom(P)
    idx = np.flatnonzero(free)
    Kd = K.toarray()
    Kd = 0.5 * (Kd + Kd.T)
    dense = scipy.linalg.eigh(Kd[np.ix_(idx, idx)], np.diag(m[idx]), eigvals_only=True)[-1]
    lam, it = explicit.power_lambda_max(lambda z: K @ z, m, free, explicit.power_start(n), 1e-10, 500)
    print(f"{case}: lambda {lam:.10e} dense {dense:.10e} rel {abs(lam - dense) / dense:.2e} after {it} iterations")
    assert it <= 500
    assert abs(lam - dense) <= 1e-6 * dense
    assert lam <= dense * (1 + 1e-12)


def test_five_step_bars_are_well_conditioned():
    """the bars of tests/test_explicit_gpu.py::test_five_steps_against_the_restatement, derived here on the CPU: none
    exceeds 1e-9 max|x| (a case that did would be ill-conditioned and replaced, not loosened), the J2 laws yield within the
    five steps, and the figures are the ones recorded in tests/_explicit_cases.py"""
    import _explicit_cases as ec
    for case in ec.CASES:
        for matname in ec.MATERIALS:
            ref = ec.reference(case, matname)
            bx, bv, be = ec.bars(case, matname)
            rel = (bx / np.abs(ref.x).max(), bv / np.abs(ref.v).max(), be)
            print(f'("{case}", "{matname}"): ({rel[0]:.2e}, {rel[1]:.2e}, {rel[2]:.2e})')
            assert 0 < rel[0] <= 1e-9
            assert np.allclose(rel, ec.MEASURED[(case, matname)], rtol=0.02)
            if ec.is_j2(matname):
                assert ref.eqps.max() > 1e-3 and (ref.eqps > 0).mean() > 0.5


def test_e_star_drift_of_the_restatement():
    """the float64 restatement's own E* drift over the 200 steps of every run of the device test: rounding, a few units in
    the last place of the energy scale -- the device's bar is 8 x this figure"""
    import _explicit_cases as ec
    for run in ec.E_RUNS:
        ref = ec.e_reference(run)
        print(f'"{run}": {ref.drift:.2e} of scale {ref.scale:.3e}')
        assert 0 < ref.drift <= 64 * 2.0 ** -53 * ref.scale
        assert ref.drift == pytest.approx(ec.E_DRIFT_MEASURED[run], rel=1e-2, abs=0)
    # the example's input (tests/test_explicit_example_gpu.py)
    dt = ec.example_dt()
    ref = ec.example_reference(dt)
    print(f"example: dt {dt:.7e}, drift {ref.drift:.2e} of scale {ref.series[0]['KE']:.3e}")
    assert 0 < ref.drift <= 64 * 2.0 ** -53 * ref.series[0]["KE"] and ref.eqps.max() > 1e-3
    assert ref.drift == pytest.approx(ec.EX_DRIFT_MEASURED, rel=1e-2, abs=0)


def test_consistent_mass_bars_are_well_conditioned():
    """the bars and CG iteration counts of tests/test_explicit_gpu.py::test_consistent_mass_five_steps, derived here"""
    import _explicit_cases as ec
    for run in ec.CM_RUNS:
        lu, cg, bx, bv, be = ec.cm_reference(run)
        rel = (bx / np.abs(lu.x).max(), bv / np.abs(lu.v).max())
        print(f'"{run}": ({rel[0]:.2e}, {rel[1]:.2e}, {cg.iterations})')
        assert 0 < rel[0] <= 1e-9
        assert np.allclose(rel, ec.CM_MEASURED[run][:2], rtol=0.02) and cg.iterations == ec.CM_MEASURED[run][2]
        assert np.abs(cg.x - lu.x).max() <= ec.MARGIN * bx              # the restated CG sits inside the bar it helped derive
        if run == "j2_viscous":
            assert lu.eqps.max() > 1e-3


def test_stable_step_formula():
    from mimi_amd import explicit
    # no damping: 2 / omega; with damping the limit of the lagged scheme, below it
    assert explicit.stable_step_from(4.0, 0.0, 1.0) == 1.0
    xi = 3.0 / (2 * 2.0)
    assert explicit.stable_step_from(4.0, 3.0, 0.9) == pytest.approx(0.9 * (np.sqrt(1 + xi * xi) - xi), rel=1e-15)


MESH = os.path.join(ROOT, "tests", "golden", "meshes", "square-nurbs.mesh")


def test_consistent_mass_flag_refusals_before_any_device_work():
    import mimi_amd as mimi
    for flags, periodic, match in (((("explicit_consistent_mass", 1),), False, "needs explicit_dynamics"),
                                   ((("explicit_dynamics", 1), ("explicit_consistent_mass", 1)), True, "periodic")):
        nl = mimi.NonlinearSolid()
        nl.read_mesh(MESH)
        rc = mimi.RuntimeCommunication()
        for k, v in flags:
            rc.set_int(k, v)
        nl.runtime_communication = rc
        bc = mimi.BoundaryConditions()
        if periodic:
            bc.initial.periodic(3, 4)
        nl.boundary_condition = bc
        with pytest.raises(RuntimeError, match=match):
            nl.setup(1)


@pytest.mark.parametrize("other", ["matrix_free", "use_iterative_solver", "host_setup"])
def test_flag_refusals_before_any_device_work(other):
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(MESH)
    rc = mimi.RuntimeCommunication()
    rc.set_int("explicit_dynamics", 1)
    rc.set_int(other, 1)
    nl.runtime_communication = rc
    nl.boundary_condition = mimi.BoundaryConditions()
    with pytest.raises(RuntimeError, match="explicit_dynamics cannot be combined"):
        nl.setup(1)


def test_explicit_entries_refuse_without_the_flag():
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    for call in (lambda: nl.explicit_steps(1), nl.explicit_energies, nl.explicit_restart, nl.stable_time_step):
        with pytest.raises(RuntimeError, match="explicit dynamics is off"):
            call()
