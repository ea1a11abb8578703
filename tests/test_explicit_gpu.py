"""NonlinearSolid under rc.set_int("explicit_dynamics", 1) on the device, against the numpy restatement of the scheme
(tests/_explicit_reference.py around the oracle's internal force and state commit; cases and bars: tests/_explicit_cases.py)
and against the scheme's exact properties: free fall, the conservation of E*, prescribed dofs bit for bit, continuation."""
import hashlib
import os

import numpy as np
import pytest

import _explicit_cases as ec

pytestmark = pytest.mark.gpu
PAIRS = [(c, m) for c in ec.FIVE_STEP_CASES for m in ec.MATERIALS]


def set_velocity(nl, v):
    nl.solution_view("displacement", "x_dot")[:] = v


# ---- 1. lumped mass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ec.FIVE_STEP_CASES))
def test_lumped_mass_is_the_row_sum_of_the_consistent_mass(case):
    import torch
    import scipy.sparse as sp
    from oracle import ref_path as rp
    nl = ec.facade(case, "neohook")
    m = nl.d_lumped_mass_.cpu().numpy()
    assert m.min() > 0
    # the row sums of AddMass on the same handle
    pat = nl.pattern_u_
    vals = torch.zeros(pat.nnz, dtype=torch.float64, device="cuda")
    nl.domain_.AddMass(nl.material.density, vals)
    n = nl.patch_.n_vdofs
    rows = np.asarray(sp.csr_matrix((vals.cpu().numpy(), np.asarray(pat.col), np.asarray(pat.rowptr)), shape=(n, n)).sum(axis=1)).ravel()
    assert np.abs(m - rows).max() <= 1e-13 * np.abs(rows).max()
    # and of the oracle's mass matrix (what the restatement steps with)
    P = ec.oracle_patch(case)
    mo = ec.lumped_mass(P, rp.DomainOracle(P, ec.material_pair("neohook")[0]))
    assert np.abs(m - mo).max() <= 1e-13 * np.abs(mo).max()


def test_lumped_mass_is_folded_with_a_periodic_pair():
    """cube_p2 with the opposite faces of attributes 3 and 5 joined (as tests/test_periodic_gpu.py joins them): the folded
    lumped mass is P^T of the unwrapped one, and still sums to rho x volume per component"""
    plain = ec.facade("cube_p2", "neohook")
    m_u = plain.d_lumped_mass_.cpu().numpy()

    def configure(bc):
        for c in range(3):
            bc.initial.dirichlet(0, c)
        bc.initial.periodic(3, 5)
    nl = ec.facade("cube_p2", "neohook", configure=configure)
    assert nl.fold_ is not None
    nm = nl.dof_map("displacement")
    want = np.zeros((nm.max() + 1, 3))
    np.add.at(want, nm, m_u.reshape(-1, 3))
    m_f = nl.d_lumped_mass_.cpu().numpy()
    assert m_f.size == want.size < m_u.size
    assert np.abs(m_f - want.ravel()).max() <= 1e-13 * np.abs(want).max()
    assert abs(m_f.sum() - m_u.sum()) <= 1e-13 * m_u.sum()
    # a periodic explicit run goes through the fold: it moves, the joined nodes move together (one dof) and E* holds
    rng = np.random.default_rng(3)
    v = 2.0 * rng.standard_normal(m_f.size)
    v[nl.dirichlet_] = 0.0
    set_velocity(nl, v)
    e0 = nl.explicit_energies()
    nl.explicit_steps(20)
    e = nl.explicit_energies()
    assert np.abs(nl.x).max() > 1e-3 and e["W_int"] > 1e-3 * e0["KE"]
    assert abs(e["E_star"] - e0["E_star"]) <= 1e-12 * e0["KE"]


# ---- 2. five steps against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", PAIRS, ids=[f"{c}-{m}" for c, m in PAIRS])
def test_five_steps_against_the_restatement(case, matname):
    ref = ec.reference(case, matname)
    bar_x, bar_v, bar_e = ec.bars(case, matname)
    nl = ec.facade(case, matname)
    set_velocity(nl, ec.initial_velocity(ec.oracle_patch(case)))
    nl.explicit_steps(ec.STEPS)
    assert nl.domain_.LastKernelFamily() == ec.CASES[case][3]
    ex, ev = np.abs(nl.x - ref.x).max(), np.abs(nl.x_dot - ref.v).max()
    print(f"{case} {matname}: x {ex:.2e} of bar {bar_x:.2e}, v {ev:.2e} of bar {bar_v:.2e}")
    assert ex <= bar_x and ev <= bar_v
    assert np.abs(nl.explicit_acceleration() - ref.a).max() <= 2.0 * bar_v / (0.5 * ec.DT)        # (v = vh + dt/2 a, both within bar_v)
    if ec.is_j2(matname):
        assert ref.eqps.max() > 1e-3                                    # the law yielded within the five steps
        ee = np.abs(nl.domain_.State("accumulated_plastic_strain") - ref.eqps).max()
        print(f"   eqps {ee:.2e} of bar {bar_e:.2e}")
        assert ee <= bar_e
    # KE = 1/2 sum m v^2 moves by at most sum m |v| bar_v (plus rounding)
    ke = float(ref.energies["KE"])
    assert abs(nl.explicit_energies()["KE"] - ke) <= float((ref.m * np.abs(ref.v)).sum()) * bar_v + 1e-13 * ke
    assert nl.current_time == pytest.approx(ec.STEPS * ec.DT, rel=1e-14) and nl.runtime_communication.i_timestep_ == ec.STEPS


# ---- 3. free fall ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sq_p2", "cube_p3"])
def test_free_fall(case):
    """a body force rho g and no Dirichlet dof: every node has a = g from the start, x = 1/2 g t^2 and v = g t"""
    g, steps = -9.81, 50
    dim = 2 if case == "sq_p2" else 3
    nl = ec.facade(case, "neohook", configure=lambda bc: bc.initial.body_force(dim - 1, g * 1.0))
    nl.explicit_steps(steps)
    t = steps * ec.DT
    x, v = nl.x.reshape(-1, dim), nl.x_dot.reshape(-1, dim)
    assert np.abs(x[:, dim - 1] - 0.5 * g * t * t).max() <= 1e-13 * abs(0.5 * g * t * t)
    assert np.abs(v[:, dim - 1] - g * t).max() <= 1e-13 * abs(g * t)
    assert np.abs(x[:, :dim - 1]).max() <= 1e-13 * abs(0.5 * g * t * t) and np.abs(v[:, :dim - 1]).max() <= 1e-13 * abs(g * t)
    e = nl.explicit_energies()
    mass = float(nl.d_lumped_mass_.sum()) / dim
    ke = 0.5 * mass * (g * t) ** 2
    assert abs(e["KE"] - ke) <= 1e-12 * ke
    assert abs(e["W_int"]) <= 1e-12 * ke and e["W_damp"] == 0.0
    # the ledger: W_ext = f . x = 2 KE here, and KE - Q - W_ext stays at -Q_0 (Q is constant: a = g)
    assert abs(e["W_ext"] - mass * g * 0.5 * g * t * t) <= 1e-12 * ke
    assert abs(e["E_star"] + e["Q"]) <= 1e-12 * ke


# ---- 4. E* over 200 steps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(ec.E_RUNS))
def test_e_star_is_conserved_over_200_steps(run):
    ref = ec.e_reference(run)
    matname, viscosity, what = ec.E_RUNS[run]
    nl = ec.facade(ec.E_CASE, matname, configure=ec.e_configure(run), viscosity=viscosity)
    nl.time_step_size = ec.E_DT
    set_velocity(nl, ec.e_initial_velocity(ec.oracle_patch(ec.E_CASE), run))
    series, touched = [nl.explicit_energies()], False
    for _ in range(ec.E_STEPS // ec.E_EVERY):
        nl.explicit_steps(ec.E_EVERY)
        series.append(nl.explicit_energies())
        touched = touched or (what == "contact" and np.abs(nl.contacts_[0].last_force_).max() > 0.0)
    star = np.array([e["E_star"] for e in series])
    drift = np.abs(star - star[0]).max()
    bar = 8.0 * ref.drift
    print(f"{run}: E* drift {drift:.2e}, the restatement's {ref.drift:.2e} (bar {bar:.2e}), scale {ref.scale:.2e}")
    # the run is the one the restatement made
    last = series[-1]
    for k in ("KE", "W_int", "W_ext", "W_damp"):
        assert abs(last[k] - float(ref.last[k])) <= 1e-6 * ref.scale, k
    if matname == "j2":
        assert nl.domain_.State("accumulated_plastic_strain").max() > 1e-3            # beyond yield
    if viscosity:
        assert last["W_damp"] > 1e-3 * ref.scale
    if what == "contact":
        assert touched                                                                  # the plane was reached
    if what == "cv":
        assert abs(last["W_ext"]) > 1e-2 * ref.scale                                   # the moving face did work
    assert drift <= bar
    if run == "neohook":
        # hyperelastic, clamped, undamped: KE + W_int - W_ext leaves its start value by Q - Q_0 only; the band is the largest
        # excursion the restatement shows over all 200 steps (the device is sampled at a subset of them)
        total = np.array([e["KE"] + e["W_int"] - e["W_ext"] for e in series])
        print(f"   KE + W_int - W_ext: excursion {np.abs(total - total[0]).max():.3e}, the restatement's band {ref.band:.3e}")
        assert ref.band > 100 * bar
        assert np.abs(total - total[0]).max() <= ref.band + bar


# ---- 5. prescribed dofs ----------------------------------------------------------------------------------------------------
def test_prescribed_dofs_bit_for_bit():
    steps = 7
    nl = ec.facade("cube_p2", "neohook", configure=ec.e_configure("constant_velocity"))
    P = ec.oracle_patch("cube_p2")
    v0 = ec.e_initial_velocity(P, "constant_velocity")
    set_velocity(nl, v0)
    x0 = 0.01 * np.random.default_rng(9).standard_normal(nl.x.size)
    nl.solution_view("displacement", "x")[:] = x0
    nl.explicit_steps(steps)
    cv = nl.constant_velocity_dofs_
    fixed = np.setdiff1d(nl.dirichlet_, cv)
    assert len(cv) and len(fixed)
    assert np.array_equal(nl.x[fixed], x0[fixed]) and np.all(nl.x_dot[fixed] == 0.0)
    assert np.array_equal(nl.x_dot[cv], np.full(len(cv), ec.E_CV))
    want = x0[cv].copy()
    for _ in range(steps):
        want = want + nl.time_step_size * ec.E_CV
    assert np.array_equal(nl.x[cv], want)
    assert np.all(nl.explicit_acceleration()[nl.dirichlet_] == 0.0)
    free = np.setdiff1d(np.arange(nl.x.size), nl.dirichlet_)
    assert np.abs(nl.x[free] - x0[free]).max() > 1e-4


# ---- 6. continuation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname,viscosity", [("neohook", None), ("j2", 0.05)])
def test_continuation_and_restart(matname, viscosity):
    def start():
        nl = ec.facade("cube_p2", matname, viscosity=viscosity)
        nl.time_step_size = ec.E_DT
        set_velocity(nl, ec.e_initial_velocity(ec.oracle_patch("cube_p2"), "neohook"))
        return nl
    a, b = start(), start()
    a.explicit_steps(6)
    b.explicit_steps(3)
    b.explicit_steps(3)
    for get in (lambda s: s.x, lambda s: s.x_dot, lambda s: s.explicit_acceleration(),
                lambda s: np.array(list(s.explicit_energies().values()))):
        assert get(a).tobytes() == get(b).tobytes()
    assert a.current_time == b.current_time and a.runtime_communication.i_timestep_ == 6
    # a host edit of x_dot is taken up by explicit_restart (and the ledger starts again)
    xr = b.x.copy()
    free = np.setdiff1d(np.arange(xr.size), b.dirichlet_)
    edit = b.x_dot.copy()
    edit[free] *= 0.5
    b.solution_view("displacement", "x_dot")[:] = edit
    b.explicit_restart()
    e = b.explicit_energies()
    assert e["W_int"] == 0.0 and e["KE"] == pytest.approx(0.25 * a.explicit_energies()["KE"], rel=1e-12)
    b.explicit_steps(1)
    a.explicit_steps(1)
    moved_a, moved_b = np.linalg.norm(a.x - xr), np.linalg.norm(b.x - xr)
    assert 0.3 * moved_a < moved_b < 0.7 * moved_a


# ---- 7. save cadence ---------------------------------------------------------------------------------------------------------
def test_save_cadence_and_downloads(tmp_path):
    nl = ec.facade("sq_p2", "j2")
    rc = nl.runtime_communication
    rc.set_fname(os.path.join(str(tmp_path), "out.npz"))
    rc.append_should_save("x", 2)
    set_velocity(nl, ec.initial_velocity(ec.oracle_patch("sq_p2")))
    assert nl.explicit_d2h_copies_ == 0
    nl.explicit_steps(5)
    with np.load(rc.fname) as z:
        assert sorted(z.files) == ["x_2", "x_4"]
        x2, x4 = z["x_2"], z["x_4"]
    # two saves and the end of the call: x and x_dot each time, nothing else crossed
    assert nl.explicit_d2h_copies_ == 2 * 3
    twin = ec.facade("sq_p2", "j2")
    set_velocity(twin, ec.initial_velocity(ec.oracle_patch("sq_p2")))
    twin.explicit_steps(2)
    assert twin.explicit_d2h_copies_ == 2
    assert np.array_equal(x2, twin.in_reference_numbering(twin.x))
    twin.explicit_steps(2)
    assert np.array_equal(x4, twin.in_reference_numbering(twin.x))
    twin.explicit_steps(1)
    assert np.array_equal(nl.x, twin.x) and twin.explicit_d2h_copies_ == 6


# ---- 8. stable time step -------------------------------------------------------------------------------------------------------
def dense_lambda(nl, viscosity=None):
    """(lambda_max(M_l^-1 K(0)), lambda_max(M_l^-1 eta C)) on the free dofs, dense, from the device's own assembled matrices"""
    import scipy.linalg
    import scipy.sparse as sp
    import torch
    pat = nl.pattern_u_
    n = nl.patch_.n_vdofs
    free = np.setdiff1d(np.arange(n), nl.dirichlet_)
    m = nl.d_lumped_mass_.cpu().numpy()
    out = []
    r, A = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(pat.nnz, dtype=torch.float64, device="cuda")
    nl._push(nl.domain_)
    nl.domain_.AddDomainResidualAndGrad(torch.zeros(n, dtype=torch.float64, device="cuda"), 1.0, r, A)
    mats = [A]
    if viscosity:
        C = torch.zeros(pat.nnz, dtype=torch.float64, device="cuda")
        nl.domain_.AddDiffusion(viscosity, C)
        mats.append(C)
    for vals in mats:
        K = sp.csr_matrix((vals.cpu().numpy(), np.asarray(pat.col), np.asarray(pat.rowptr)), shape=(n, n)).toarray()
        K = 0.5 * (K + K.T)
        out.append(scipy.linalg.eigh(K[np.ix_(free, free)], np.diag(m[free]), eigvals_only=True)[-1])
    return out + [0.0] * (2 - len(out))


@pytest.mark.parametrize("case", ["sq_p2", "cube_p2"])
def test_stable_time_step_against_the_dense_eigenvalue(case):
    nl = ec.facade(case, "neohook")
    lam, _ = dense_lambda(nl)
    dt = nl.stable_time_step(safety=1.0, rel_tol=1e-10, max_iter=500)
    exact = 2.0 / np.sqrt(lam)
    print(f"{case}: dt {dt:.8e} exact {exact:.8e} rel {dt / exact - 1:.2e} after {nl.stable_iterations_} iterations")
    assert nl.stable_iterations_ <= 500
    assert abs(dt - exact) <= 1e-6 * exact
    assert dt >= exact * (1 - 1e-12)            # the Rayleigh quotient comes from below: the estimate errs long, never short
    assert 0.9 * exact * (1 - 1e-12) <= nl.stable_time_step() < exact      # the defaults: the safety factor covers the loose tolerance
    # at a deformed state the limit moves
    u = 0.05 * np.random.default_rng(2).standard_normal(nl.x.size)
    u[nl.dirichlet_] = 0.0
    assert nl.stable_time_step(u=u, safety=1.0, rel_tol=1e-8) != dt


def test_stable_time_step_with_viscosity():
    eta = 0.05
    nl = ec.facade("cube_p2", "neohook", viscosity=eta)
    lam_k, lam_c = dense_lambda(nl, eta)
    dt = nl.stable_time_step(safety=1.0, rel_tol=1e-10, max_iter=500)
    omega = np.sqrt(lam_k)
    xi = lam_c / (2 * omega)
    exact = (2.0 / omega) * (np.sqrt(1 + xi * xi) - xi)
    assert xi > 1e-3
    assert abs(dt - exact) <= 1e-6 * exact
    assert abs(nl.stable_lambda_[0] - lam_k) <= 1e-6 * lam_k and abs(nl.stable_lambda_[1] - lam_c) <= 1e-6 * lam_c


# ---- 9. consistent mass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(ec.CM_RUNS))
def test_consistent_mass_five_steps(run):
    """rc.set_int("explicit_consistent_mass", 1): (rho M + dt/2 eta C) a = f - r - eta C v_{n+1/2} by the operator CG, against
    the restatement that solves it with the oracle's matrices and scipy's LU; the CG iteration counts are the restated CG's"""
    lu, cg, bar_x, bar_v, bar_e = ec.cm_reference(run)
    matname, eta = ec.CM_RUNS[run]
    nl = ec.facade(ec.CM_CASE, matname, flags=(("explicit_dynamics", 1), ("explicit_consistent_mass", 1)), viscosity=eta)
    nl.time_step_size = ec.CM_DT
    set_velocity(nl, ec.cm_initial_velocity(ec.oracle_patch(ec.CM_CASE)))
    nl.explicit_steps(ec.STEPS)
    ex, ev = np.abs(nl.x - lu.x).max(), np.abs(nl.x_dot - lu.v).max()
    print(f"{run}: x {ex:.2e} of bar {bar_x:.2e}, v {ev:.2e} of bar {bar_v:.2e}, CG iterations {nl.explicit_cg_iterations_} / {cg.iterations}")
    assert ex <= bar_x and ev <= bar_v
    assert nl.explicit_cg_iterations_ == cg.iterations
    assert np.abs(nl.explicit_acceleration() - lu.a).max() <= 2.0 * bar_v / (0.5 * ec.CM_DT)
    if matname == "j2":
        assert lu.eqps.max() > 1e-3
        assert np.abs(nl.domain_.State("accumulated_plastic_strain") - lu.eqps).max() <= bar_e
    # no ledger on this route, no matrix either; the lumped route on the same input gives another answer
    with pytest.raises(RuntimeError, match="ledger belongs to the lumped-mass step"):
        nl.explicit_energies()
    assert getattr(nl, "d_jac_", None) is None and nl.d_mass_ is None and nl.d_visc_ is None
    lumped = ec.facade(ec.CM_CASE, matname, viscosity=eta)
    lumped.time_step_size = ec.CM_DT
    set_velocity(lumped, ec.cm_initial_velocity(ec.oracle_patch(ec.CM_CASE)))
    lumped.explicit_steps(ec.STEPS)
    assert np.abs(lumped.x_dot - lu.v).max() > 100 * bar_v
    # continuation holds here too
    twin = ec.facade(ec.CM_CASE, matname, flags=(("explicit_dynamics", 1), ("explicit_consistent_mass", 1)), viscosity=eta)
    twin.time_step_size = ec.CM_DT
    set_velocity(twin, ec.cm_initial_velocity(ec.oracle_patch(ec.CM_CASE)))
    twin.explicit_steps(2)
    twin.explicit_steps(3)
    assert twin.x.tobytes() == nl.x.tobytes() and twin.x_dot.tobytes() == nl.x_dot.tobytes()


def test_consistent_mass_flag_rules():
    for flags, periodic, match in (((("explicit_consistent_mass", 1),), False, "needs explicit_dynamics"),
                                   ((("explicit_dynamics", 1), ("explicit_consistent_mass", 1)), True, "periodic")):
        def configure(bc):
            for c in range(3):
                bc.initial.dirichlet(0, c)
            if periodic:
                bc.initial.periodic(3, 5)
        with pytest.raises(RuntimeError, match=match):
            ec.facade("cube_p2", "neohook", flags=flags, configure=configure)


# ---- 10. flag rules ---------------------------------------------------------------------------------------------------------
def test_flag_rules():
    nl = ec.facade("sq_p2", "neohook", viscosity=0.05)
    assert getattr(nl, "d_jac_", None) is None and nl.d_mass_ is None and nl.d_visc_ is None
    assert nl._mass_host is None and nl.mass_ is None
    for entry in (nl.step_time2, nl.fixed_point_solve2, nl.fixed_point_advance2, nl.advance_time2):
        with pytest.raises(RuntimeError, match="under explicit_dynamics"):
            entry()
    for other in ("matrix_free", "use_iterative_solver", "host_setup"):
        with pytest.raises(RuntimeError, match="explicit_dynamics cannot be combined"):
            ec.facade("sq_p2", "neohook", flags=(("explicit_dynamics", 1), (other, 1)))
    off = ec.facade("sq_p2", "neohook", flags=())
    with pytest.raises(RuntimeError, match="explicit dynamics is off"):
        off.explicit_steps(1)
    assert off.d_jac_ is not None and off.d_mass_ is not None


def test_the_implicit_route_is_untouched():
    """with the flag unset (absent, or set to 0) step_time2 is the implicit route as before: the same bytes either way, a
    Jacobian and a mass matrix on the device, no stepper.  The SHA-1 of x after three steps of the golden beam
    (tests/test_nonlinear_solid.py: beam("neohook")) is printed; DESIGN.md 4.10 records it beside the parent commit's, which is
    equal (the direct solve runs on the host, so the digest belongs to a machine and is not asserted here)."""
    from test_nonlinear_solid import beam
    runs = []
    for runtime in ((), (("explicit_dynamics", 0),)):
        nl = beam("neohook", runtime=runtime)
        assert not nl.explicit_ and nl.d_jac_ is not None and not hasattr(nl, "explicit_stepper_")
        for _ in range(3):
            nl.step_time2()
        runs.append(nl.x.copy())
    print("golden beam, three implicit steps: sha1(x) =", hashlib.sha1(runs[0].tobytes()).hexdigest())
    assert runs[0].tobytes() == runs[1].tobytes() and np.abs(runs[0]).max() > 1e-3
