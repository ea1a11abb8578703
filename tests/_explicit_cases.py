"""Cases, inputs, references and bars of tests/test_explicit_gpu.py: NonlinearSolid under explicit_dynamics against the
numpy restatement of tests/_explicit_reference.py, whose internal force and state commit are the oracle's (oracle/ is read,
not changed) and whose lumped mass is the row sums of the oracle's mass matrix.

Cases: the kernel-family cases of tests/_domain_cases.py -- rep2d_p3 (tensor_small), col8_p2 (tensor_p2_two_phase), col5_p3
(tensor_p3_two_phase), mix3d_231 (general) -- and the rational patch nurbs_tp_p2 of its FORMS_CASES, each handed to the facade as
its patch; and three meshes the facade reads itself (one cell, refined uniformly), which the other tests run on --
  sq_p2    square-nurbs.mesh (a quadrilateral with a slanted side), degree 2, 2 x 2 elements      tensor_small
  cube_p2  cube-nurbs.mesh, degree 2, 2 x 2 x 2 elements                                          tensor_p2_two_phase
  cube_p3  cube-nurbs.mesh, degree 3, 2 x 2 x 2 elements                                          tensor_p3_two_phase
-- with the bottom (boundary 0) clamped.  Materials: neohook, j2 (the default law) and j2[JohnsonCookRate].  The initial
velocity is synthetic_u scaled by V_SCALE, which makes the J2 laws yield within the five steps (asserted on the CPU).

Bars, derived and never read off the device: the restatement is run a second time with every residual entry moved by that
residual's own bar with random signs (fixed seed) -- RESIDUAL_BAR x max|r| (tests/_domain_cases.py) and, for the J2 laws, the
stress a return map that stops at |d delta| < 1e-10 may be off by, integrated against |dN/dX| (tests/_radial_return.py:
stress_bar, once for the committed state and once for the step's own return) -- and the spread between the two runs,
divided by MARGIN = 0.125, is the bar of x, v after five steps; the committed plastic strain gets the spread / MARGIN plus
the 2 x 1e-10 of each of the five commits.  A case whose bar of x exceeds 1e-9 max|x| would be ill-conditioned and replaced;
tests/test_explicit_cpu.py asserts that none is.  MEASURED holds the figures this gives, for the record; the tests use the
derivation itself."""
import functools
import os
import types

import numpy as np

import _explicit_reference as er
import _radial_return as rr
from _cases import oracle_material, product_material, synthetic_u
import _domain_cases as _dc
from _domain_cases import MARGIN, RESIDUAL_BAR, is_j2, law_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(ROOT, "tests", "golden", "meshes")
CASES = {"sq_p2": ("square-nurbs.mesh", 1, 1, "tensor_small"),
         "cube_p2": ("cube-nurbs.mesh", 1, 1, "tensor_p2_two_phase"),
         "cube_p3": ("cube-nurbs.mesh", 2, 1, "tensor_p3_two_phase")}
# the kernel-family cases of tests/_domain_cases.py (EXTRA) and one rational patch of its FORMS_CASES: the patch is handed to the
# facade in place of the mesh's own (the mesh file supplies the boundary ids of a square / a box)
NAMED = ("rep2d_p3", "col8_p2", "col5_p3", "mix3d_231", "nurbs_tp_p2")
for _name in NAMED:
    _a = _dc.arrays(_name)
    CASES[_name] = ("square-nurbs.mesh" if _a.dim == 2 else "cube-nurbs.mesh", 0, 0, _a.family)
FIVE_STEP_CASES = NAMED + ("sq_p2", "cube_p2", "cube_p3")
MATERIALS = ("neohook", "j2", "j2[JohnsonCookRate]")
DT, STEPS, V_SCALE, RHO = 1e-4, 5, 60.0, 1.0
# (case, material) -> (bar of x / max|x|, bar of v / max|v|, bar of eqps), as `bars` computes them (printed by
# tests/test_explicit_cpu.py::test_five_step_bars_are_well_conditioned)
MEASURED = {
    ("rep2d_p3", "neohook"): (2.97e-14, 9.29e-14, 1.00e-09),   # |x| 9.341e-02
    ("rep2d_p3", "j2"): (9.88e-11, 1.96e-10, 1.01e-09),   # |x| 9.342e-02 eqps max 1.297e-01 plastic share 0.64
    ("rep2d_p3", "j2[JohnsonCookRate]"): (9.88e-11, 1.97e-10, 1.01e-09),   # |x| 9.342e-02 eqps max 1.047e-01 plastic share 0.64
    ("col8_p2", "neohook"): (1.19e-14, 3.65e-14, 1.00e-09),   # |x| 9.344e-02
    ("col8_p2", "j2"): (1.18e-10, 2.30e-10, 1.01e-09),   # |x| 9.344e-02 eqps max 9.031e-02 plastic share 0.70
    ("col8_p2", "j2[JohnsonCookRate]"): (1.18e-10, 2.30e-10, 1.01e-09),   # |x| 9.344e-02 eqps max 6.793e-02 plastic share 0.70
    ("col5_p3", "neohook"): (1.96e-14, 6.08e-14, 1.00e-09),   # |x| 9.344e-02
    ("col5_p3", "j2"): (1.58e-10, 3.17e-10, 1.02e-09),   # |x| 9.344e-02 eqps max 1.252e-01 plastic share 0.80
    ("col5_p3", "j2[JohnsonCookRate]"): (1.58e-10, 3.17e-10, 1.02e-09),   # |x| 9.344e-02 eqps max 1.004e-01 plastic share 0.80
    ("mix3d_231", "neohook"): (1.60e-14, 4.76e-14, 1.00e-09),   # |x| 9.344e-02
    ("mix3d_231", "j2"): (1.30e-10, 2.59e-10, 1.03e-09),   # |x| 9.344e-02 eqps max 1.301e-01 plastic share 0.70
    ("mix3d_231", "j2[JohnsonCookRate]"): (1.30e-10, 2.59e-10, 1.02e-09),   # |x| 9.344e-02 eqps max 1.050e-01 plastic share 0.70
    ("nurbs_tp_p2", "neohook"): (2.05e-14, 6.39e-14, 1.00e-09),   # |x| 9.344e-02
    ("nurbs_tp_p2", "j2"): (1.18e-10, 2.42e-10, 1.01e-09),   # |x| 9.344e-02 eqps max 8.475e-02 plastic share 0.68
    ("nurbs_tp_p2", "j2[JohnsonCookRate]"): (1.18e-10, 2.42e-10, 1.01e-09),   # |x| 9.344e-02 eqps max 6.281e-02 plastic share 0.68
    ("sq_p2", "neohook"): (2.80e-14, 5.29e-14, 1.00e-09),   # |x| 6.140e-02
    ("sq_p2", "j2"): (2.38e-10, 4.75e-10, 1.08e-09),   # |x| 6.141e-02 eqps max 1.274e-01 plastic share 0.89
    ("sq_p2", "j2[JohnsonCookRate]"): (2.38e-10, 4.75e-10, 1.07e-09),   # |x| 6.141e-02 eqps max 1.025e-01 plastic share 0.89
    ("cube_p2", "neohook"): (1.96e-14, 4.93e-14, 1.00e-09),   # |x| 9.339e-02
    ("cube_p2", "j2"): (2.35e-10, 4.66e-10, 1.06e-09),   # |x| 9.340e-02 eqps max 2.453e-01 plastic share 0.94
    ("cube_p2", "j2[JohnsonCookRate]"): (2.35e-10, 4.66e-10, 1.05e-09),   # |x| 9.339e-02 eqps max 2.152e-01 plastic share 0.94
    ("cube_p3", "neohook"): (3.89e-14, 1.21e-13, 1.00e-09),   # |x| 9.341e-02
    ("cube_p3", "j2"): (3.50e-10, 6.98e-10, 1.13e-09),   # |x| 9.341e-02 eqps max 3.185e-01 plastic share 0.96
    ("cube_p3", "j2[JohnsonCookRate]"): (3.50e-10, 6.98e-10, 1.13e-09),   # |x| 9.341e-02 eqps max 2.861e-01 plastic share 0.96
}


def material_pair(matname):
    if is_j2(matname):
        return oracle_material("j2", law_of(matname)), product_material("j2", law_of(matname))
    return oracle_material(matname), product_material(matname)


def facade(case, matname, flags=(("explicit_dynamics", 1),), configure=None, setup=True, viscosity=None, material=None):
    """the NonlinearSolid of a case, the bottom clamped unless `configure(bc)` says otherwise; setup=False: no device work;
    material: this product material instead of matname's"""
    import mimi_amd as mimi
    mesh, elevate, subdivide, _ = CASES[case]
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(MESHES, mesh))
    nl.elevate_degrees(elevate)
    nl.subdivide(subdivide)
    if case in NAMED:
        B = _dc.product_patch(case)
        nl.patch = lambda: B
    mat = material_pair(matname)[1] if material is None else material
    if viscosity is not None:
        mat.viscosity = viscosity
    nl.set_material(mat)
    bc = mimi.BoundaryConditions()
    if configure is None:
        for c in range(nl.mesh_dim()):
            bc.initial.dirichlet(0, c)
    else:
        configure(bc)
    nl.boundary_condition = bc
    rc = mimi.RuntimeCommunication()
    for k, v in flags:
        rc.set_int(k, v)
    nl.runtime_communication = rc
    nl.time_step_size = DT
    if setup:
        nl.setup(1)
    return nl


@functools.lru_cache(maxsize=None)
def oracle_patch(case):
    from oracle import iga
    B = facade(case, "neohook", setup=False).patch()
    return iga.Patch(list(B.degrees), [np.asarray(k, dtype=np.float64) for k in B.knots], np.asarray(B.control_points, dtype=np.float64),
                     None if getattr(B, "weights", None) is None else np.asarray(B.weights, dtype=np.float64))


def lumped_mass(P, D, rho=RHO):
    """the row sums of the oracle's consistent mass matrix"""
    import scipy.sparse as sp
    from oracle import harness as hz
    n = P.n_vdofs
    return np.asarray(sp.csr_matrix((hz.assemble_mass(P, D.tables, rho, D.rowptr, D.col), D.col, D.rowptr), shape=(n, n)).sum(axis=1)).ravel()


def clamped_bottom(P):
    """the dofs of boundary 0 (attribute 1: the face xi_last = 0)"""
    nodes = P.boundary_nodes(P.dim - 1, 0)
    fixed = np.zeros(P.n_vdofs, dtype=bool)
    for c in range(P.dim):
        fixed[nodes * P.dim + c] = True
    return fixed


def initial_velocity(P):
    v = synthetic_u(P, scale=V_SCALE, seed=20241008, clamp_axis=P.dim - 1)
    v.setflags(write=False)
    return v


def _residual_perturbation(P, D, matname, r, x, rng):
    """a vector of the size of the residual's own bar, random signs"""
    bar = np.full(r.size, RESIDUAL_BAR * np.abs(r).max())
    if is_j2(matname):
        dim = P.dim
        g = D.dN_dX                                                     # [e, q, J, a]
        ue = x.reshape(-1, dim)[D.conn]                                 # [e, a, i]
        F = np.eye(dim) + np.einsum("eai,eqJa->eqiJ", ue, g)
        JFinvT = np.linalg.det(F)[..., None, None] * np.swapaxes(np.linalg.inv(F), -1, -2)
        per_point = 2.0 * rr.stress_bar(np.sqrt((JFinvT ** 2).sum(axis=(-1, -2))))          # committed state + this return
        rows = np.zeros(P.n_nodes)
        np.add.at(rows, D.conn, np.einsum("eq,eqa->ea", D.weight * D.det * per_point, np.abs(g).sum(axis=2)))
        bar = bar + np.repeat(rows, dim)
    return bar * rng.choice([-1.0, 1.0], r.size)


def run_restatement(case, matname, perturb=False, steps=STEPS, dt=DT):
    from oracle import ref_path as rp
    P = oracle_patch(case)
    D = rp.DomainOracle(P, material_pair(matname)[0])
    D.set_dt(dt)
    rng = np.random.default_rng(77)

    def force(x):
        r = np.zeros(P.n_vdofs)
        D.add_domain_residual(x, r)
        return r + _residual_perturbation(P, D, matname, r, x, rng) if perturb else r

    s = er.Stepper(lumped_mass(P, D), clamped_bottom(P)).start(np.zeros(P.n_vdofs), initial_velocity(P), None, force,
                                                               commit=D.domain_post_time_advance)
    for _ in range(steps):
        s.step(dt)
    return types.SimpleNamespace(x=s.x.copy(), v=s.v.copy(), a=s.a.copy(), eqps=D.eqps.copy(), energies=s.energies(dt), m=s.m)


@functools.lru_cache(maxsize=None)
def reference(case, matname):
    """the five steps of the restatement: computed once, shared, never modified"""
    out = run_restatement(case, matname)
    for a in (out.x, out.v, out.a, out.eqps):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bars(case, matname):
    """(bar of x, bar of v, bar of eqps): absolute, as the module docstring derives them"""
    base, moved = reference(case, matname), run_restatement(case, matname, perturb=True)
    spread = lambda a, b: float(np.abs(a - b).max()) / MARGIN
    return spread(base.x, moved.x), spread(base.v, moved.v), spread(base.eqps, moved.eqps) + STEPS * 2.0 * rr.SOLVER_XTOL


# ---- the runs of the E* test: 200 steps on cube_p2 -------------------------------------------------------------------------
# name -> (material, viscosity, what moves).  The bar of a run is 8 x the largest |E*_n - E*_0| the float64 restatement shows
# on the same input (E_DRIFT_MEASURED, printed by tests/test_explicit_cpu.py::test_e_star_drift_of_the_restatement; the GPU
# test takes the figure from the restatement itself, at the steps it samples).
E_CASE, E_STEPS, E_DT, E_V_SCALE, E_EVERY = "cube_p2", 200, 1e-3, 2.0, 20
E_VISCOSITY, E_PENALTY, E_GAP, E_CV, E_PRESSURE = 0.05, 1.0e4, 0.002, 0.4, 60.0
E_RUNS = {"neohook": ("neohook", None, "clamped"), "j2": ("j2", None, "clamped"), "j2_viscous": ("j2", E_VISCOSITY, "clamped"),
          "contact": ("neohook", None, "contact"), "pressure": ("neohook", None, "pressure"),
          "constant_velocity": ("neohook", None, "cv"), "friction": ("neohook", None, "contact")}
E_FRICTION = {"friction": 0.3}              # run -> mu on the plane of the contact run (the tangential penalty: E_PENALTY)
E_DRIFT_MEASURED = {"neohook": 2.66e-15, "j2": 1.78e-15, "j2_viscous": 1.78e-15, "contact": 1.78e-15, "pressure": 2.66e-15,
                    "constant_velocity": 5.33e-15, "friction": 4.44e-15}


def e_plane(P):
    """a rigid plane just above the top face, facing down"""
    top = float(P.ctrl[:, P.dim - 1].max())
    return dict(kind="plane", point=[0.0] * (P.dim - 1) + [top + E_GAP], normal=[0.0] * (P.dim - 1) + [-1.0])


def e_configure(run):
    """the boundary conditions of a run, for `facade`"""
    what = E_RUNS[run][2]

    def configure(bc):
        from mimi_amd.integrators import RigidPlane
        for c in range(3):
            bc.initial.dirichlet(0, c)
        if what == "contact":
            b = e_plane(oracle_patch(E_CASE))
            kw = dict(friction=E_FRICTION[run]) if run in E_FRICTION else {}
            bc.current.contact(1, RigidPlane(b["point"], b["normal"], E_PENALTY, **kw))
        if what == "cv":
            bc.initial.constant_velocity(1, 2, E_CV)
        if what == "pressure":
            bc.initial.pressure(1, E_PRESSURE)
    return configure


def e_initial_velocity(P, run):
    v = synthetic_u(P, scale=E_V_SCALE, seed=20241008, clamp_axis=P.dim - 1).reshape(-1, P.dim).copy()
    if E_RUNS[run][2] == "contact":
        v[:, P.dim - 1] += 3.0 * P.ctrl[:, P.dim - 1]              # upwards, into the plane
    return v.reshape(-1)


@functools.lru_cache(maxsize=None)
def e_reference(run):
    """the E* series of the float64 restatement at steps 0, E_EVERY, 2 E_EVERY, ..., its energies at the end, the largest
    |E*_n - E*_0| over ALL steps (drift) and the largest |(KE + W_int - W_ext)_n - (KE + W_int - W_ext)_0| over all steps (band);
    for a run of E_FRICTION also `counts`, (sticking points, slipping points, kink margin) of the force evaluation at the
    sampled steps, and `rough`, the contact with its evaluation log"""
    import scipy.sparse as sp
    from oracle import harness as hz, ref_path as rp
    matname, viscosity, what = E_RUNS[run]
    P = oracle_patch(E_CASE)
    D = rp.DomainOracle(P, material_pair(matname)[0])
    D.set_dt(E_DT)
    n = P.n_vdofs
    contact = rp.ContactOracle(P, P.dim - 1, 1, e_plane(P), penalty=E_PENALTY) if what == "contact" else None
    rough = None
    if run in E_FRICTION:
        # domain + RoughContact (tests/_friction_stepping.py: long double, rounded to float64 on output), committed with the
        # domain after every step and not at the start, as explicit_steps does
        import _friction_stepping as fs
        contact = rough = fs.RoughContact(P, P.dim - 1, 1, e_plane(P), E_PENALTY, E_FRICTION[run], E_PENALTY)

    face = None
    if what == "pressure":
        # the follower pressure on the top face, from the long-double face reference of tests/_face_reference.py
        import _face_reference as fr
        B = facade(E_CASE, "neohook", setup=False).patch()
        face = fr.face_basis(tuple(B.degrees), [np.asarray(k, dtype=np.float64) for k in B.knots], P.dim - 1, 1)

    def force(x):
        r = np.zeros(n)
        D.add_domain_residual(x, r)
        if contact is not None:
            contact.add_boundary_residual(x, r)
        if face is not None:
            pts = fr.face_points(face, P.ctrl + x.reshape(-1, P.dim))
            r += np.asarray(fr.follower_pressure(pts, E_PRESSURE, with_tangent=False).r, dtype=np.float64)
        return r

    damping = None
    if viscosity:
        C = sp.csr_matrix((hz.assemble_viscosity(P, D.tables, viscosity, D.rowptr, D.col), D.col, D.rowptr), shape=(n, n))
        damping = lambda v: C @ v
    fixed, pres, vbar = clamped_bottom(P), None, None
    if what == "cv":
        pres, vbar = np.zeros(n, dtype=bool), np.zeros(n)
        top = P.boundary_nodes(P.dim - 1, 1) * P.dim + (P.dim - 1)
        pres[top], vbar[top] = True, E_CV
    def commit(x):
        D.domain_post_time_advance(x)
        if rough is not None:
            rough.post_time_advance(x)

    s = er.Stepper(lumped_mass(P, D), fixed, pres, vbar).start(np.zeros(n), e_initial_velocity(P, run), None, force, damping,
                                                              commit=commit)
    counts = []
    e0 = s.energies(E_DT)
    series, worst, scale = [e0["E_star"]], 0.0, abs(e0["KE"])
    total = lambda en: en["KE"] + en["W_int"] - en["W_ext"]
    band = 0.0
    for k in range(1, E_STEPS + 1):
        s.step(E_DT)
        e = s.energies(E_DT)
        worst = max(worst, abs(e["E_star"] - e0["E_star"]))
        band = max(band, abs(total(e) - total(e0)))
        scale = max(scale, abs(e["KE"]), abs(e["W_int"]), abs(e["W_ext"]), abs(e["W_damp"]))
        if k % E_EVERY == 0:
            series.append(e["E_star"])
            if rough is not None:
                # (stick, slip, kink margin) of the step's evaluation
                counts.append((rough.n_stick, rough.n_slip, rough.log[-1]["kink"]))
    return types.SimpleNamespace(series=np.array(series), last=e, first=e0, drift=worst, scale=scale, eqps_max=float(D.eqps.max()),
                                 x=s.x.copy(), band=band, counts=counts, rough=rough)


# ---- examples/explicit_impact.py: the float64 restatement on the example's input ---------------------------------------------
# the free 5 x 1 J2 bar (balken.mesh, degree 2, 8 x 8 elements) flying at EX_VELOCITY into the oracle's rigid plane.  The bar of
# the example's E* is the bar of the E* test: 8 x the restatement's own largest |E*_n - E*_0| on that input.  The example takes
# its step from stable_time_step on the device; EX_DRIFT_MEASURED is the figure at the step the same iteration gives in numpy
# (`example_dt`), the GPU test runs the restatement at the device's own step.
EX_LENGTH, EX_GAP, EX_PENALTY, EX_VELOCITY, EX_STEPS, EX_EVERY = 5.0, 0.01, 1.0e4, 5.0, 40, 10
EX_DRIFT_MEASURED = 2.13e-14          # at dt = example_dt() = 1.9243916e-03, energy scale 62.5 (tests/test_explicit_cpu.py prints it)


@functools.lru_cache(maxsize=None)
def example_patch():
    import mimi_amd as mimi
    from oracle import iga
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(MESHES, "balken.mesh"))
    nl.elevate_degrees(1)
    nl.subdivide(3)
    B = nl.patch()
    return iga.Patch(list(B.degrees), [np.asarray(k, dtype=np.float64) for k in B.knots], np.asarray(B.control_points, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def example_dt():
    """0.9 x the body's limit by the iteration of stable_time_step (its defaults), in numpy on the oracle's tangent at rest"""
    import scipy.sparse as sp
    from mimi_amd import explicit
    from oracle import ref_path as rp
    P = example_patch()
    D = rp.DomainOracle(P, material_pair("j2")[0])
    n = P.n_vdofs
    r, A = np.zeros(n), np.zeros(D.nnz)
    D.add_domain_residual_and_grad(np.zeros(n), 1.0, r, A, rp.TANGENT_EXACT)
    K = sp.csr_matrix((A, D.col, D.rowptr), shape=(n, n))
    lam, _ = explicit.power_lambda_max(lambda z: K @ z, lumped_mass(P, D), np.ones(n), explicit.power_start(n), 1e-3, 500)
    return explicit.stable_step_from(lam, 0.0, 0.9)


@functools.lru_cache(maxsize=None)
def example_reference(dt, steps=EX_STEPS, every=EX_EVERY):
    from oracle import ref_path as rp
    P = example_patch()
    D = rp.DomainOracle(P, material_pair("j2")[0])
    D.set_dt(dt)
    n = P.n_vdofs
    wall = rp.ContactOracle(P, 0, 1, dict(kind="plane", point=[EX_LENGTH + EX_GAP, 0.0], normal=[-1.0, 0.0]), penalty=EX_PENALTY)

    def force(x):
        r = np.zeros(n)
        D.add_domain_residual(x, r)
        wall.add_boundary_residual(x, r)
        return r

    v0 = np.zeros((P.n_nodes, 2))
    v0[:, 0] = EX_VELOCITY
    s = er.Stepper(lumped_mass(P, D)).start(np.zeros(n), v0.ravel(), None, force, commit=D.domain_post_time_advance)
    e0 = s.energies(dt)
    worst, series = 0.0, [e0]
    for k in range(1, steps + 1):
        s.step(dt)
        e = s.energies(dt)
        worst = max(worst, abs(e["E_star"] - e0["E_star"]))
        if k % every == 0:
            series.append(e)
    return types.SimpleNamespace(drift=worst, series=series, eqps=D.eqps.copy(), x=s.x.copy())


# ---- the consistent-mass route: five steps on col8_p2 ---------------------------------------------------------------------------
# (rho M + dt/2 eta C) a = f - r - eta C v_{n+1/2} with the oracle's matrices, the bottom eliminated (identity rows), solved by
# scipy's LU: the reference.  The device solves by conjugate gradients to rel 1e-8, so its own bar has to hold what that stop
# rule permits: the second run of the derivation moves every residual entry by the residual's bar AND solves with the restated CG
# (tests/_kronecker_reference.py: cg, the stop rule of oracle/krylov.py: cg, with mimi_amd.kronecker's operator as preconditioner);
# spread / MARGIN as for the lumped step.  The unperturbed CG run gives the iteration counts the device must reproduce.
# Its own step and velocity scale: the inverse of the consistent mass amplifies a random-sign residual perturbation about a
# hundredfold against the lumped one, and at DT / V_SCALE the J2 run's bar of x is 1.07e-8 max|x| -- ill-conditioned by the
# rule above.  The bar relative to max|x| goes as (time / velocity); a fifth of the step at five times the velocity keeps the
# displacements (and the yielding) and brings it under 1e-9.
CM_CASE, CM_DT, CM_V_SCALE = "col8_p2", 2e-5, 300.0
CM_RUNS = {"neohook": ("neohook", None), "j2_viscous": ("j2", E_VISCOSITY)}
# run -> (bar of x / max|x|, bar of v / max|v|, CG iterations of the six solves)
CM_MEASURED = {"neohook": (5.00e-12, 1.56e-11, [0, 7, 7, 7, 7, 7]),          # |x| 9.345e-02
               "j2_viscous": (4.28e-10, 9.15e-10, [7, 7, 7, 7, 7, 7])}       # |x| 9.344e-02, eqps max 9.03e-02


def cm_initial_velocity(P):
    return initial_velocity(P) * (CM_V_SCALE / V_SCALE)


def cm_run(run, solver="lu", perturb=False, steps=STEPS, dt=CM_DT):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import _kronecker_reference as kr
    from mimi_amd.kronecker import KroneckerOperator, stiffness_coefficients
    from oracle import harness as hz, ref_path as rp
    matname, eta = CM_RUNS[run]
    P = oracle_patch(CM_CASE)
    om, pm = material_pair(matname)
    D = rp.DomainOracle(P, om)
    D.set_dt(dt)
    n, dim = P.n_vdofs, P.dim
    fixed = clamped_bottom(P)
    ess = np.flatnonzero(fixed)
    csr = lambda vals: sp.csr_matrix((vals, D.col, D.rowptr), shape=(n, n))
    M = csr(hz.assemble_mass(P, D.tables, RHO, D.rowptr, D.col))
    C = csr(hz.assemble_viscosity(P, D.tables, eta, D.rowptr, D.col)) if eta else None
    keep = sp.diags((~fixed).astype(float))
    op = KroneckerOperator(_dc.product_patch(CM_CASE), ess, dim)
    rng = np.random.default_rng(77)
    iterations = []

    def solve(fac1, b):
        A = M + fac1 * C if eta else M
        A = (keep @ A @ keep + sp.diags(fixed.astype(float))).tocsc()
        b = np.where(fixed, 0.0, b)
        if solver == "lu":
            return spla.splu(A).solve(b)
        stiff = stiffness_coefficients(pm.lambda_, pm.mu, 0.0, fac1, eta or -1.0, dim)
        s = kr.cg(A.tocsr(), b, lambda v: op.apply(v, RHO, stiff))
        assert s[3], "the restated CG did not converge"
        iterations.append(s[1])
        return s[0]

    def rhs(x, v):
        r = np.zeros(n)
        D.add_domain_residual(x, r)
        if perturb:
            r = r + _residual_perturbation(P, D, matname, r, x, rng)
        return -r - (C @ v if eta else 0.0)

    x, v = np.zeros(n), np.where(fixed, 0.0, cm_initial_velocity(P))
    a = solve(0.0, rhs(x, v))
    for _ in range(steps):
        v = v + (0.5 * dt) * a
        x = x + dt * v
        a = solve(0.5 * dt, rhs(x, v))
        v = v + (0.5 * dt) * a
        D.domain_post_time_advance(x)
    return types.SimpleNamespace(x=x, v=v, a=a, eqps=D.eqps.copy(), iterations=iterations)


@functools.lru_cache(maxsize=None)
def cm_reference(run):
    """(the LU run, the restated-CG run with its iteration counts, bar of x, bar of v, bar of eqps)"""
    lu, cg, moved = cm_run(run), cm_run(run, solver="cg"), cm_run(run, solver="cg", perturb=True)
    spread = lambda a, b: float(np.abs(a - b).max()) / MARGIN
    return lu, cg, spread(lu.x, moved.x), spread(lu.v, moved.v), spread(lu.eqps, moved.eqps) + STEPS * 2.0 * rr.SOLVER_XTOL
