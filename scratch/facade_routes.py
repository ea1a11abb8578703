#!/usr/bin/env python3
"""Same library calls, same bits: every assembly and solver route of the facade (mimi_amd/solid.py, mimi_amd/explicit.py) at
the smallest shapes the tests use, for comparing two versions of the facade's Python over ONE built library across a refactor
of the facade.

  MIMI_HIP_LIBRARY=mimi_amd/lib/libmimi_hip.so python scratch/facade_routes.py [--package DIR] > hashes.txt
        one line per result: route, what, SHA-256 of the bytes (norms, energies and the stable step in hex, iteration counts
        as they are); --package DIR: import mimi_amd from DIR (a copy of another revision's mimi_amd/*.py) instead of the tree
  python scratch/facade_routes.py --compare A.txt B.txt

Cases: sq_p2 and cube_p2 of tests/_explicit_cases.py (the bottom clamped, a body force, the pair = attributes 3 and 5 of the
cube), the golden beam with the contact plane of tests/test_boundary_action_gpu.py; three steps each.  Routes: direct, iterative
with Jacobi, Kronecker, matrix-free, each with and without the pair; contact and pressure, assembled and as actions; viscosity;
constant velocity; host set-up; a quadrature order of the caller's (the temporary forms handle); set_body_force between steps;
the fixed-point entries with a coupling surface; nodal fields; explicit lumped (pair, viscosity, contact, pressure, constant
velocity, save cadence), stable_time_step, explicit consistent mass.  The direct-solve lines are the machine's SciPy's: compare
on one machine."""
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package" in sys.argv:
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--package") + 1]))
sys.path[1:1] = [ROOT, os.path.join(ROOT, "tests")]

BODY, DT = -40.0, 0.05
ITERATIVE = (("use_iterative_solver", 1),)
KRONECKER = ITERATIVE + (("use_kronecker_preconditioner", 1),)
PERIODIC = KRONECKER + (("periodic_iterative", 1),)
MATRIX_FREE = (("matrix_free", 1),)
ACTIONS = MATRIX_FREE + (("matrix_free_boundary", 1),)
EXPLICIT = (("explicit_dynamics", 1),)


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def out(route, what, value):
    print(f"{route:44s} {what:22s} {value}", flush=True)


def configure(dim, pair=False, body=True, mark=None):
    def f(bc):
        for c in range(dim):
            bc.initial.dirichlet(0, c)
        if body:
            bc.initial.body_force(dim - 1, BODY)
        if pair:
            bc.initial.periodic(3, 5)
        if mark:
            mark(bc)
    return f


def count_solves(nl):
    """the iteration counts of every GMRES / CG solve, through wrappers on the solver (looked up at call time)"""
    counts = []
    for name in ("Mult", "MultCG"):
        def counted(*args, _f=getattr(nl.linear_, name), _name=name, **kw):
            r = _f(*args, **kw)
            counts.append(f"{_name}:{nl.linear_.final_iter_}")
            return r
        setattr(nl.linear_, name, counted)
    return counts


def report(route, nl, counts):
    out(route, "rhs", sha(nl.rhs_))
    out(route, "newton", " ".join(f"{h['iterations']}:{float(h['norm']).hex()}:{float(h['norm0']).hex()}:{int(h['converged'])}"
                                  for h in nl.newton_history))
    out(route, "krylov", " ".join(counts) or "-")
    out(route, "von_mises nodes", sha(nl.field("von_mises_stress")))
    for k, c in enumerate(nl.contacts_):
        out(route, f"contact {k} force", sha(c.last_force_))


def implicit(route, nl, steps=3, between=None, step=None):
    counts = count_solves(nl)
    for k in range(steps):
        (step or type(nl).step_time2)(nl)
        out(route, f"x step {k + 1}", sha(nl.x))
        out(route, f"x_dot step {k + 1}", sha(nl.x_dot))
        if between:
            between(nl, k)
    report(route, nl, counts)


def solid(case, flags=(), matname="neohook", viscosity=None, **kw):
    import _explicit_cases as ec
    dim = 2 if case == "sq_p2" else 3
    nl = ec.facade(case, matname, flags=flags, configure=configure(dim, **kw), viscosity=viscosity)
    nl.configure_newton("nonlinear_solid", 1e-12, 1e-10, 20, False)
    nl.time_step_size = DT
    return nl


def beam(flags, mark):
    import test_boundary_action_gpu as tb
    return tb._beam(list(flags), mark)


def run_implicit():
    import numpy as np
    import test_boundary_action_gpu as tb
    pressure = lambda bc: bc.initial.pressure(1, 30.0)
    # assembled routes
    implicit("direct sq_p2", solid("sq_p2"))
    implicit("direct cube_p2", solid("cube_p2"))
    implicit("direct cube_p2 j2", solid("cube_p2", matname="j2"))
    implicit("direct cube_p2 pair", solid("cube_p2", pair=True))
    implicit("direct cube_p2 pair j2", solid("cube_p2", matname="j2", pair=True))
    implicit("jacobi sq_p2", solid("sq_p2", ITERATIVE))
    implicit("jacobi cube_p2", solid("cube_p2", ITERATIVE))
    implicit("jacobi cube_p2 pair", solid("cube_p2", ITERATIVE, pair=True))
    implicit("kronecker cube_p2", solid("cube_p2", KRONECKER))
    implicit("kronecker cube_p2 pair", solid("cube_p2", PERIODIC, pair=True))
    implicit("direct cube_p2 pressure", solid("cube_p2", mark=pressure))
    implicit("kronecker cube_p2 pair pressure", solid("cube_p2", PERIODIC, pair=True, mark=pressure))
    implicit("direct beam contact", beam((), tb._mark_contact))
    implicit("kronecker beam contact", beam(tb.ASSEMBLED, tb._mark_contact))
    # matrix-free routes
    implicit("matrix-free sq_p2", solid("sq_p2", KRONECKER + MATRIX_FREE))
    implicit("matrix-free cube_p2", solid("cube_p2", KRONECKER + MATRIX_FREE))
    implicit("matrix-free cube_p2 pair", solid("cube_p2", PERIODIC + MATRIX_FREE, pair=True))
    implicit("actions cube_p2 pressure", solid("cube_p2", KRONECKER + ACTIONS, mark=pressure))
    implicit("actions beam contact", beam(tb.MATRIX_FREE, tb._mark_contact))
    implicit("actions cube_p2 pair pressure", solid("cube_p2", PERIODIC + ACTIONS, pair=True, mark=pressure))
    # material, load and set-up variants
    implicit("direct cube_p2 viscous", solid("cube_p2", viscosity=0.05))
    implicit("direct cube_p2 pair viscous", solid("cube_p2", viscosity=0.05, pair=True))
    implicit("matrix-free cube_p2 viscous", solid("cube_p2", KRONECKER + MATRIX_FREE, viscosity=0.05))
    implicit("matrix-free cube_p2 pair viscous", solid("cube_p2", PERIODIC + MATRIX_FREE, viscosity=0.05, pair=True))
    velocity = lambda bc: bc.initial.constant_velocity(1, 2, 0.4)
    implicit("direct cube_p2 velocity", solid("cube_p2", mark=velocity))
    implicit("kronecker cube_p2 pair velocity", solid("cube_p2", PERIODIC, pair=True, mark=velocity))
    traction = lambda bc: bc.initial.traction(1, 0, 7.0)
    for pair in (False, True):
        tag = " pair" if pair else ""
        implicit("host set-up cube_p2" + tag, solid("cube_p2", (("host_setup", 1),), viscosity=0.05, pair=pair, mark=traction))
        implicit("device set-up cube_p2 traction" + tag, solid("cube_p2", viscosity=0.05, pair=pair, mark=traction))
        implicit("quadrature order cube_p2" + tag, solid("cube_p2", (("nonlinear_solid_quadrature_order", 5),), viscosity=0.05, pair=pair))
        implicit("set_body_force cube_p2" + tag, solid("cube_p2", (("nonlinear_solid_quadrature_order", 5),), pair=pair),
                 between=lambda nl, k: nl.set_body_force(0, 9.0 * (k + 1)))
        implicit("set_body_force jacobi cube_p2" + tag, solid("cube_p2", ITERATIVE, pair=pair, body=False),
                 between=lambda nl, k: nl.set_body_force(2, -11.0 * (k + 1)))

    # the fixed-point entries with a coupling surface on the top: two solves per step, the traction following the iterate
    def coupled_step(nl):
        s = nl.coupling_surface(1)
        t = np.zeros((s.n_points_, 3))
        for it in range(2):
            t[:, 2] = -5.0 * (it + 1)
            s.set_traction(t, None if it == 0 else nl.fixed_point_advance2()[0].reshape(-1))
            nl.fixed_point_solve2()
            xa, va = nl.fixed_point_advance2()
            out(nl.route_name, "advanced x", sha(xa))
            out(nl.route_name, "advanced v", sha(va))
        nl.advance_time2()
    for name, flags, pair in (("fixed-point direct cube_p2", (), False), ("fixed-point direct cube_p2 pair", (), True),
                              ("fixed-point matrix-free cube_p2 pair", PERIODIC + MATRIX_FREE, True)):
        nl = solid("cube_p2", flags, pair=pair)
        nl.route_name = name
        implicit(name, nl, step=coupled_step)
    # fields on a given displacement, at points and nodes
    for pair in (False, True):
        nl = solid("cube_p2", matname="j2", pair=pair)
        nl.step_time2()
        u = 0.5 * nl.x
        for name in ("von_mises_stress", "cauchy_stress", "accumulated_plastic_strain"):
            out("fields cube_p2 j2" + (" pair" if pair else ""), name[:12] + " nodes", sha(nl.field(name, u=u)))
            out("fields cube_p2 j2" + (" pair" if pair else ""), name[:12] + " points", sha(nl.field(name, where="points", u=u)))


def run_explicit():
    import numpy as np
    import _explicit_cases as ec

    def start(nl, dt=ec.DT, scale=2.0):
        v = scale * np.random.default_rng(3).standard_normal(nl.x.size)
        v[nl.dirichlet_] = 0.0
        nl.solution_view("displacement", "x_dot")[:] = v
        nl.time_step_size = dt
        return nl

    def explicit(route, nl, chunks=(1, 1, 1), energies=True):
        done = 0
        for n in chunks:
            nl.explicit_steps(n)
            done += n
            out(route, f"x step {done}", sha(nl.x))
            out(route, f"x_dot step {done}", sha(nl.x_dot))
        out(route, "acceleration", sha(nl.explicit_acceleration()))
        out(route, "d2h copies", nl.explicit_d2h_copies_)
        if energies:
            out(route, "energies", " ".join(f"{k}:{float(v).hex()}" for k, v in nl.explicit_energies().items()))
        else:
            out(route, "cg", nl.explicit_cg_iterations_)
        out(route, "von_mises nodes", sha(nl.field("von_mises_stress")))
        out(route, "time", f"{float(nl.current_time).hex()} {nl.runtime_communication.i_timestep_}")
        for k, c in enumerate(nl.contacts_):
            out(route, f"contact {k} force", sha(c.last_force_))

    facade = lambda case, pair=False, flags=(), matname="neohook", **kw: ec.facade(
        case, matname, flags=EXPLICIT + flags, configure=configure(2 if case == "sq_p2" else 3, pair=pair), **kw)
    explicit("explicit sq_p2", start(facade("sq_p2")))
    explicit("explicit cube_p2 j2", start(facade("cube_p2", matname="j2")))
    explicit("explicit cube_p2 pair", start(facade("cube_p2", pair=True)))
    explicit("explicit cube_p2 viscous", start(facade("cube_p2", viscosity=0.05)))
    explicit("explicit cube_p2 pair viscous", start(facade("cube_p2", pair=True, viscosity=0.05)))
    for run in ("contact", "pressure", "constant_velocity"):
        nl = ec.facade(ec.E_CASE, "neohook", configure=ec.e_configure(run))
        nl.solution_view("displacement", "x_dot")[:] = ec.e_initial_velocity(ec.oracle_patch(ec.E_CASE), run)
        nl.time_step_size = ec.E_DT
        explicit("explicit cube_p2 " + run, nl, chunks=(20, 20, 1))
    # the save cadence: x every 2nd step, v every 3rd, a field every 2nd, within one call and across calls
    for pair in (False, True):
        route = "explicit cube_p2 saves" + (" pair" if pair else "")
        nl = start(facade("cube_p2", pair=pair, matname="j2"))
        rc = nl.runtime_communication
        with tempfile.TemporaryDirectory() as tmp:
            rc.set_fname(os.path.join(tmp, "out.npz"))
            rc.append_should_save("x", 2)
            rc.append_should_save("v", 3)
            rc.append_should_save("von_mises_stress", 2)
            explicit(route, nl, chunks=(4, 3))
            saved = np.load(rc.fname)
            for key in sorted(saved.files):
                out(route, "saved " + key, sha(saved[key]))
    # the stable step at rest, at a given displacement and with damping
    for pair in (False, True):
        for eta in (None, 0.05):
            nl = start(facade("cube_p2", pair=pair, viscosity=eta))
            route = "stable step cube_p2" + (" pair" if pair else "") + (" viscous" if eta else "")
            out(route, "at rest", f"{float(nl.stable_time_step()).hex()} {nl.stable_iterations_}")
            nl.explicit_steps(2)
            out(route, "after 2 steps", f"{float(nl.stable_time_step()).hex()} {nl.stable_iterations_}")
            out(route, "at u", f"{float(nl.stable_time_step(u=3.0 * nl.x)).hex()} {nl.stable_iterations_}")
    # consistent mass
    consistent = (("explicit_consistent_mass", 1),)
    explicit("consistent cube_p2", start(facade("cube_p2", flags=consistent), dt=ec.CM_DT), energies=False)
    explicit("consistent cube_p2 pair", start(facade("cube_p2", pair=True, flags=consistent + (("periodic_iterative", 1),)), dt=ec.CM_DT),
             energies=False)
    explicit("consistent cube_p2 pair j2 viscous", start(facade("cube_p2", pair=True, matname="j2", viscosity=0.05,
                                                                 flags=consistent + (("periodic_iterative", 1),)), dt=ec.CM_DT), energies=False)
    # the implicit save cadence, for the order of the writes against next_time_step
    nl = solid("cube_p2", pair=True)
    rc = nl.runtime_communication
    with tempfile.TemporaryDirectory() as tmp:
        rc.set_fname(os.path.join(tmp, "out.npz"))
        rc.append_should_save("x", 1)
        rc.append_should_save("v", 2)
        rc.append_should_save("cauchy_stress", 2)
        implicit("direct cube_p2 pair saves", nl)
        saved = np.load(rc.fname)
        for key in sorted(saved.files):
            out("direct cube_p2 pair saves", "saved " + key, sha(saved[key]))


def compare(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    bad = [(x, y) for x, y in zip(la, lb) if x != y]
    for x, y in bad[:20]:
        print(f"- {x}\n+ {y}")
    print(f"{len(la)} / {len(lb)} lines, {len(bad)} differ" + ("" if len(la) == len(lb) else ": DIFFERENT LENGTHS"))
    return 1 if bad or len(la) != len(lb) or not la else 0


if __name__ == "__main__":
    if "--compare" in sys.argv:
        sys.exit(compare(*sys.argv[-2:]))
    import mimi_amd
    print("# mimi_amd from", os.path.relpath(os.path.dirname(mimi_amd.__file__), ROOT), file=sys.stderr)
    run_implicit()
    run_explicit()
