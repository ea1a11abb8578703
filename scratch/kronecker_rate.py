"""The Kronecker preconditioner (csrc/kronecker.hpp) against the reference's Jacobi on the north-star block
through the facade: 128 x 128 x 16 degree-2 elements of side 1 / 64 (the cell of scratch/facade_newton.py's cube), neo-Hookean,
one face clamped, a body force, the facade's own set-up.  For the flag off and on, at the facade's fac0 (dt = 0.01) and at
ten times that (dt x sqrt 10), two implicit steps each; of the second one (the first also makes the explicit mass solve,
whose conjugate-gradient iterations are printed): Newton iterations, GMRES iterations per Newton iteration, milliseconds per
Newton iteration and in its linear solves.  Then one preconditioner application beside one matrix-vector product.

    python scratch/kronecker_rate.py [128x128x16]
    rocprofv3 --kernel-trace --stats -- python scratch/kronecker_rate.py 128x128x16 passes      (the six passes of 50
                                                      applications alone, on a diagonal pattern: which pass takes what)

Runs on a commit without the preconditioner too (the flag-on rows are left out), so that the parent can be measured with
the same script on the same machine."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mimi_amd as mimi
from mimi_amd.linear import LinearSolver

n_el = tuple(int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "128x128x16").split("x"))
HAVE = hasattr(LinearSolver, "SetKronecker")
CELL = 1.0 / 64


def facade(kronecker, dt):
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "cube-nurbs.mesh"))      # the faces and boundary ids of a box
    nl.elevate_degrees(1)
    block = mimi.BSplinePatch.block(n_el, 2, lengths=[m * CELL for m in n_el])
    nl.patch = lambda: block
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.viscosity = -1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    rc.set_int("use_iterative_solver", 1)
    rc.set_int("use_kronecker_preconditioner", 1 if kronecker else 0)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, -0.5)
    nl.boundary_condition = bc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-10, 1e-8, 10, False)
    nl.time_step_size = dt
    return nl


def one_step(kronecker, dt):
    nl = facade(kronecker, dt)
    solves = []
    cg = nl.linear_.MultCG

    def counted_cg(*args, **kw):
        out = cg(*args, **kw)
        nl.mass_cg_iterations_ = nl.linear_.final_iter_
        return out
    nl.linear_.MultCG = counted_cg
    mult = nl.linear_.Mult

    def timed(*args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mult(*args)
        torch.cuda.synchronize()
        solves.append((time.perf_counter() - t0, nl.linear_.final_iter_, nl.linear_.converged_))
        return out
    nl.linear_.Mult = timed
    nl.step_time2()
    first = len(solves)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nl.step_time2()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    solves = solves[first:]
    h = nl.newton_history[-1]
    newton = max(h["iterations"], 1)
    row = dict(kronecker=bool(kronecker), dt=dt, fac0=nl._fac0, vdofs=len(nl.x), newton_iterations=h["iterations"],
               newton_converged=h["converged"], gmres_iterations=[s[1] for s in solves], gmres_converged=all(s[2] for s in solves),
               gmres_iterations_per_newton=sum(s[1] for s in solves) / newton,
               ms_per_newton_iteration=seconds * 1e3 / newton, solve_ms_per_newton_iteration=sum(s[0] for s in solves) * 1e3 / newton,
               max_displacement=float(np.abs(nl.x).max()), mass_solve_cg_iterations=nl.mass_cg_iterations_)
    return nl, row


def per_call_ms(f, reps=50):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


if sys.argv[2:] == ["passes"]:
    from mimi_amd.integrators import CSRPattern
    from mimi_amd.kronecker import KroneckerOperator, stiffness_coefficients
    block = mimi.BSplinePatch.block(n_el, 2, lengths=[m * CELL for m in n_el])
    n = block.n_vdofs
    ess = np.sort(np.concatenate([block.boundary_nodes(0, 0) * 3 + c for c in range(3)])).astype(np.int64)
    S = LinearSolver(CSRPattern(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), n), ess)
    S.SetKronecker(KroneckerOperator(block, ess, 3))
    S.SetKroneckerCoefficients(1.0, stiffness_coefficients(1211.5, 807.7, 2.96e-5))
    r = torch.randn(n, dtype=torch.float64, device=torch.device("cuda", 0))
    z = torch.zeros_like(r)
    print(json.dumps(dict(elements=list(n_el), kronecker_application_ms=per_call_ms(lambda: S.ApplyPreconditioner(2, None, r, z)))))
    sys.exit(0)

out = dict(elements=list(n_el), have_kronecker=HAVE, rows=[])
nl = None
for dt in (0.01, 0.01 * np.sqrt(10.0)):
    for kronecker in ((0, 1) if HAVE else (0,)):
        nl = None                       # one facade's matrices in HBM at a time
        nl, row = one_step(kronecker, dt)
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
# one application beside one product, on the last facade's handle and Jacobian
S, A = nl.linear_, nl.d_jac_
r = torch.randn(len(nl.x), dtype=torch.float64, device=A.device)
z = torch.zeros_like(r)
out["product_ms"] = per_call_ms(lambda: S.AddMult(A, r, z))
if HAVE:
    out["kronecker_application_ms"] = per_call_ms(lambda: S.ApplyPreconditioner(2, None, r, z))
    out["jacobi_application_ms"] = per_call_ms(lambda: S.ApplyPreconditioner(1, A, r, z))
print(json.dumps({k: v for k, v in out.items() if k != "rows"}), flush=True)
