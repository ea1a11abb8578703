"""The matrix-free action of the contact tangent (csrc/kernels_face_action.hpp) against the assembled Jacobian on
BASELINE configuration 4 through the facade: 96 x 96 x 12 degree-2 elements of side 1 / 64, one face clamped, a body force, the
rigid sphere of bench.py's cfg4 (radius a quarter of the block's length, pressed 10 % of its radius into the top face: 9 216
contact faces of 9 nodes and 16 points), the iterative route with the Kronecker preconditioner.  Per route, of the second
implicit step: Newton iterations, GMRES iterations per Newton iteration, milliseconds per Newton iteration, the device
memory in use at the end (the peak: nothing is returned), and per call, device-synchronised and warmed: the contact action
beside the domain action, the contact linearisation, and the assembled contact residual + tangent.

    python scratch/boundary_action_rate.py                 both routes, each in a process of its own under its own time limit,
                                                           into profiles/boundary_action_rate.txt
    python scratch/boundary_action_rate.py one FLAG        one route, one JSON line (FLAG 1: matrix_free + matrix_free_boundary)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL = 1.0 / 64
N_EL = (96, 96, 12)
PENALTY = 1.0e2      # (the frozen-pressure Newton iteration contracts only for a penalty small beside the body's stiffness)
LIMIT = 300          # seconds per route


def one(flag):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import mimi_amd as mimi
    from mimi_amd.integrators import RigidSphere
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "cube-nurbs.mesh"))      # the faces and boundary ids of a box
    nl.elevate_degrees(1)
    L = [m * CELL for m in N_EL]
    block = mimi.BSplinePatch.block(N_EL, 2, lengths=L)
    nl.patch = lambda: block
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density, mat.viscosity = 1, -1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    rc.set_int("use_iterative_solver", 1)
    rc.set_int("use_kronecker_preconditioner", 1)
    if flag:
        rc.set_int("matrix_free", 1)
        rc.set_int("matrix_free_boundary", 1)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, -0.5)
    top = [a - 1 for a, f in nl._faces.items() if f == (2, 1)][0]
    R = 0.25 * L[0]
    bc.current.contact(top, RigidSphere([0.5 * L[0], 0.5 * L[1], L[2] + 0.9 * R], R, PENALTY))
    nl.boundary_condition = bc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-10, 1e-8, 10, False)
    nl.time_step_size = 0.01
    solves = []
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
    free_b, total_b = torch.cuda.mem_get_info()
    c = nl.contacts_[0]
    c.BoundaryPostTimeAdvance(nl.x)
    row = dict(matrix_free=bool(flag), vdofs=len(nl.x), nnz=int(nl.pattern_.nnz), contact_faces=c.n_marked_boundaries_,
               newton_iterations=h["iterations"], newton_converged=h["converged"], gmres_iterations=[s[1] for s in solves],
               gmres_converged=all(s[2] for s in solves), gmres_iterations_per_newton=sum(s[1] for s in solves) / newton,
               ms_per_newton_iteration=seconds * 1e3 / newton, solve_ms_per_newton_iteration=sum(s[0] for s in solves) * 1e3 / newton,
               device_memory_gb=(total_b - free_b) / 1e9, max_displacement=float(np.abs(nl.x).max()),
               contact_pressure_integral=float(c.last_pressure_), active_nodes=int((c.AveragePressure() != 0).sum()))

    def per_call_ms(f, reps=200):
        for _ in range(10):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    r = torch.randn(len(nl.x), dtype=torch.float64, device=torch.device("cuda", 0))
    z = torch.zeros_like(r)
    c.Linearize(nl.d_x_)
    nl.domain_.Linearize(nl.d_x_)
    row["contact_action_ms"] = per_call_ms(lambda: c.ApplyTangent(r, z, nl._fac0))
    row["contact_linearize_ms"] = per_call_ms(lambda: c.Linearize(nl.d_x_))
    row["contact_record_mb"] = c.LinearizationBytes() / 1e6
    row["domain_action_ms"] = per_call_ms(lambda: nl.domain_.ApplyTangent(r, z, stiffness=nl._fac0, density=1.0), reps=50)
    row["contact_residual_ms"] = per_call_ms(lambda: c.AddBoundaryResidual(nl.d_x_, z))
    row["tangent_blocks_before_assembly"] = c.HoldsTangentBlocks()
    # the sphere touches few of the 9 216 faces; a uniform follower pressure on the same face makes every face active
    from mimi_amd.integrators import FollowerPressure
    fp = FollowerPressure("pressure", nl.pattern_u_, block, 2, 1).Prepare()
    fp.SetPressure(1.0)
    fp.Linearize(nl.d_x_)
    row["contact_active_faces"] = int(np.count_nonzero((c.AveragePressure()[np.searchsorted(c.MarkedNodes(), nl.contacts_[0]._keep[0])] != 0).any(axis=1)))
    row["all_faces_active_action_ms"] = per_call_ms(lambda: fp.ApplyTangent(r, z, nl._fac0))
    row["all_faces_active_linearize_ms"] = per_call_ms(lambda: fp.Linearize(nl.d_x_))
    z.zero_()
    row["all_faces_active_residual_ms"] = per_call_ms(lambda: fp.AddBoundaryResidual(nl.d_x_, z))
    if not flag:
        a = torch.zeros_like(nl.d_jac_)
        row["all_faces_active_residual_and_tangent_ms"] = per_call_ms(lambda: fp.AddBoundaryResidualAndGrad(nl.d_x_, nl._fac0, z, a))
    if not flag:
        row["contact_residual_and_tangent_ms"] = per_call_ms(lambda: c.AddBoundaryResidualAndGrad(nl.d_x_, nl._fac0, z, nl.d_jac_))
    print(json.dumps(row), flush=True)


def table():
    out_path = os.path.join(ROOT, "profiles", "boundary_action_rate.txt")
    lines = ["scratch/boundary_action_rate.py on one MI355X: configuration 4 with the contact tangent as an action and assembled,",
             "each route in a process of its own.  Figures of the second implicit step; per-call times device-synchronised, warmed."]
    for label, flag in (("matrix_free + matrix_free_boundary", 1), ("assembled", 0)):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "one", str(flag)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        rows = [l for l in p.stdout.splitlines() if l.startswith("{")]
        lines.append(f"-- {label} --")
        lines += rows if rows else [f"(no result: exit status {p.returncode})"] + p.stderr.splitlines()[-5:]
        print("\n".join(lines[-1 - max(len(rows), 1):]), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
        if p.returncode != 0:
            # a route that failed, faulted or ran out of time ends the table: nothing more is started on the card
            return p.returncode
    return 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["one"]:
        one(int(sys.argv[2]))
    else:
        sys.exit(table())
