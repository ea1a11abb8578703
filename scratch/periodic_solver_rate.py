"""A periodic pair on the iterative routes on the north-star block through the facade: 128 x 128 x 16
degree-2 elements of side 1 / 64 (the block of scratch/matrix_free_rate.py), periodic along x, the face z = 0 clamped, a body
force.  Routes: "jacobi", the assembled periodic route with GMRES + Jacobi (the only iterative periodic route before
"periodic_iterative"); "kronecker", the flag with the Kronecker preconditioner on the assembled route; "matrix_free", the flag
with the matrix-free product through the fold.  Per route, of the second implicit step: Newton iterations, GMRES iterations per
Newton iteration, milliseconds per Newton iteration and in its linear solves, the device memory in use at the end (the library
returns no buffer and torch's caching allocator keeps its peak, so this is the peak), a digest of the displacement; on the
matrix-free route one folded product (LinearSolver.OperatorMult through the fold) beside one unfolded product of the same
domain handle (a solver on the unwrapped pattern).

    python scratch/periodic_solver_rate.py                     the table: every route in a process of its own, each under its
                                                               own time limit, everything into profiles/periodic_solver_rate.txt
    python scratch/periodic_solver_rate.py one ROUTE           one route, one JSON line
    MIMI_AMD_TREE=DIR MIMI_HIP_LIBRARY=LIB python scratch/periodic_solver_rate.py one jacobi     the same on another commit's
                                                               package and library (the parent has the jacobi route only)

The table runs the parent's row when PERIODIC_PARENT_TREE and PERIODIC_PARENT_LIBRARY name the parent's package directory and
library (python -m mimi_amd.build --out LIB --rev REV; git archive REV mimi_amd)."""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL = 1.0 / 64
LIMIT = 360          # seconds per route
ELEMENTS = (128, 128, 16)
ROUTES = {"jacobi": (), "kronecker": ("use_kronecker_preconditioner", "periodic_iterative"),
          "matrix_free": ("use_kronecker_preconditioner", "periodic_iterative", "matrix_free")}


def one(route):
    sys.path.insert(0, os.environ.get("MIMI_AMD_TREE") or ROOT)
    import numpy as np
    import torch
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "cube-nurbs.mesh"))      # the faces and boundary ids of a box
    nl.elevate_degrees(1)
    block = mimi.BSplinePatch.block(ELEMENTS, 2, lengths=[m * CELL for m in ELEMENTS])
    nl.patch = lambda: block
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.viscosity = -1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    rc.set_int("use_iterative_solver", 1)
    for flag in ROUTES[route]:
        rc.set_int(flag, 1)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, -0.5)
    x_faces = sorted(a for a, (axis, _) in nl._faces.items() if axis == 0)
    bc.initial.periodic(*x_faces)
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
    row = dict(route=route, package="another commit's" if os.environ.get("MIMI_AMD_TREE") else "this commit's",
               vdofs_folded=len(nl.x), vdofs_unwrapped=int(nl.patch_.n_vdofs), nnz_folded=int(nl.pattern_.nnz),
               newton_iterations=h["iterations"], newton_converged=h["converged"],
               gmres_iterations=[s[1] for s in solves], gmres_converged=all(s[2] for s in solves),
               gmres_iterations_per_newton=sum(s[1] for s in solves) / newton, ms_per_newton_iteration=seconds * 1e3 / newton,
               solve_ms_per_newton_iteration=sum(s[0] for s in solves) * 1e3 / newton,
               device_memory_gb=(total_b - free_b) / 1e9, holds_Au=hasattr(nl, "d_Au_"), holds_J=hasattr(nl, "d_jac_"),
               max_displacement=float(np.abs(nl.x).max()),
               displacement_sha1=hashlib.sha1(np.ascontiguousarray(nl.x).tobytes()).hexdigest())

    def per_call_ms(f, reps=50):
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    dev = torch.device("cuda", 0)
    r = torch.randn(len(nl.x), dtype=torch.float64, device=dev)
    z = torch.zeros_like(r)
    if route == "matrix_free":
        from mimi_amd.linear import LinearSolver
        row["folded_product_ms"] = per_call_ms(lambda: nl.linear_.OperatorMult(r, z))
        unwrapped = LinearSolver(nl.pattern_u_, None)
        unwrapped.SetOperator(nl.domain_, 1.0, nl._fac0, 0.0)
        ru = torch.randn(nl.patch_.n_vdofs, dtype=torch.float64, device=dev)
        zu = torch.zeros_like(ru)
        row["unfolded_product_ms"] = per_call_ms(lambda: unwrapped.OperatorMult(ru, zu))
    else:
        row["csr_product_ms"] = per_call_ms(lambda: nl.linear_.AddMult(nl.d_jac_, r, z))
    print(json.dumps(row), flush=True)


def table():
    out_path = os.path.join(ROOT, "profiles", "periodic_solver_rate.txt")
    parent_tree, parent_lib = os.environ.get("PERIODIC_PARENT_TREE"), os.environ.get("PERIODIC_PARENT_LIBRARY")
    lines = ["scratch/periodic_solver_rate.py on one MI355X: the parent commit's only iterative periodic route and this commit's three,",
             "one session on one machine; every route in a process of its own.  Neo-Hookean, degree 2, 128x128x16 elements, periodic",
             "along x, z = 0 clamped.  Figures of the second implicit step."]
    runs = []
    if parent_tree and parent_lib:
        runs.append(("parent commit, assembled, GMRES + Jacobi", "jacobi", dict(MIMI_AMD_TREE=parent_tree, MIMI_HIP_LIBRARY=parent_lib)))
    runs += [("this commit, assembled, GMRES + Jacobi (flag unset)", "jacobi", {}),
             ("this commit, periodic_iterative, assembled, GMRES + Kronecker", "kronecker", {}),
             ("this commit, periodic_iterative, matrix_free, GMRES + Kronecker", "matrix_free", {})]
    for label, route, env in runs:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "one", route]
        p = subprocess.run(cmd, env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        rows = [l for l in p.stdout.splitlines() if l.startswith("{")]
        lines.append(f"-- {label} --")
        lines += rows if rows else [f"(no result: exit status {p.returncode})"] + p.stderr.splitlines()[-5:]
        print("\n".join(lines[-1 - max(len(rows), 1):]), flush=True)
        with open(out_path + ".part", "w") as f:
            f.write("\n".join(lines) + "\n")
        if p.returncode != 0:
            # a route that failed, faulted or ran out of time ends the table: nothing more is started on the card
            os.replace(out_path + ".part", out_path)
            return p.returncode
    os.replace(out_path + ".part", out_path)
    return 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["one"]:
        one(sys.argv[2])
    else:
        sys.exit(table())
