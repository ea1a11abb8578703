"""The node-block diagonal of the matrix-free tangent (csrc/kernels_diagonal.hpp) and the two preconditioners built
on it, on the blocks of scratch/matrix_free_rate.py: elements of side 1 / 64, one face clamped, a body force.

    python scratch/diagonal_rate.py [table [kernel | route]]  the table (or its kernel / route rows alone): every configuration in a
                                                             process of its own, each under its own time limit, everything
                                                             into profiles/diagonal_rate.txt
    python scratch/diagonal_rate.py kernel MATERIAL DEGREE ELEMENTS          TangentDiagonal (both modes) beside ApplyTangent of
                                                             the same handle, one JSON line
    python scratch/diagonal_rate.py route MATERIAL DEGREE ELEMENTS ROUTE FORCE     the second implicit step through the facade,
                                                             one JSON line (ROUTE: assembled_jacobi | mf_jacobi | mf_block |
                                                             mf_kronecker; FORCE: the body force)

kernel: A (TangentDiagonal) and B (ApplyTangent) in ONE process, after a warm-up, in alternating batches of CALLS calls between two
events on the stream both launch on; the median over BATCHES batches of each.  The expectation of the issue: a diagonal build
costs no more than ten actions of the same handle (a Jacobi solve of the north-star block takes about 180 products)."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scratch")]
CELL = 1.0 / 64
LIMIT = 300          # seconds per configuration
CALLS, BATCHES, WARMUP = 10, 9, 5
KERNELS = [("neohook", 2, "128x128x16"), ("j2", 2, "128x128x16"), ("j2", 3, "64x64x8")]
ROUTES = ["assembled_jacobi", "mf_jacobi", "mf_block", "mf_kronecker"]
# (label, material, degree, elements, body force): the north-star block, a thin plate, J2 at the onset of yield and beyond it
FACADE = [("north-star block", "neohook", 2, "128x128x16", -0.5),
          ("thin plate", "neohook", 2, "128x128x2", -0.5),
          ("J2 at the onset of yield", "j2", 2, "64x64x8", -400.0),
          ("J2 beyond yield", "j2", 2, "64x64x8", -1000.0)]
FLAGS = {"assembled_jacobi": [], "mf_jacobi": ["matrix_free", "matrix_free_jacobi"],
         "mf_block": ["matrix_free", "use_block_jacobi_preconditioner"], "mf_kronecker": ["matrix_free", "use_kronecker_preconditioner"]}


def facade(matname, degree, elements, flags, force):
    import mimi_amd as mimi
    from matrix_free_rate import material
    n_el = tuple(int(x) for x in elements.split("x"))
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "cube-nurbs.mesh"))      # the faces and boundary ids of a box
    nl.elevate_degrees(degree - 1)
    block = mimi.BSplinePatch.block(n_el, degree, lengths=[m * CELL for m in n_el])
    nl.patch = lambda: block
    nl.set_material(material(mimi, matname))
    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    for k in ["use_iterative_solver"] + flags:
        rc.set_int(k, 1)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, force)
    nl.boundary_condition = bc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-10, 1e-8, 10, False)
    nl.time_step_size = 0.01
    return nl, n_el


def kernel(matname, degree, elements):
    import torch
    nl, n_el = facade(matname, degree, elements, FLAGS["mf_jacobi"], -0.5)
    nl.step_time2()          # (leaves a linearisation at a deformed state, and for J2 a committed one)
    G = nl.domain_
    dev = torch.device("cuda", 0)
    n = len(nl.x)
    x = torch.randn(n, dtype=torch.float64, device=dev)
    y = torch.zeros_like(x)
    d1 = torch.zeros(n, dtype=torch.float64, device=dev)
    d3 = torch.zeros(3 * n, dtype=torch.float64, device=dev)
    calls = {"action": lambda: G.ApplyTangent(x, y, stiffness=nl._fac0, density=1.0),
             "diagonal": lambda: G.TangentDiagonal(d1, stiffness=nl._fac0, density=1.0),
             "blocks": lambda: G.TangentDiagonal(d3, stiffness=nl._fac0, density=1.0, block=True)}
    for f in calls.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(BATCHES):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / CALLS)
    row = dict(material=matname, degree=degree, elements=list(n_el), vdofs=n, calls_per_batch=CALLS, batches=BATCHES)
    for k, t in times.items():
        row[f"{k}_ms_median"], row[f"{k}_ms_min"], row[f"{k}_ms_max"] = statistics.median(t), min(t), max(t)
    row["diagonal_over_action"] = row["diagonal_ms_median"] / row["action_ms_median"]
    row["blocks_over_action"] = row["blocks_ms_median"] / row["action_ms_median"]
    row["record_gb"] = G.LinearizationBytes() / 1e9
    print(json.dumps(row), flush=True)


def route(matname, degree, elements, which, force):
    import numpy as np
    import torch
    nl, n_el = facade(matname, degree, elements, FLAGS[which], force)
    nl.linear_.max_iter = 3000
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
    row = dict(route=which, material=matname, degree=degree, elements=list(n_el), body_force=force, vdofs=len(nl.x),
               newton_iterations=h["iterations"], newton_converged=h["converged"], gmres_iterations=[s[1] for s in solves],
               gmres_converged=all(s[2] for s in solves), gmres_iterations_per_newton=sum(s[1] for s in solves) / newton,
               ms_per_newton_iteration=seconds * 1e3 / newton, solve_ms_per_newton_iteration=sum(s[0] for s in solves) * 1e3 / newton,
               device_memory_gb=(total_b - free_b) / 1e9, max_displacement=float(np.abs(nl.x).max()),
               displacement_sha1=hashlib.sha1(np.ascontiguousarray(nl.x).tobytes()).hexdigest())
    if matname == "j2":
        eqps = nl.domain_.State("accumulated_plastic_strain")
        row["plastic_share"] = float((eqps > 0).mean())
    print(json.dumps(row), flush=True)


def table(only=None):
    out_path = os.path.join(ROOT, "profiles", "diagonal_rate.txt")
    lines = ["scratch/diagonal_rate.py on one MI355X, one session on one machine; every configuration in a process of its own.",
             "kernel rows: milliseconds per call, the median of 9 batches of 10 calls between two events, TangentDiagonal (diagonal /",
             "blocks) and ApplyTangent (action) alternating in one process.  route rows: figures of the second implicit step.",
             "(The assembled route's code is the parent commit's: this commit changes nothing on it.)"]
    jobs = [("kernel", f"{m} p{p} {e}", ["kernel", m, str(p), e]) for m, p, e in KERNELS]
    for label, m, p, e, force in FACADE:
        jobs += [("route", f"{label}: {m} p{p} {e}, body force {force:g}, {r}", ["route", m, str(p), e, r, str(force)]) for r in ROUTES]
    for kind, label, args in jobs:
        if only and kind != only:
            continue
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__)] + args
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        rows = [l for l in p.stdout.splitlines() if l.startswith("{")]
        lines.append(f"-- {label} --")
        lines += rows if rows else [f"(no result: exit status {p.returncode})"] + p.stderr.splitlines()[-5:]
        print("\n".join(lines[-1 - max(len(rows), 1):]), flush=True)
        with open(out_path + ".part", "w") as f:
            f.write("\n".join(lines) + "\n")
        if p.returncode != 0:
            # a configuration that failed, faulted or ran out of time ends the table: nothing more is started on the card
            os.replace(out_path + ".part", out_path)
            return p.returncode
    os.replace(out_path + ".part", out_path)
    return 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["kernel"]:
        kernel(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    elif sys.argv[1:2] == ["route"]:
        route(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5], float(sys.argv[6]))
    else:
        sys.exit(table(sys.argv[2] if sys.argv[1:2] == ["table"] and len(sys.argv) > 2 else None))
