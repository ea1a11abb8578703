"""The matrix-free tangent action (csrc/kernels_apply.hpp) against the assembled Jacobian on the north-star block
through the facade: 128 x 128 x 16 degree-2 elements of side 1 / 64 (the block of scratch/kronecker_rate.py), one face clamped,
a body force, the iterative route with the Kronecker preconditioner.  Per configuration, of the second implicit step: Newton
iterations, GMRES iterations per Newton iteration, milliseconds per Newton iteration and in its linear solves, one tangent
action beside one CSR product (AddMult), the device memory in use at the end (the library returns no buffer and torch's
caching allocator keeps its peak, so this is the peak), and a digest of the displacement.

    python scratch/matrix_free_rate.py                         the table: every configuration in a process of its own, each
                                                               under its own time limit, everything into profiles/matrix_free_rate.txt
    python scratch/matrix_free_rate.py one MATERIAL DEGREE ELEMENTS FLAG     one configuration, one JSON line
                                                               (MATERIAL neohook | j2, FLAG 0 | 1)
    MIMI_AMD_TREE=DIR MIMI_HIP_LIBRARY=LIB python scratch/matrix_free_rate.py one ...     the same on another commit's package and
                                                               library (the parent: it has no flag, so FLAG 0 only)

The table runs the parent's rows when MATRIX_FREE_PARENT_TREE and MATRIX_FREE_PARENT_LIBRARY name the parent's package
directory and library (python -m mimi_amd.build --out LIB --rev REV; git archive REV mimi_amd)."""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL = 1.0 / 64
LIMIT = 420          # seconds per configuration
# (material, degree, elements): the north-star block; J2 on that mesh (the record route); one degree-3 neo-Hookean block
CONFIGURATIONS = [("neohook", 2, "128x128x16"), ("j2", 2, "128x128x16"), ("neohook", 3, "64x64x8")]


def material(mimi, name):
    if name == "neohook":
        mat = mimi.CompressibleOgdenNeoHookean()
    else:
        mat = mimi.J2()
        mat.heat_fraction, mat.specific_heat, mat.initial_temperature, mat.melting_temperature = 0.9, 450, 20, 1500
        h = mimi.JohnsonCookTemperatureAndRateDependentHardening()
        for k, v in dict(A=70, B=140, n=0.2835, m=1.3558, eps0_dot=0.004, reference_temperature=20).items():   # (the reference's test law)
            setattr(h, k, v)
        mat.hardening = h
    mat.density = 1
    mat.viscosity = -1
    mat.set_young_poisson(2100, 0.3)
    return mat


def one(matname, degree, elements, flag):
    sys.path.insert(0, os.environ.get("MIMI_AMD_TREE") or ROOT)
    import numpy as np
    import torch
    import mimi_amd as mimi
    n_el = tuple(int(x) for x in elements.split("x"))
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "cube-nurbs.mesh"))      # the faces and boundary ids of a box
    nl.elevate_degrees(degree - 1)
    block = mimi.BSplinePatch.block(n_el, degree, lengths=[m * CELL for m in n_el])
    nl.patch = lambda: block
    nl.set_material(material(mimi, matname))
    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    rc.set_int("use_iterative_solver", 1)
    rc.set_int("use_kronecker_preconditioner", 1)
    if flag:
        rc.set_int("matrix_free", 1)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, -0.5)
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
    row = dict(material=matname, degree=degree, elements=list(n_el), matrix_free=bool(flag), package="another commit's" if os.environ.get("MIMI_AMD_TREE") else "this commit's",
               vdofs=len(nl.x), nnz=int(nl.pattern_.nnz), newton_iterations=h["iterations"], newton_converged=h["converged"],
               gmres_iterations=[s[1] for s in solves], gmres_converged=all(s[2] for s in solves),
               gmres_iterations_per_newton=sum(s[1] for s in solves) / newton, ms_per_newton_iteration=seconds * 1e3 / newton,
               solve_ms_per_newton_iteration=sum(s[0] for s in solves) * 1e3 / newton,
               device_memory_gb=(total_b - free_b) / 1e9, max_displacement=float(np.abs(nl.x).max()),
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
    r = torch.randn(len(nl.x), dtype=torch.float64, device=torch.device("cuda", 0))
    z = torch.zeros_like(r)
    if hasattr(nl, "d_jac_"):
        row["product_ms"] = per_call_ms(lambda: nl.linear_.AddMult(nl.d_jac_, r, z))
    else:
        row["product_ms_mass_matrix"] = per_call_ms(lambda: nl.linear_.AddMult(nl.d_mass_, r, z))
    if hasattr(nl.domain_, "ApplyTangent"):
        if not flag:
            nl.domain_.Linearize(nl.d_x_)
        row["linearize_ms"] = per_call_ms(lambda: nl.domain_.Linearize(nl.d_x_), reps=10)
        row["action_ms"] = per_call_ms(lambda: nl.domain_.ApplyTangent(r, z, stiffness=nl._fac0, density=1.0))
        row["record_gb"] = nl.domain_.LinearizationBytes() / 1e9
        z.zero_()
        row["residual_only_ms"] = per_call_ms(lambda: nl.domain_.AddDomainResidual(nl.d_x_, z))
    print(json.dumps(row), flush=True)


def table():
    out_path = os.path.join(ROOT, "profiles", "matrix_free_rate.txt")
    parent_tree, parent_lib = os.environ.get("MATRIX_FREE_PARENT_TREE"), os.environ.get("MATRIX_FREE_PARENT_LIBRARY")
    lines = ["scratch/matrix_free_rate.py on one MI355X: this commit with the flag on, with the flag off, and the parent commit, one",
             "session on one machine; every configuration in a process of its own.  Figures of the second implicit step."]
    for matname, degree, elements in CONFIGURATIONS:
        runs = [("this commit, matrix_free on", 1, {}), ("this commit, matrix_free off", 0, {})]
        if parent_tree and parent_lib:
            runs.append(("parent commit", 0, dict(MIMI_AMD_TREE=parent_tree, MIMI_HIP_LIBRARY=parent_lib)))
        lines.append(f"\n== {matname}, degree {degree}, {elements} elements ==")
        for label, flag, env in runs:
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "one", matname, str(degree), elements, str(flag)]
            p = subprocess.run(cmd, env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
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
    if sys.argv[1:2] == ["one"]:
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    else:
        sys.exit(table())
