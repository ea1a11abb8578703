"""Milliseconds per explicit central-difference step (mimi_amd/explicit.py, csrc/explicit.hip) through the
facade: the north-star block (128 x 128 x 16 degree-2 elements of side 1 / 64, neo-Hookean, and J2 on that mesh) and cfg3
(128 x 128 x 16, degree 3, J2), one face clamped, a body force.  Per configuration: device-synchronised wall time per step
over STEPS steps after WARMUP, beside it in the same process the residual-only assembly alone, the state commit alone and the
two kernels of the stepper alone, the device memory in use at the end (torch's caching allocator keeps its peak and the library
returns no buffer, so this is the peak), E* before and after, and -- for context -- one implicit step (the second one; iterative route,
Kronecker preconditioner) on the same mesh, of this tree or of the parent commit's package.

    python scratch/explicit_rate.py                         the table: every configuration in a process of its own, each under
                                                            its own time limit, everything into profiles/explicit_rate.txt
    python scratch/explicit_rate.py one MATERIAL DEGREE ELEMENTS MODE      one configuration, one JSON line
                                                            (MATERIAL neohook | j2, MODE explicit | implicit)
    MIMI_AMD_TREE=DIR MIMI_HIP_LIBRARY=LIB python scratch/explicit_rate.py one ... implicit     the implicit step on another
                                                            commit's package and library (the parent)

The table runs the parent's implicit rows when EXPLICIT_PARENT_TREE and EXPLICIT_PARENT_LIBRARY name the parent's package
directory and library (python -m mimi_amd.build --out LIB --rev REV; git archive REV mimi_amd); without them the implicit
rows are this commit's with the flag unset, which tests/test_explicit_gpu.py holds to the parent's bytes."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL = 1.0 / 64
LIMIT = 420          # seconds per configuration
STEPS, WARMUP = 200, 20
CONFIGURATIONS = [("neohook", 2, "128x128x16"), ("j2", 2, "128x128x16"), ("j2", 3, "128x128x16")]


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


def per_call_ms(torch, f, reps=50):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def one(matname, degree, elements, mode):
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
    if mode == "explicit":
        rc.set_int("explicit_dynamics", 1)
    else:
        rc.set_int("use_iterative_solver", 1)
        rc.set_int("use_kronecker_preconditioner", 1)
    nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, -0.5)
    nl.boundary_condition = bc
    nl.setup(1)
    row = dict(material=matname, degree=degree, elements=list(n_el), mode=mode, vdofs=len(nl.x),
               package="MIMI_AMD_TREE" if os.environ.get("MIMI_AMD_TREE") else "this tree")
    if mode == "implicit":
        nl.configure_newton("nonlinear_solid", 1e-10, 1e-8, 10, False)
        nl.time_step_size = 0.01
        nl.step_time2()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nl.step_time2()
        torch.cuda.synchronize()
        h = nl.newton_history[-1]
        row.update(ms_per_implicit_step=(time.perf_counter() - t0) * 1e3, newton_iterations=h["iterations"], newton_converged=h["converged"],
                   time_step_size=nl.time_step_size)
    else:
        # an estimate at a loose tolerance is enough to pick a stable step for a timing run
        nl.time_step_size = nl.stable_time_step(rel_tol=1e-2, max_iter=60)
        row.update(time_step_size=nl.time_step_size, power_iterations=nl.stable_iterations_)
        e0 = nl.explicit_energies()
        nl.explicit_steps(WARMUP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nl.explicit_steps(STEPS)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        e = nl.explicit_energies()
        row.update(steps=STEPS, ms_per_explicit_step=seconds * 1e3 / STEPS, e_star_start=e0["E_star"], e_star_end=e["E_star"],
                   kinetic_energy=e["KE"], w_int=e["W_int"], w_ext=e["W_ext"], max_displacement=float(np.abs(nl.x).max()),
                   d2h_copies=nl.explicit_d2h_copies_)
        z = torch.zeros_like(nl.d_x_)
        st, x, v = nl.explicit_stepper_, nl.d_x_.clone(), nl.d_v_.clone()
        nl._push(nl.domain_)
        row["residual_only_ms"] = per_call_ms(torch, lambda: nl.domain_.AddDomainResidual(nl.d_x_, z))
        row["forces_ms"] = per_call_ms(torch, lambda: nl._explicit_forces(nl.d_x_, z))
        row["state_commit_ms"] = per_call_ms(torch, lambda: nl.domain_.DomainPostTimeAdvance(nl.d_x_), reps=20)
        row["predict_ms"] = per_call_ms(torch, lambda: st.Predict(0.0, x, v))
        r2 = [torch.zeros_like(z), torch.zeros_like(z)]
        flip = [0]

        def correct():
            flip[0] ^= 1
            st.Correct(0.0, nl._rhs, r2[flip[0]], None, v)
        st.Start(v, nl._rhs, z, None)
        row["correct_ms"] = per_call_ms(torch, correct)
    free_b, total_b = torch.cuda.mem_get_info()
    row["device_memory_gb"] = (total_b - free_b) / 1e9
    print(json.dumps(row), flush=True)


def table():
    out_path = os.path.join(ROOT, "profiles", "explicit_rate.txt")
    parent_tree, parent_lib = os.environ.get("EXPLICIT_PARENT_TREE"), os.environ.get("EXPLICIT_PARENT_LIBRARY")
    lines = ["scratch/explicit_rate.py on one MI355X: explicit steps of this commit and, for context, one implicit step (iterative",
             "route, Kronecker preconditioner) of " + ("the parent commit" if parent_tree and parent_lib else "this commit with the flag unset") +
             " on the same mesh; one session on one machine, every configuration in a process of its own."]
    for matname, degree, elements in CONFIGURATIONS:
        env = dict(MIMI_AMD_TREE=parent_tree, MIMI_HIP_LIBRARY=parent_lib) if parent_tree and parent_lib else {}
        lines.append(f"\n== {matname}, degree {degree}, {elements} elements ==")
        for label, mode, env in (("explicit", "explicit", {}), ("implicit", "implicit", env)):
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "one", matname, str(degree), elements, mode]
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
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5])
    else:
        sys.exit(table())
