"""Set-up of the facade on the device against the host pass, and the three form kernels at full size.

In fresh child processes, on the same GPU in the same run:
  * NonlinearSolid.setup() of cube-nurbs.mesh with elevate_degrees(1) and subdivide(6) (64^3 degree-2 elements, the case
    behind DESIGN.md's 17.6 s), once with MIMI_HIP_HOST_SETUP=1 and once without: wall time, peak device memory
    (torch.cuda.max_memory_allocated), host arrays of nnz doubles, host-to-device bytes of the set-up arrays;
  * mimi_hip_domain_add_mass / _add_diffusion / _add_body_force at 128 x 128 x 16, degree 2 and 3, timed with events on the
    handle's stream, against the store floor nnz / dim x 8 B / 6.3 TB/s (the copy rate VERDICT.md quotes).
Writes profiles/setup_device.json.

    python scratch/setup_time.py [--subdivide 6] [--out profiles/setup_device.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MESH = os.path.join(ROOT, "tests", "golden", "meshes", "cube-nurbs.mesh")
COPY_RATE = 6.3e12


def child_setup(subdivide):
    import numpy as np
    import torch
    import mimi_amd as mimi
    torch.zeros(1, device="cuda")                      # the runtime is up before the clock starts
    nl = mimi.NonlinearSolid()
    nl.read_mesh(MESH)
    nl.elevate_degrees(1)
    nl.subdivide(subdivide)
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    bc.initial.body_force(2, -9.81)
    nl.boundary_condition = bc
    rc = mimi.RuntimeCommunication()
    rc.set_int("use_iterative_solver", 1)
    nl.runtime_communication = rc
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    nl.setup(1)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    nnz, n = int(nl.pattern_.nnz), int(nl.rhs_.size)
    # what setup copies to the device: rhs, x, x_dot, the Dirichlet dofs; on the host route the matrix values too
    h2d = 8 * (3 * n + int(np.size(nl.dirichlet_))) + 8 * nnz * nl.host_nnz_arrays_
    return dict(route="host" if nl.host_setup_ else "device", elements=int(nl.n_elements()), n_vdofs=n, nnz=nnz,
                setup_seconds=seconds, peak_device_bytes=int(torch.cuda.max_memory_allocated()),
                host_arrays_of_nnz_doubles=int(nl.host_nnz_arrays_), host_to_device_bytes=int(h2d))


def child_kernels(p):
    import numpy as np
    import torch
    import mimi_amd as mimi
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    n_el = (128, 128, 16)
    patch = mimi.BSplinePatch.block(n_el, p)
    pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.set_young_poisson(2100, 0.3)
    G = NonlinearSolid("domain", mat, pattern, patch=patch).Prepare()
    A = torch.zeros(pattern.nnz, dtype=torch.float64, device="cuda")
    r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device="cuda")
    b = np.array([0.0, 0.0, -9.81])
    calls = dict(mass=lambda: G.AddMass(1.0, A), diffusion=lambda: G.AddDiffusion(1.0, A), body_force=lambda: G.AddBodyForce(b, r))
    out = dict(n_el=list(n_el), degree=p, nnz=int(pattern.nnz), store_floor_ms=1e3 * pattern.nnz / 3 * 8 / COPY_RATE)
    for name, call in calls.items():
        call()                                             # first call: adjacency, buffers
        times = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()                                    # (the handle launches on torch's current stream)
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out[name + "_ms"] = sorted(times)
    out["holds_gradient_tables"] = bool(G.HoldsGradientTables())
    return out


def run_child(args, env=None):
    e = dict(os.environ)
    e.pop("MIMI_HIP_HOST_SETUP", None)
    e.update(env or {})
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=e, stdout=subprocess.PIPE, text=True, check=True)
    print(res.stdout.strip().splitlines()[-1], file=sys.stderr, flush=True)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdivide", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_device.json"))
    ap.add_argument("--child", choices=["setup", "kernels"])
    ap.add_argument("--degree", type=int, default=2)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_setup(a.subdivide) if a.child == "setup" else child_kernels(a.degree)))
        return
    result = dict(case=f"cube-nurbs.mesh elevate_degrees(1) subdivide({a.subdivide})", copy_rate_bytes_per_s=COPY_RATE)
    result["setup_host"] = run_child(["--child", "setup", "--subdivide", str(a.subdivide)], {"MIMI_HIP_HOST_SETUP": "1"})
    result["setup_device"] = run_child(["--child", "setup", "--subdivide", str(a.subdivide)])
    result["kernels"] = [run_child(["--child", "kernels", "--degree", str(p)]) for p in (2, 3)]
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
