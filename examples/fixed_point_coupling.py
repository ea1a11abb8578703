"""Partitioned fluid-structure coupling, headless: the reference's beam (tests/golden/meshes/balken.mesh at degree 3,
clamped at x = 0) under a toy "fluid" -- a hydrostatic pressure p = rho g (level - y) on its top face, evaluated at the
quadrature points of the ADVANCED configuration.  Every step iterates

    fluid:  points(u) of the wet surface  ->  traction t = -p n   ->  set_traction(t, u)
    solid:  fixed_point_solve2()  ->  fixed_point_advance2()  ->  the advanced displacement

with Aitken relaxation of the interface displacement until it stops changing, then advance_time2() commits the step.

    python examples/fixed_point_coupling.py [--steps 5] [--tol 1e-9]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mimi_amd as mimi  # noqa: E402


def build_beam(mesh_file):
    beam = mimi.NonlinearSolid()
    beam.read_mesh(mesh_file)
    beam.elevate_degrees(2)
    beam.subdivide(1)
    rubber = mimi.CompressibleOgdenNeoHookean()
    rubber.density = 1
    rubber.set_young_poisson(2100, 0.3)
    beam.set_material(rubber)
    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    beam.runtime_communication = rc
    conditions = mimi.BoundaryConditions()
    conditions.initial.dirichlet(2, 0).dirichlet(2, 1)       # the clamped end, as the reference's beam tests
    beam.boundary_condition = conditions
    beam.setup(1)
    beam.configure_newton("nonlinear_solid", 1e-12, 1e-11, 20, False)
    return beam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--tol", type=float, default=1e-9, help="relative change of the interface displacement")
    ap.add_argument("--max-iterations", type=int, default=50)
    args = ap.parse_args()
    beam = build_beam(os.path.join(REPO, "tests", "golden", "meshes", "balken.mesh"))
    beam.time_step_size = args.dt
    # the top face y = 1: of the patch's 2 dim boundaries, the one whose nodes all lie at the largest y
    dim = beam.mesh_dim()
    x_ref = beam.solution_view("displacement", "x_ref").reshape(-1, dim)
    top = next(b for b in range(2 * dim)
               if np.all(x_ref[beam.boundary_dof_ids("displacement", b, 1) // dim, 1] == x_ref[:, 1].max()))
    surface = beam.coupling_surface(top)
    wet = np.concatenate([beam.boundary_dof_ids("displacement", top, c) for c in range(dim)])
    rho_g, level = 1.0, 1.5

    def fluid(u):
        """the toy fluid: the wet surface of X + u -> its traction -p n (Cauchy: u is the advanced displacement)"""
        x, n, _ = surface.points(u)
        p = rho_g * (level - x[:, 1])
        return -p[:, None] * n

    u = beam.solution_view("displacement", "x").copy()                  # the relaxed displacement the fluid sees
    for step in range(args.steps):
        omega, r_prev, residual = 0.5, None, np.inf
        for it in range(1, args.max_iterations + 1):
            surface.set_traction(fluid(u), u)
            beam.fixed_point_solve2()
            x_adv = beam.fixed_point_advance2()[0].reshape(-1)
            r = x_adv - u
            residual = np.linalg.norm(r[wet]) / max(np.linalg.norm(x_adv[wet]), 1e-30)
            if residual <= args.tol:
                break
            if r_prev is not None:                                       # Aitken's factor from the last two residuals
                dr = r[wet] - r_prev
                dd = float(dr @ dr)
                if dd > 0.0:                                             # (a residual that did not change keeps omega)
                    omega = -omega * float(r_prev @ dr) / dd
            r_prev = r[wet].copy()
            u = u + omega * r
        beam.advance_time2()
        u = beam.solution_view("displacement", "x").copy()
        tip = u.reshape(-1, beam.mesh_dim())[:, 1].min()
        print(f"step {step:3d}  t = {beam.current_time:.3f}  iterations {it:2d}  residual {residual:.3e}  tol {args.tol:.1e}  "
              f"converged {residual <= args.tol}  tip deflection {tip:+.6e}", flush=True)


if __name__ == "__main__":
    main()
