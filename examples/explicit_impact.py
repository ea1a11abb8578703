"""Impact of a plastic bar on a rigid wall with explicit dynamics: a 5 x 1 J2 bar (2-D, degree 2, 8 x 8 elements, Johnson-Cook
hardening) flies along its axis into a rigid plane; central differences with a lumped mass, no Jacobian and no linear solve
(rc.set_int("explicit_dynamics", 1), NonlinearSolid.explicit_steps).  The step is 0.9 of the body's stability limit
(stable_time_step); the energy ledger is sampled every few steps and goes into an .npz with the final displacement and the
accumulated plastic strain at the control points.  Headless.

    python examples/explicit_impact.py [--steps 60] [--every 5] [--velocity 5] [--out explicit_impact.npz]

The ledger's E* = KE - Q + W_int + W_damp - W_ext is conserved by the scheme up to rounding whatever the bar and the wall do;
it is printed with the samples.  A drift there means the step is too long -- the estimate covers the body, not the wall's
penalty (here the penalty spring of a wall node is far softer than the stiffest element, so the body's limit governs).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mimi_amd as mimi  # noqa: E402

LENGTH, GAP, PENALTY = 5.0, 0.01, 1.0e4
LEDGER = ("KE", "W_int", "W_ext", "W_damp", "Q", "E_star")


def build_bar(mesh_file):
    solid = mimi.NonlinearSolid()
    solid.read_mesh(mesh_file)
    solid.elevate_degrees(1)          # p = 2
    solid.subdivide(3)                # 8 x 8 elements

    steel = mimi.J2()
    steel.density, steel.viscosity = 1, -1
    steel.set_young_poisson(2100, 0.3)
    steel.heat_fraction, steel.specific_heat = 0.9, 450
    steel.initial_temperature, steel.melting_temperature = 20, 1500
    law = mimi.JohnsonCookTemperatureAndRateDependentHardening()
    law.A, law.B, law.n, law.m, law.eps0_dot, law.reference_temperature = 70, 140, 0.2835, 1.3558, 0.004, 20
    steel.hardening = law
    solid.set_material(steel)

    # no Dirichlet dof: the bar is free; the wall faces its right end (boundary 3: x = LENGTH)
    conditions = mimi.BoundaryConditions()
    wall = mimi.RigidPlane([LENGTH + GAP, 0.0], [-1.0, 0.0], PENALTY)
    conditions.current.contact(3, wall)
    solid.boundary_condition = conditions

    rc = mimi.RuntimeCommunication()
    rc.set_int("explicit_dynamics", 1)
    solid.runtime_communication = rc
    solid.setup(1)
    return solid


def run(steps=60, every=5, velocity=5.0, out="explicit_impact.npz", mesh_file=None):
    solid = build_bar(mesh_file or os.path.join(REPO, "tests", "golden", "meshes", "balken.mesh"))
    solid.time_step_size = solid.stable_time_step()
    v = solid.solution_view("displacement", "x_dot").reshape(-1, 2)
    v[:, 0] = velocity
    print(f"{len(solid.x)} dofs, dt = {solid.time_step_size:.3e} ({solid.stable_iterations_} power iterations)")
    samples = [(0.0, solid.explicit_energies())]
    done = 0
    while done < steps:
        n = min(every, steps - done)
        solid.explicit_steps(n)
        done += n
        e = solid.explicit_energies()
        samples.append((solid.current_time, e))
        print(f"step {done:4d}  t = {solid.current_time:.4e}  KE = {e['KE']:.6e}  W_int = {e['W_int']:.6e}  "
              f"E* - E*_0 = {e['E_star'] - samples[0][1]['E_star']:+.2e}  wall force = {solid.contacts_[0].last_force_[0]:+.3e}")
    eqps = solid.field("accumulated_plastic_strain")[:, 0]
    x_ref = solid.solution_view("displacement", "x_ref").reshape(-1, 2)
    print(f"plastic strain: max {eqps.max():.3e}, at the wall end {eqps[x_ref[:, 0] == x_ref[:, 0].max()].max():.3e}, "
          f"at the far end {eqps[x_ref[:, 0] == x_ref[:, 0].min()].max():.3e}")
    np.savez(out, time=np.array([t for t, _ in samples]), **{k: np.array([e[k] for _, e in samples]) for k in LEDGER},
             time_step_size=solid.time_step_size, x=solid.x.copy(), x_dot=solid.x_dot.copy(), x_ref=x_ref,
             accumulated_plastic_strain=eqps)
    return solid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--velocity", type=float, default=5.0)
    ap.add_argument("--out", default="explicit_impact.npz")
    args = ap.parse_args()
    run(args.steps, args.every, args.velocity, args.out)


if __name__ == "__main__":
    main()
