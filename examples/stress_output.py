"""Stress and plastic-strain fields of a plastic cantilever: the 5 x 1 J2 beam of the solver tests (degree 3, 2 x 2
elements, Johnson-Cook hardening) bends under its own weight; every step the von Mises stress and the accumulated plastic
strain at the control points go into an .npz archive beside the displacement, and their maxima are printed.  Headless.

    python examples/stress_output.py [--steps 5] [--out stress_output.npz]

The nodal values are the lumped L2 projection of the quadrature-point values (NonlinearSolid.field).  In this 2-D problem
"von_mises_stress" is sqrt(3/2) |sigma - tr(sigma)/2 I|, the q of the material's own yield function.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mimi_amd as mimi  # noqa: E402


def build_beam(mesh_file, archive):
    solid = mimi.NonlinearSolid()
    solid.read_mesh(mesh_file)
    solid.elevate_degrees(2)          # p = 3
    solid.subdivide(1)                # 2 x 2 elements

    steel = mimi.J2()
    steel.density, steel.viscosity = 1, -1
    steel.set_young_poisson(2100, 0.3)
    steel.heat_fraction, steel.specific_heat = 0.9, 450
    steel.initial_temperature, steel.melting_temperature = 20, 1500
    law = mimi.JohnsonCookTemperatureAndRateDependentHardening()
    law.A, law.B, law.n, law.m, law.eps0_dot, law.reference_temperature = 70, 140, 0.2835, 1.3558, 0.004, 20
    steel.hardening = law
    solid.set_material(steel)

    conditions = mimi.BoundaryConditions()
    conditions.initial.dirichlet(2, 0).dirichlet(2, 1)
    conditions.initial.body_force(1, -3)
    solid.boundary_condition = conditions

    rc = mimi.RuntimeCommunication()
    rc.set_real("ode_coefficient", 0.5)
    rc.set_fname(archive)
    for name in ("x", "von_mises_stress", "accumulated_plastic_strain"):
        rc.append_should_save(name, 1)
    solid.runtime_communication = rc

    solid.setup(1)
    solid.configure_newton("nonlinear_solid", 1e-12, 1e-8, 10, False)
    solid.time_step_size = 0.5
    return solid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="stress_output.npz")
    args = ap.parse_args()
    if os.path.exists(args.out):
        os.remove(args.out)
    beam = build_beam(os.path.join(REPO, "tests", "golden", "meshes", "balken.mesh"), args.out)
    for k in range(args.steps):
        beam.step_time2()
        q = beam.field("von_mises_stress")
        eqps = beam.field("accumulated_plastic_strain")
        at_points = beam.field("accumulated_plastic_strain", where="points")
        print(f"step {k:3d}  t = {beam.current_time:.2f}  max von Mises {q.max():9.4f}  max plastic strain {eqps.max():.6f}  "
              f"yielded points {int((at_points > 0).sum())} / {at_points.size}")
    with np.load(args.out) as z:
        names = sorted(z.files)
    print(f"wrote {args.out}: {len(names)} arrays ({', '.join(names[:3])}, ...)")


if __name__ == "__main__":
    main()
