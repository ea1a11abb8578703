"""Rigid-curve contact: the scenario of the reference's examples/nl_contact.py (a skewed quadrilateral block, a rigid
cubic Bezier punch that first descends, then slides sideways) on mimi_amd, printed instead of plotted.

The punch is handed over as any object with `degrees`, `knot_vectors`, `control_points` (a splinepy spline qualifies);
a SimpleNamespace is enough.

    python examples/nl_contact.py [--steps 30] [--friction MU] [--matrix-free] [--consistent-tangent]
                                  [--augmented N [--gap-tolerance T]]

--friction MU puts Coulomb friction on the punch (the reference has none): the tangential penalty is the scene's
coefficient, and the punch's displacement of the step is handed over as step_displacement, so that only the relative slip
of the surface against the punch loads the block.  The default, 0, prints what the frictionless run prints.

--consistent-tangent solves the Newton steps matrix-free (GMRES with the Kronecker preconditioner, the domain and contact
tangents as actions) and lets the contact action carry the derivative of the nodal pressure, which the reference's Jacobian
freezes: rc.set_int("contact_consistent_tangent", 1).  With --friction it needs --matrix-free.

--matrix-free solves the Newton steps matrix-free with the frozen-pressure contact action; with --friction the friction
tangent joins that action, rc.set_int("friction_matrix_free", 1), and --consistent-tangent may stand beside it: in slip
the traction is mu p_N s / |s|, so the consistent action then carries the pressure's derivative of the friction residual too.

--augmented N switches the contact to the augmented-Lagrangian law, rc.set_int("contact_augmented_lagrange", 1): a multiplier
per marked node, and up to N multiplier updates per step (each followed by a Newton solve) until the largest violation of the
constraint, a length, is at most --gap-tolerance (default 0: always N).  The loop contracts like k / (k + eps), k the stiffness
under the contact: worth its solves at a penalty of the order of the body's stiffness, as here; use --consistent-tangent with it.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import mimi_amd as mimi  # noqa: E402

DESCEND_STEPS = 100          # after that many steps the punch slides in -x
PUNCH_SPEED = 0.005          # per step


def make_block():
    block = mimi.NonlinearSolid()
    block.read_mesh(os.path.join(REPO, "tests", "golden", "meshes", "square-nurbs.mesh"))
    block.elevate_degrees(1)
    block.subdivide(3)
    steel_like = mimi.CompressibleOgdenNeoHookean()
    steel_like.density, steel_like.viscosity = 7e4, -1
    steel_like.set_young_poisson(1e10, 0.3)
    block.set_material(steel_like)
    return block


def make_punch():
    """cubic Bezier above the top edge; its normal (t_y, -t_x) points down, out of the rigid side"""
    pts = np.array([[-2.5, 1.3], [0.3, 0.7], [0.7, 0.7], [1.5, 1.3]])
    pts += np.array([0.05, 1.0])
    return SimpleNamespace(degrees=[3], knot_vectors=[[0.0] * 4 + [1.0] * 4], control_points=pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--friction", type=float, default=0.0, metavar="MU", help="friction coefficient of the punch (default 0)")
    ap.add_argument("--consistent-tangent", action="store_true",
                    help="matrix-free Newton solves with the consistent contact tangent (with --friction: needs --matrix-free)")
    ap.add_argument("--matrix-free", action="store_true",
                    help="matrix-free Newton solves; with --friction the friction tangent as a part of the contact action")
    ap.add_argument("--augmented", type=int, default=0, metavar="N",
                    help="augmented-Lagrangian contact with up to N multiplier updates per step (default 0: the penalty law)")
    ap.add_argument("--gap-tolerance", type=float, default=0.0, metavar="T",
                    help="stop updating once the largest violation of the constraint is at most T (with --augmented)")
    args = ap.parse_args()
    if args.consistent_tangent and args.friction > 0.0 and not args.matrix_free:
        ap.error("--consistent-tangent cannot be combined with --friction: the friction tangent is assembled only "
                 "(--matrix-free makes it an action)")

    block, punch = make_block(), make_punch()
    rigid_scene = mimi.NearestDistanceToSplines()
    rigid_scene.add_spline(punch)
    rigid_scene.plant_kd_tree(100000, 4)
    rigid_scene.coefficient = 0.5e11

    conditions = mimi.BoundaryConditions()
    conditions.initial.dirichlet(0, 0).dirichlet(0, 1)       # bottom edge clamped
    conditions.current.contact(1, rigid_scene)               # top edge may touch the punch
    block.boundary_condition = conditions
    if args.consistent_tangent or args.matrix_free or args.augmented > 0:
        flags = mimi.RuntimeCommunication()
        if args.augmented > 0:
            flags.set_int("contact_augmented_lagrange", 1)
            flags.set_int("contact_augmentations", args.augmented)
            flags.set_real("contact_gap_tolerance", args.gap_tolerance)
        for key in ("use_iterative_solver", "use_kronecker_preconditioner", "matrix_free", "matrix_free_boundary"):
            if args.consistent_tangent or args.matrix_free:
                flags.set_int(key, 1)
        if args.consistent_tangent:
            flags.set_int("contact_consistent_tangent", 1)
        if args.matrix_free and args.friction > 0.0:
            flags.set_int("friction_matrix_free", 1)
        block.runtime_communication = flags
    block.setup(4)
    block.configure_newton("nonlinear_solid", 1e-10, 1e-8, 100, False)
    block.time_step_size = 0.001
    rigid_scene.coefficient = 1e11                           # stiffer penalty once everything is set up
    rigid_scene.friction = args.friction

    disp = block.solution_view("displacement", "x").reshape(-1, block.mesh_dim())
    for k in range(args.steps):
        shift = [0.0, -PUNCH_SPEED] if k < DESCEND_STEPS else [-PUNCH_SPEED, 0.0]
        punch.control_points += shift
        rigid_scene.plant_kd_tree(10000, 4)                  # the moved body reaches the device handles here
        rigid_scene.step_displacement = shift                # (read by the friction law only)
        block.step_time2()
        info = block.newton_history[-1]
        contact = block.contacts_[0]
        rubbing = ""
        if args.friction > 0.0:
            rubbing = f"  friction force {contact.last_friction_force_}  stick {contact.n_stick_} slip {contact.n_slip_}"
        if args.augmented > 0 and block.augmentation_loops:
            loop = block.augmentation_loops[-1]
            rubbing += f"  augmentations {loop['augmentations']}  violation {loop['violations'][0]:.2e} -> {loop['violations'][-1]:.2e}"
        print(f"step {k:3d}  Newton iterations {info['iterations']:2d}  converged {info['converged']}  "
              f"|u|max = {np.abs(disp).max():.3e}  contact force {contact.last_force_}{rubbing}")


if __name__ == "__main__":
    main()
