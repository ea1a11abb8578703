#!/usr/bin/env python3
"""usage: scratch/face_bits.py LIBRARY > hashes.txt        (one process per library; needs one GPU)
          scratch/face_bits.py --compare A.txt B.txt

Every route of the boundary integrators (contact, friction, the matrix-free actions, follower pressure, coupling surface) on
seeded inputs, through the library at LIBRARY (MIMI_HIP_LIBRARY): one line `label sha256` per result, the pattern of
scratch/dispatch_trace.py, which visits no face route.  Shapes: 2-D degree 2 on 4 x 4 elements, 3-D degrees 1 and 3 on
3 x 3 x 2 -- the smallest with interior, edge and corner face nodes, n_dof 3 / 4 / 16 and node pairs below and above 64.
The friction inputs are chosen so that stick and slip points both occur; the script asserts it from the history scalars.
--compare prints the labels whose hashes differ and exits 1 if there are any (or if the label sets differ)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 2, (4, 4)), (3, 1, (3, 3, 2)), (3, 3, (3, 3, 2)))
PENALTY, MU = 1.0e2, 0.3


def compare(a, b):
    read = lambda p: dict(line.split() for line in open(p) if line.strip())
    A, B = read(a), read(b)
    bad = sorted(set(A) ^ set(B)) + sorted(k for k in set(A) & set(B) if A[k] != B[k])
    for k in bad:
        print("differs:", k)
    print(f"{len(bad)} of {len(set(A) | set(B))} lines differ")
    return 1 if bad else 0


def main(library):
    os.environ["MIMI_HIP_LIBRARY"] = os.path.abspath(library)
    sys.path.insert(0, ROOT)
    import numpy as np
    import mimi_amd
    from mimi_amd.integrators import (CouplingSurface, CSRPattern, FollowerPressure, MortarContact, RigidPlane, RigidSphere,
                                      RigidSpline)

    def put(label, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        print(label.replace(" ", "_"), h.hexdigest())

    def bodies(dim, **kw):
        up = [0.0] * (dim - 1)
        yield "plane", RigidPlane(up + [0.98], up + [-1.0], PENALTY, **kw)
        yield "sphere", RigidSphere([0.5] * (dim - 1) + [1.0 + 0.9 * 0.4], 0.4, PENALTY, **kw)
        # a rigid spline that dips to 0.96 over the middle of the face, its normal pointing down
        if dim == 2:
            yield "spline", RigidSpline([2], [[0, 0, 0, 1, 1, 1]], [[-1.0, 1.02], [0.5, 0.90], [2.0, 1.02]], resolution=40,
                                        coefficient=PENALTY, **kw)
        else:
            z = [[1.02, 1.02, 1.02], [1.02, 0.78, 1.02], [1.02, 1.02, 1.02]]
            # (the first parameter, fastest in the list, along y, the second along x: S_u x S_v points down)
            cp = [[(-1.0, 0.5, 2.0)[ix], (-1.0, 0.5, 2.0)[iy], z[iy][ix]] for ix in range(3) for iy in range(3)]
            yield "spline", RigidSpline([2, 2], [[0, 0, 0, 1, 1, 1]] * 2, cp, resolution=20, coefficient=PENALTY, **kw)

    for dim, p, n_el in SHAPES:
        tag = f"d{dim}p{p}"
        rng = np.random.default_rng(1000 * dim + p)
        patch = mimi_amd.BSplinePatch.block(n_el, p, lengths=[1.0] * dim)
        pattern = CSRPattern.of_bspline_patch(patch, device=0)
        n, axis = patch.n_vdofs, dim - 1
        X = np.asarray(patch.control_points).reshape(-1, dim)
        u = 2.0e-3 * rng.standard_normal(n)
        x = rng.standard_normal(n)
        u0 = np.zeros(n)
        shear = np.zeros((n // dim, dim))
        shear[:, 0] = 0.012 * X[:, 0]              # eps_T |s| = mu p_N near x = 0.5 under the plane: stick below, slip above
        u1 = (shear + 2.0e-4 * rng.standard_normal(shear.shape)).reshape(-1)

        def actions(c, label, at):
            for mode in (False, True):
                c.SetConsistentTangent(mode)
                c.Linearize(at)
                y = np.full(n, 0.25)
                c.ApplyTangent(x, y, 0.7)
                put(f"{label} action consistent={int(mode)} y", y)
                put(f"{label} action consistent={int(mode)} bytes", np.int64(c.LinearizationBytes()))
            c.SetConsistentTangent(False)

        # contact, frictionless
        for name, body in bodies(dim):
            c = MortarContact(body, "contact", pattern, patch, axis, 1).Prepare()
            r, A = np.zeros(n), np.zeros(pattern.nnz)
            c.AddBoundaryResidual(u, r)
            put(f"{tag} contact {name} residual r", r)
            c.BoundaryPostTimeAdvance(u)
            put(f"{tag} contact {name} residual history", c.last_area_, c.last_pressure_, c.last_force_)
            r[:] = 0.0
            c.AddBoundaryResidualAndGrad(u, 0.9, r, A)
            put(f"{tag} contact {name} tangent r", r)
            put(f"{tag} contact {name} tangent A", A)
            c.BoundaryPostTimeAdvance(u)
            put(f"{tag} contact {name} tangent history", c.last_area_, c.last_pressure_, c.last_force_)
            put(f"{tag} contact {name} pressure", c.AveragePressure())
            put(f"{tag} contact {name} gap norm", np.float64(c.GapNorm(u)))
            assert np.any(c.AveragePressure() != 0.0), (tag, name)
            actions(c, f"{tag} contact {name}", u)
        # contact with friction: evaluate and commit at u0, evaluate at u1, commit, evaluate again
        for name, body in bodies(dim, friction=MU):
            c = MortarContact(body, "contact", pattern, patch, axis, 1).Prepare()
            c.BoundaryPostTimeAdvance(u0)
            r, A = np.zeros(n), np.zeros(pattern.nnz)
            c.AddBoundaryResidualAndGrad(u1, 1.0, r, A)
            c._history()
            put(f"{tag} friction {name} first r", r)
            put(f"{tag} friction {name} first A", A)
            put(f"{tag} friction {name} first history", c.last_friction_force_, c.last_friction_traction_,
                np.int64([c.n_stick_, c.n_slip_]))
            # (the sphere is exempt: it touches the middle of the face only, where in 3-D the shear is already past the stick limit of
            # its small pressure, so all its points slip; plane and spline cover both branches on every shape)
            if name != "sphere":
                assert c.n_stick_ > 0 and c.n_slip_ > 0, (tag, name, c.n_stick_, c.n_slip_)
            print(f"# {tag} friction {name}: {c.n_stick_} points stick, {c.n_slip_} slip", file=sys.stderr)
            c.SetFrictionAction(True)
            actions(c, f"{tag} friction {name}", u1)
            c.CommitFriction()
            r[:] = 0.0
            c.AddBoundaryResidual(1.5 * u1, r)
            c._history()
            put(f"{tag} friction {name} second r", r)
            put(f"{tag} friction {name} second history", c.last_friction_force_, c.last_friction_traction_,
                np.int64([c.n_stick_, c.n_slip_]))
            c.BoundaryPostTimeAdvance(1.5 * u1)
            put(f"{tag} friction {name} state", *c.FrictionState())
        # follower pressure, uniform and nodal (some nodes without pressure: inactive faces)
        fp = FollowerPressure("pressure", pattern, patch, axis, 1).Prepare()
        nodal = rng.standard_normal(len(fp.FaceNodes()))
        nodal[np.asarray(X[fp.FaceNodes(), 0]) < 0.5] = 0.0
        for name, value in (("uniform", 2.0), ("nodal", nodal)):
            fp.SetPressure(value)
            r, A = np.zeros(n), np.zeros(pattern.nnz)
            fp.AddBoundaryResidual(u, r)
            put(f"{tag} pressure {name} residual r", r)
            r[:] = 0.0
            fp.AddBoundaryResidualAndGrad(u, 0.9, r, A)
            fp.BoundaryPostTimeAdvance(u)
            put(f"{tag} pressure {name} tangent r", r)
            put(f"{tag} pressure {name} tangent A", A)
            put(f"{tag} pressure {name} history", fp.last_area_, fp.last_force_)
            fp.Linearize(u)
            y = np.full(n, 0.25)
            fp.ApplyTangent(x, y, 0.7)
            put(f"{tag} pressure {name} action y", y)
        # coupling surface
        s = CouplingSurface(patch, axis, 1).Prepare()
        for name, at in (("current", u), ("reference", None)):
            xq, nq, wq = (np.zeros((s.n_points_, dim)), np.zeros((s.n_points_, dim)), np.zeros(s.n_points_))
            s.Points(at, xq, nq, wq)
            put(f"{tag} surface {name} points", xq)
            put(f"{tag} surface {name} normals", nq)
            put(f"{tag} surface {name} weights", wq)
            f = np.full(n, 0.125)
            s.AddLoad(at, rng.standard_normal((s.n_points_, dim)), f)
            put(f"{tag} surface {name} load", f)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
