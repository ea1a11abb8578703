"""The device coupling surface (integrators.CouplingSurface, csrc/surface.hip, NonlinearSolid.coupling_surface): points and
nodal loads against a numpy restatement of the formulas in include/mimi_hip.h and against closed forms (Nanson's formula
under a homogeneous deformation, the traction marker's dead load), then end to end through the fixed-point entries: with
ode_coefficient = 0 the coupling loop with t = -p n on the advanced configuration has the pressure marker's discrete
equations as its fixed point."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_pressure_gpu import homogeneous, smooth_u

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CASES = [((4, 3), 1), ((3, 3), 2), ((3, 2), 3), ((3, 2, 2), 1), ((2, 3, 2), 2), ((2, 2, 2), 3)]


def faces(dim):
    return [(0, 1), (dim - 1, 0), (1, 1)]


def restate(patch, axis, side, u=None, t=None):
    """x_q, n_q, w_q |m_q| and (with t) the nodal load, in numpy from splines.face_tables"""
    from mimi_amd import splines
    dim = patch.dim
    dofs, N, dN, w = splines.face_tables(patch, axis, side)
    X = patch.control_points + (0.0 if u is None else np.asarray(u).reshape(-1, dim))
    x = X[dofs]                                                          # [f, a, i]
    xq = np.einsum("fqa,fai->fqi", N, x)
    T = np.einsum("fqka,fai->fqki", dN, x)
    m = np.stack([T[:, :, 0, 1], -T[:, :, 0, 0]], axis=-1) if dim == 2 else np.cross(T[:, :, 0, :], T[:, :, 1, :])
    length = np.linalg.norm(m, axis=-1)
    wa = w * length
    f = None
    if t is not None:
        F = np.einsum("fq,fqa,fqi->fai", wa, N, np.asarray(t).reshape(w.shape + (dim,)))
        f = np.zeros(patch.n_vdofs)
        np.add.at(f, (dofs[:, :, None] * dim + np.arange(dim)).ravel(), F.ravel())
    return xq.reshape(-1, dim), (m / length[..., None]).reshape(-1, dim), wa.reshape(-1), f


def surface(patch, axis, side):
    from mimi_amd.integrators import CouplingSurface
    return CouplingSurface(patch, axis, side).Prepare()


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("n_el,p", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_points_reference_and_affine(n_el, p):
    import mimi_amd
    dim = len(n_el)
    lengths = [1.0 + 0.4 * d for d in range(dim)]
    patch = mimi_amd.BSplinePatch.block(n_el, p, lengths)
    rng = np.random.default_rng(5)
    F = np.eye(dim) + 0.1 * rng.standard_normal((dim, dim))
    J = np.linalg.det(F)
    u = homogeneous(patch, F)
    for axis, side in faces(dim):
        s = surface(patch, axis, side)
        assert s.n_points_ == s.n_faces_ * s.n_q_
        x, n, w = host(*s.points())
        xr, nr, wr, _ = restate(patch, axis, side)
        assert np.abs(x - xr).max() <= 1e-14 * np.abs(xr).max()
        assert np.abs(n - nr).max() <= 1e-14 and np.abs(w - wr).max() <= 1e-14 * wr.max()
        # affine u = (F - I) X: positions F X_q, normal * weight = J F^-T N dA0 (Nanson)
        x, n, w = host(*s.points(u))
        assert np.abs(x - xr @ F.T).max() <= 1e-13 * np.abs(xr).max()
        N0 = np.zeros(dim)
        N0[axis] = 1.0 if side else -1.0
        nda = J * (np.linalg.inv(F).T @ N0)[None, :] * wr[:, None]
        assert np.abs(n * w[:, None] - nda).max() <= 1e-13 * np.abs(nda).max()


@pytest.mark.parametrize("n_el,p", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_loads(n_el, p):
    import mimi_amd
    from mimi_amd import solid
    dim = len(n_el)
    patch = mimi_amd.BSplinePatch.block(n_el, p, [0.8 + 0.5 * d for d in range(dim)])
    rng = np.random.default_rng(11)
    for axis, side in faces(dim):
        s = surface(patch, axis, side)
        # a uniform nominal traction on the reference configuration is the traction marker's dead load
        t0 = rng.uniform(-2.0, 2.0, dim)
        s.set_traction(np.broadcast_to(t0, (s.n_points_, dim)).copy())
        f = s.load_.cpu().numpy()
        tv = solid.traction_vector(patch, axis, side, {i: t0[i] for i in range(dim)})
        assert np.abs(f - tv).max() <= 1e-13 * np.abs(tv).max()
        # random t on a random small displacement: the restatement; conservation; the same bits every run
        u = smooth_u(patch, scale=0.02, seed=axis + 7)
        t = rng.standard_normal((s.n_points_, dim))
        s.set_traction(t, u)
        f = s.load_.cpu().numpy()
        _, _, wa, fr = restate(patch, axis, side, u, t)
        assert np.abs(f - fr).max() <= 1e-13 * np.abs(fr).max()
        total = (wa[:, None] * t).sum(axis=0)
        assert np.abs(f.reshape(-1, dim).sum(axis=0) - total).max() <= 1e-13 * np.abs(wa[:, None] * t).sum()
        s.set_traction(t, u)
        assert s.load_.cpu().numpy().tobytes() == f.tobytes()
        # the C ABI adds into a pre-filled vector (host arrays here)
        base = rng.standard_normal(patch.n_vdofs)
        out = base.copy()
        s.AddLoad(u, t, out)
        assert np.array_equal(out, base + f)
        s.set_traction(None)
        assert s.load_ is None


# ---- through the facade ---------------------------------------------------------------------------------------------
FACADE = [("square-nurbs.mesh", (0, 1)), ("square-nurbs.mesh", (1, 1)), ("cube-nurbs.mesh", (0, 1)),
          ("cube-nurbs.mesh", (1, 1))]


def block_solid(mesh, face, pressure=None, traction=None, body=-20.0, ode_coefficient=None):
    """the golden square / cube at degree 2, 2 elements per direction, clamped on {xi_0 = 0}, loaded on `face` =
    (axis, side); returns the solid and the loaded face's bid"""
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(HERE, "golden", "meshes", mesh))
    nl.elevate_degrees(1)
    nl.subdivide(1)
    dim = nl.mesh_dim()
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    if ode_coefficient is not None:
        rc = mimi.RuntimeCommunication()
        rc.set_real("ode_coefficient", ode_coefficient)
        nl.runtime_communication = rc
    bc = mimi.BoundaryConditions()
    clamp = [a - 1 for a, f in nl._faces.items() if f == (0, 0)][0]
    loaded = [a - 1 for a, f in nl._faces.items() if f == tuple(face)][0]
    for c in range(dim):
        bc.initial.dirichlet(clamp, c)
    if body:
        bc.initial.body_force(dim - 1, body)
    if pressure is not None:
        bc.initial.pressure(loaded, pressure)
    if traction is not None:
        bc.initial.traction(loaded, dim - 1, traction)
    nl.boundary_condition = bc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-12, 1e-11, 20, False)
    nl.time_step_size = 0.05
    return nl, loaded


@pytest.mark.parametrize("mesh,face", FACADE, ids=lambda c: str(c).replace(" ", ""))
def test_constant_nominal_traction_matches_the_traction_marker(mesh, face):
    marker, loaded = block_solid(mesh, face, traction=-40.0, body=0.0)
    nl, _ = block_solid(mesh, face, body=0.0)
    dim = nl.mesh_dim()
    s = nl.coupling_surface(loaded)
    assert nl.coupling_surface(loaded) is s
    with pytest.raises(RuntimeError, match="quadrature_order"):
        nl.coupling_surface(loaded, quadrature_order=3)
    t = np.zeros((s.n_points_, dim))
    t[:, dim - 1] = -40.0
    with pytest.raises(ValueError, match="shape"):
        s.set_traction(t.T.copy())                     # [dim, n_points]: refused, not reinterpreted
    for _ in range(10):
        marker.step_time2()
        s.set_traction(t)                             # nominal: u = None
        nl.fixed_point_solve2()
        first = nl.fixed_point_advance2()[0].copy()
        nl.fixed_point_solve2()                        # the load does not depend on the iterate: a fixed point at once
        assert np.array_equal(nl.fixed_point_advance2()[0], first)
        nl.advance_time2()
        assert np.abs(nl.x - marker.x).max() <= 1e-10 * np.abs(marker.x).max()
    assert np.abs(marker.x).max() > 1e-3


@pytest.mark.parametrize("mesh,face", FACADE, ids=lambda c: str(c).replace(" ", ""))
def test_coupling_loop_converges_to_the_pressure_marker(mesh, face):
    """ode_coefficient = 0: alpha_f = 1, the residual is evaluated on the end-of-step configuration, which is what
    fixed_point_advance2 returns; t = -p n on it gives -p m w N_a, the pressure marker's load, at the fixed point"""
    p = 5.0                                            # moderate: plain Aitken converges on every case
    marker, loaded = block_solid(mesh, face, pressure=p, body=-2.0, ode_coefficient=0.0)
    assert marker._fac[1] == 1.0
    nl, _ = block_solid(mesh, face, body=-2.0, ode_coefficient=0.0)
    s = nl.coupling_surface(loaded)
    for step in range(3):
        marker.step_time2()
        u = nl.x.copy()
        omega, r_prev = 0.5, None                      # Aitken-relaxed, as a partitioned coupling runs it
        for it in range(60):
            _, n, _ = s.points(u)
            s.set_traction(-p * n, u)
            nl.fixed_point_solve2()
            x_adv = nl.fixed_point_advance2()[0].reshape(-1).copy()
            r = x_adv - u
            change = np.abs(r).max()
            if change <= 1e-12 * np.abs(x_adv).max():
                break
            if r_prev is not None:
                dr = r - r_prev
                if float(dr @ dr) > 0.0:
                    omega = -omega * float(r_prev @ dr) / float(dr @ dr)
            r_prev = r
            u = u + omega * r
        assert change <= 1e-10 * np.abs(x_adv).max(), (step, it, change)
        nl.advance_time2()
        assert np.abs(nl.x - marker.x).max() <= 1e-8 * np.abs(marker.x).max(), step
    assert np.abs(marker.x).max() > 1e-3


def test_refusals_and_the_folded_surface():
    import mimi_amd
    from mimi_amd import solid
    from mimi_amd.integrators import CouplingSurface
    from test_periodic_gpu import facade
    nl, _ = block_solid("cube-nurbs.mesh", (0, 1), body=0.0)
    with pytest.raises(RuntimeError, match="no boundary 17"):
        nl.coupling_surface(17)
    patch = mimi_amd.BSplinePatch.block((2, 2), 2)
    rational = mimi_amd.BSplinePatch(patch.degrees, patch.knots, patch.control_points, np.ones(patch.n_nodes))
    with pytest.raises(RuntimeError, match="rational patch"):
        CouplingSurface(rational, 0, 1).Prepare()
    # periodic: a joined face is refused; a free face gives the folded load, the traction marker's folded rhs
    per, x = facade("square-nurbs.mesh", "neohook", {3: 4}, steps=0, body=0.0)
    with pytest.raises(RuntimeError, match="interior"):
        per.coupling_surface(2)
    s = per.coupling_surface(1)                          # attribute 2: the top
    t0 = np.array([0.3, -1.7])
    s.set_traction(np.broadcast_to(t0, (s.n_points_, 2)).copy())
    f = s.load_.cpu().numpy()
    assert len(f) == len(x)
    axis, side = per._faces[2]
    tv = solid.traction_vector(per.patch_, axis, side, {0: t0[0], 1: t0[1]})
    folded = np.zeros(len(x))
    per.fold_.Add(tv, folded)
    assert np.abs(f - folded).max() <= 1e-13 * np.abs(folded).max()
    # a folded displacement: points and load on its expansion (every copy of a joined node moves with it)
    rng = np.random.default_rng(9)
    u_f = 0.02 * rng.standard_normal(len(x))
    u_u = u_f.reshape(-1, 2)[per.node_map_].reshape(-1)
    t = rng.standard_normal((s.n_points_, 2))
    xq, nq, wq = host(*s.points(u_f))
    s.set_traction(t, u_f)
    f = s.load_.cpu().numpy()
    xr, nr, wr, fr = restate(per.patch_, axis, side, u_u, t)
    assert np.abs(xq - xr).max() <= 1e-14 * np.abs(xr).max()
    assert np.abs(nq - nr).max() <= 1e-14 and np.abs(wq - wr).max() <= 1e-14 * wr.max()
    fr_f = np.zeros(len(x))
    per.fold_.Add(fr, fr_f)
    assert np.abs(f - fr_f).max() <= 1e-13 * np.abs(fr_f).max()
    # what a solve subtracts: the right-hand side plus the folded load, Dirichlet rows zero
    per.fixed_point_solve2()
    expect = per.rhs_ + f
    expect[per.dirichlet_] = 0.0
    assert np.abs(per._rhs.cpu().numpy() - expect).max() <= 1e-15 * np.abs(expect).max()
    per.advance_time2()
    assert np.abs(per.x).max() > 0


def test_northstar_top_face():
    """128 x 128 x 16, p = 2: the top face (16 384 faces x 16 points) against the restatement"""
    import torch
    import mimi_amd
    patch = mimi_amd.BSplinePatch.block((128, 128, 16), 2)
    s = surface(patch, 2, 1)
    assert (s.n_faces_, s.n_q_) == (16384, 16)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    u_h = 0.01 * rng.standard_normal(patch.n_vdofs)
    t_h = rng.standard_normal((s.n_points_, 3))
    u, t = torch.from_numpy(u_h).to(dev), torch.from_numpy(t_h).to(dev)
    x, n, w = host(*s.points(u))
    s.set_traction(t, u)
    f = s.load_.cpu().numpy()
    xr, nr, wr, fr = restate(patch, 2, 1, u_h, t_h)
    assert np.abs(x - xr).max() <= 1e-13 * np.abs(xr).max()
    assert np.abs(n - nr).max() <= 1e-13 and np.abs(w - wr).max() <= 1e-13 * wr.max()
    assert np.abs(f - fr).max() <= 1e-13 * np.abs(fr).max()


def test_example_runs_and_converges_every_step():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fixed_point_coupling.py"), "--steps", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("step")]
    assert len(lines) == 3
    for l in lines:
        fields = l.split()
        residual, tol = float(fields[fields.index("residual") + 1]), float(fields[fields.index("tol") + 1])
        assert residual <= tol and "converged True" in l, l
