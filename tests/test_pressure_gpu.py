"""Follower pressure (integrators.FollowerPressure, csrc/pressure.hip) and the facade's pressure / traction markers on the
GPU.  The reference stores BCMarker::pressure_ and never applies it, so there is no reference output to compare with: the
kernels are checked against a numpy restatement of the formulas in include/mimi_hip.h, against difference quotients of
their own residual, and against closed forms (a closed surface feels no net force; Nanson's formula under a homogeneous
deformation; the homogeneous equilibrium of a neo-Hookean block under a follower or a dead load)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu


# ---- numpy restatement ----------------------------------------------------------------------------------------------
def face_blocks(patch, tables, u, pressure, face_nodes=None):
    """per face: residual Re[f, a, i] = sum_q w p N_a m_i and tangent Ke[f, a, i, b, j] = sum_q w p N_a dm_i/dx_bj, plus
    the area sum_q w |m| and the force -sum_q w p m of every face"""
    dofs, N, dN, w = tables
    dim = patch.dim
    x = patch.control_points + u.reshape(-1, dim)
    T = np.einsum("fqka,fai->fqki", dN, x[dofs])                       # a_k [f, q, k, i]
    if dim == 2:
        m = np.stack([T[:, :, 0, 1], -T[:, :, 0, 0]], axis=-1)
    else:
        m = np.cross(T[:, :, 0, :], T[:, :, 1, :])
    if np.isscalar(pressure):
        pq = np.full(w.shape, float(pressure))
    else:
        local = np.searchsorted(face_nodes, dofs)
        pq = np.einsum("fqa,fa->fq", N, np.asarray(pressure)[local])
    wp = w * pq
    Re = np.einsum("fq,fqa,fqi->fai", wp, N, m)
    # dm_i / dx_bj = sum_k dN_b,k D_k[i, j]
    if dim == 2:
        D = np.broadcast_to(np.array([[0.0, 1.0], [-1.0, 0.0]]), w.shape + (1, 2, 2))
    else:
        def skew(v):                                                    # [v]x: skew(v) @ e = v x e
            z = np.zeros(v.shape[:-1])
            return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                             np.stack([-v[..., 1], v[..., 0], z], -1)], -2)
        D = np.stack([-skew(T[:, :, 1, :]), skew(T[:, :, 0, :])], axis=2)   # [f, q, k, i, j]
    Ke = np.einsum("fq,fqa,fqkb,fqkij->faibj", wp, N, dN, D)
    area = np.einsum("fq,fq->f", w, np.linalg.norm(m, axis=-1))
    force = -np.einsum("fq,fqi->fi", wp, m)
    return Re, Ke, area, force


def assemble(patch, dofs, Re, Ke):
    dim = patch.dim
    n = patch.n_vdofs
    vd = (dofs[:, :, None] * dim + np.arange(dim)[None, None, :])       # [f, a, i]
    r = np.zeros(n)
    np.add.at(r, vd.ravel(), Re.ravel())
    nf, nd = dofs.shape
    rows = np.broadcast_to(vd[:, :, :, None, None], Ke.shape).ravel()
    cols = np.broadcast_to(vd[:, None, None, :, :], Ke.shape).ravel()
    A = sp.coo_matrix((Ke.ravel(), (rows, cols)), shape=(n, n)).tocsr()
    return r, A


def smooth_u(patch, scale=0.03, seed=1):
    rng = np.random.default_rng(seed)
    X = patch.control_points
    L = X.max(axis=0) - X.min(axis=0)
    u = np.zeros_like(X)
    for i in range(patch.dim):
        for _ in range(3):
            k = rng.uniform(0.5, 2.0, patch.dim) * np.pi / L
            u[:, i] += scale * L.mean() * np.sin(X @ k + rng.uniform(0, 2 * np.pi))
    return u.reshape(-1)


def gpu_csr(pattern, A, n):
    return sp.csr_matrix((A, pattern.col, pattern.rowptr), shape=(n, n))


def make(patch, axis, side, pattern=None, **kw):
    from mimi_amd.integrators import CSRPattern, FollowerPressure
    pattern = pattern or CSRPattern.of_bspline_patch(patch)
    return FollowerPressure("pressure", pattern, patch, axis, side, **kw).Prepare(), pattern


def run(fp, pattern, patch, u, gf=1.0):
    r = np.zeros(patch.n_vdofs)
    A = np.zeros(pattern.nnz)
    fp.AddBoundaryResidualAndGrad(u, gf, r, A)
    return r, A


PARITY = [((5,), 1), ((4,), 2), ((3,), 3), ((3, 2), 1), ((3, 3), 2), ((2, 3), 3)]


@pytest.mark.parametrize("n_tan,p", PARITY, ids=lambda c: str(c).replace(" ", ""))
@pytest.mark.parametrize("kind", ["uniform", "nodal"])
def test_parity_with_the_numpy_restatement(n_tan, p, kind):
    import mimi_amd
    from mimi_amd import splines
    dim = len(n_tan) + 1
    n_el = tuple(n_tan) + (2,)
    lengths = [1.0 + 0.4 * d for d in range(dim)]
    patch = mimi_amd.BSplinePatch.block(n_el, p, lengths)
    axis, side = dim - 1, 1
    fp, pattern = make(patch, axis, side)
    u = smooth_u(patch)
    nodes = fp.FaceNodes()
    if kind == "uniform":
        pressure = 3.7
    else:
        X = patch.control_points[nodes]
        pressure = 2.0 + np.sin(X.sum(axis=1)) + 0.3 * X[:, 0]
    fp.SetPressure(pressure)
    r, A = run(fp, pattern, patch, u, gf=0.8)
    tables = splines.face_tables(patch, axis, side)
    Re, Ke, _, _ = face_blocks(patch, tables, u, pressure, nodes)
    r_ref, A_ref = assemble(patch, tables[0], Re, Ke)
    A_ref = 0.8 * A_ref
    assert np.abs(r - r_ref).max() <= 1e-13 * np.abs(r_ref).max()
    Ad, Ad_ref = gpu_csr(pattern, A, patch.n_vdofs).toarray(), A_ref.toarray()
    assert np.abs(Ad - Ad_ref).max() <= 1e-12 * np.abs(Ad_ref).max()
    # nothing outside the face rows; the tangent is not symmetric
    rows = (nodes[:, None] * dim + np.arange(dim)).ravel()
    off = np.ones(patch.n_vdofs, bool)
    off[rows] = False
    assert np.all(r[off] == 0.0) and np.all(Ad[off] == 0.0)
    assert np.linalg.norm(Ad - Ad.T) > 1e-3 * np.linalg.norm(Ad)
    # the residual-only entry gives the same bits
    r2 = np.zeros(patch.n_vdofs)
    fp.AddBoundaryResidual(u, r2)
    assert np.array_equal(r, r2)


@pytest.mark.parametrize("n_el,p", [((4, 3), 2), ((3, 3), 3), ((3, 2, 2), 2), ((2, 2, 2), 3), ((3, 2, 3), 1)])
def test_tangent_against_central_differences(n_el, p):
    import mimi_amd
    dim = len(n_el)
    patch = mimi_amd.BSplinePatch.block(n_el, p, [1.0 + 0.3 * d for d in range(dim)])
    fp, pattern = make(patch, 0, 1)
    X = patch.control_points[fp.FaceNodes()]
    fp.SetPressure(5.0 + X[:, 1])
    u = smooth_u(patch, seed=3)
    v = smooth_u(patch, scale=1.0, seed=4)
    r, A = run(fp, pattern, patch, u)
    h = 1e-6
    rp_, rm_ = np.zeros(patch.n_vdofs), np.zeros(patch.n_vdofs)
    fp.AddBoundaryResidual(u + h * v, rp_)
    fp.AddBoundaryResidual(u - h * v, rm_)
    fd = (rp_ - rm_) / (2 * h)
    Av = gpu_csr(pattern, A, patch.n_vdofs) @ v
    assert np.abs(Av - fd).max() <= 1e-6 * np.abs(fd).max()


@pytest.mark.parametrize("n_el,p", [((4, 3), 1), ((3, 4), 2), ((3, 3), 3), ((3, 2, 2), 1), ((2, 3, 2), 2), ((2, 2, 2), 3),
                                    ((3, 2), 4)])
def test_closed_surface_feels_no_net_force(n_el, p):
    import mimi_amd
    from mimi_amd.integrators import CSRPattern
    dim = len(n_el)
    patch = mimi_amd.BSplinePatch.block(n_el, p, [0.8 + 0.5 * d for d in range(dim)])
    pattern = CSRPattern.of_bspline_patch(patch)
    u = smooth_u(patch, scale=0.05, seed=11)
    r = np.zeros(patch.n_vdofs)
    A = np.zeros(pattern.nnz)
    abs_r = np.zeros(patch.n_vdofs)
    for axis in range(dim):
        for side in (0, 1):
            fp, _ = make(patch, axis, side, pattern)
            fp.SetPressure(2.5)
            ri, Ai = run(fp, pattern, patch, u)
            r += ri
            A += Ai
            abs_r += np.abs(ri)
    R = r.reshape(-1, dim)
    for i in range(dim):
        assert abs(R[:, i].sum()) <= 1e-12 * abs_r.sum()
    # sum over the rows of a component of every column: d/dx of sum_a r(a, i) = 0
    M = gpu_csr(pattern, A, patch.n_vdofs)
    for i in range(dim):
        sel = np.zeros(patch.n_vdofs)
        sel[i::dim] = 1.0
        assert np.abs(M.T @ sel).max() <= 1e-11 * np.abs(A).max()


def homogeneous(patch, F):
    X = patch.control_points
    return (X @ (F - np.eye(patch.dim)).T).reshape(-1)


@pytest.mark.parametrize("n_el,p", [((4, 3), 2), ((3, 2), 3), ((3, 2, 2), 2), ((2, 3, 2), 3)])
def test_nanson(n_el, p):
    import mimi_amd
    dim = len(n_el)
    lengths = [1.0 + 0.5 * d for d in range(dim)]
    patch = mimi_amd.BSplinePatch.block(n_el, p, lengths)
    rng = np.random.default_rng(5)
    F = np.eye(dim) + 0.1 * rng.standard_normal((dim, dim))
    J = np.linalg.det(F)
    u = homogeneous(patch, F)
    for axis in range(dim):
        side = axis % 2
        fp, pattern = make(patch, axis, side)
        N0 = np.zeros(dim)
        N0[axis] = 1.0 if side else -1.0
        A0 = np.prod([lengths[d] for d in range(dim) if d != axis])
        nda = J * np.linalg.inv(F).T @ N0 * A0
        pv = 1.7
        fp.SetPressure(pv)
        run(fp, pattern, patch, u)
        fp.BoundaryPostTimeAdvance(u)
        assert np.abs(fp.last_force_ - (-pv * nda)).max() <= 1e-12 * np.abs(pv * nda).max()
        assert abs(fp.last_area_ - np.linalg.norm(nda)) <= 1e-12 * np.linalg.norm(nda)
        # a nodal pressure linear in X: the mean over the face is its value at the face's centroid
        p0, g = 0.9, np.array([0.4, -0.7, 0.25][:dim])
        nodes = fp.FaceNodes()
        fp.SetPressure(p0 + patch.control_points[nodes] @ g)
        Xc = np.array([lengths[d] / 2 for d in range(dim)])
        Xc[axis] = lengths[axis] if side else 0.0
        expect = -(p0 + g @ Xc) * nda
        run(fp, pattern, patch, u)
        fp.BoundaryPostTimeAdvance(u)
        assert np.abs(fp.last_force_ - expect).max() <= 1e-12 * np.abs(expect).max()


# ---- static equilibrium: follower pressure against the dead-load traction -------------------------------------------
def homogeneous_state(dim, target):
    """diagonal stretches lam with target(F = diag(lam)) = 0, by Newton with a complex-step Jacobian"""
    lam = np.ones(dim)
    for _ in range(50):
        g = target(np.diag(lam))
        Jm = np.zeros((dim, dim))
        for k in range(dim):
            e = np.zeros(dim, dtype=complex)
            e[k] = 1e-30j
            Jm[:, k] = np.imag(target(np.diag(lam + e))) / 1e-30
        step = np.linalg.solve(Jm, np.real(g))
        lam = lam - step
        if np.abs(step).max() < 1e-16:
            break
    return lam


@pytest.mark.parametrize("n_el", [(3, 2), (2, 2, 2)])
def test_static_equilibrium_follower_against_dead_load(n_el):
    import mimi_amd
    from mimi_amd import solid
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from test_closed_form_gpu import pk1
    dim = len(n_el)
    lengths = [1.2, 1.0, 0.8][:dim]
    patch = mimi_amd.BSplinePatch.block(n_el, 2, lengths)
    pattern = CSRPattern.of_bspline_patch(patch)
    mat = mimi_amd.CompressibleOgdenNeoHookean()
    mat.density = 1.0
    mat.set_young_poisson(2100, 0.3)
    G = NonlinearSolid("domain", mat, pattern, patch=patch).Prepare()
    fixed = np.unique(np.concatenate([patch.boundary_nodes(d, 0) * dim + d for d in range(dim)]))
    load = 80.0
    n = patch.n_vdofs
    sel = [(i, i) for i in range(dim)]

    def cauchy(F):
        return pk1("neohookean", F) @ F.T / np.linalg.det(F)

    def solve(extra):
        u = np.zeros(n)
        errs = []
        for it in range(8):
            r = np.zeros(n)
            A = np.zeros(pattern.nnz)
            G.AddDomainResidualAndGrad(u, 1.0, r, A)
            extra(u, r, A)
            r[fixed] = 0.0
            K = gpu_csr(pattern, A, n).tolil()
            K[fixed, :] = 0.0
            K[:, fixed] = 0.0
            K[fixed, fixed] = 1.0
            u = u - spla.spsolve(K.tocsc(), r)
            errs.append(u.copy())
        return u, errs

    # follower pressure on the face x_0 = L_0: Cauchy sigma_00 = -p, the lateral stresses 0
    fp, _ = make(patch, 0, 1, pattern)
    fp.SetPressure(load)
    lam_p = homogeneous_state(dim, lambda F: np.array([cauchy(F)[i, j] for i, j in sel]) + load * np.eye(dim)[0])
    u_p_exact = homogeneous(patch, np.diag(lam_p))
    u_p, hist_p = solve(lambda u, r, A: fp.AddBoundaryResidualAndGrad(u, 1.0, r, A))
    # dead load: first Piola P_00 = -t
    f_t = solid.traction_vector(patch, 0, 1, {0: -load})
    lam_t = homogeneous_state(dim, lambda F: np.array([pk1("neohookean", F)[i, j] for i, j in sel]) + load * np.eye(dim)[0])
    u_t_exact = homogeneous(patch, np.diag(lam_t))

    def dead(u, r, A):
        r -= f_t
    u_t, hist_t = solve(dead)
    for u_ex, hist in ((u_p_exact, hist_p), (u_t_exact, hist_t)):
        e = [np.abs(h - u_ex).max() / np.abs(u_ex).max() for h in hist]
        assert e[-1] <= 1e-10, e
        # quadratic rate over the last two steps that end above round-off
        k = [j for j in range(1, len(e)) if e[j] > 1e-12][-2:]
        assert len(k) == 2 and all(e[j] <= 100.0 * e[j - 1] ** 2 for j in k), e
    # the two loads of the same value give different states: the pressure follows the surface
    assert np.abs(lam_p - lam_t).max() > 1e-4
    assert np.abs(u_p - u_t).max() > 1e-3 * np.abs(u_p).max()


# ---- facade -----------------------------------------------------------------------------------------------------------
def cube(pressure=None, traction=None, body=-20.0, set_to=None, steps=3):
    import os
    import mimi_amd as mimi
    here = os.path.dirname(os.path.abspath(__file__))
    nl = mimi.NonlinearSolid()
    nl.read_mesh(os.path.join(here, "golden", "meshes", "cube-nurbs.mesh"))
    nl.elevate_degrees(1)
    nl.subdivide(1)
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    bc = mimi.BoundaryConditions()
    clamp = [a - 1 for a, f in nl._faces.items() if f == (0, 0)][0]
    loaded = [a - 1 for a, f in nl._faces.items() if f == (0, 1)][0]
    bc.initial.dirichlet(clamp, 0).dirichlet(clamp, 1).dirichlet(clamp, 2)
    if body:
        bc.initial.body_force(2, body)
    if pressure is not None:
        bc.initial.pressure(loaded, pressure)
    if traction is not None:
        bc.initial.traction(loaded, 2, traction)
    nl.boundary_condition = bc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-12, 1e-9, 20, False)
    nl.time_step_size = 0.05
    if set_to is not None:
        nl.set_pressure(loaded, set_to)
    for _ in range(steps):
        nl.step_time2()
    return nl, loaded


def test_facade_pressure_steps_and_zero_pressure_is_bitwise_no_marker():
    nl, loaded = cube(pressure=40.0)
    assert len(nl.newton_history) == 3 and all(h["converged"] for h in nl.newton_history)
    x = nl.solution_view("displacement", "x").reshape(-1, 3)
    assert np.abs(x).max() > 1e-4
    # the face x = 1 is pushed towards x = 0
    assert x[nl.patch_.boundary_nodes(0, 1), 0].mean() < 0
    fp = nl.pressures_[0]
    assert fp.last_area_ > 0 and fp.last_force_[0] < 0
    # a ramp between steps: applies from the next assembly
    nl.set_pressure(loaded, 80.0)
    nl.step_time2()
    assert nl.newton_history[-1]["converged"]
    with pytest.raises(KeyError):
        nl.set_pressure(loaded + 1, 1.0)
    plain, _ = cube()
    zero, _ = cube(pressure=0.0)
    reset, _ = cube(pressure=40.0, set_to=0.0)
    ref = plain.solution_view("displacement", "x")
    assert np.abs(ref).max() > 1e-4
    for other in (zero, reset):
        assert other.solution_view("displacement", "x").tobytes() == ref.tobytes()
        assert all(h["converged"] for h in other.newton_history)


def test_facade_traction_rhs_is_the_host_traction_vector():
    from mimi_amd import solid
    plain, _ = cube(body=0.0, steps=0)
    nl, loaded = cube(traction=-40.0, body=0.0, steps=1)
    axis, side = nl._faces[loaded + 1]
    tv = solid.traction_vector(nl.patch_, axis, side, {2: -40.0})
    tv[nl.dirichlet_] = 0.0
    assert np.all(plain.rhs_ == 0.0)
    assert np.array_equal(nl.rhs_ - plain.rhs_, tv)
    assert nl.newton_history[-1]["converged"]
    assert nl.solution_view("displacement", "x").reshape(-1, 3)[:, 2].min() < 0


# ---- element slabs, reproducibility, size ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_el,p", [((6, 3), 2), ((4, 5, 2), 2), ((4, 3, 2), 3)])
def test_element_slabs_sum_to_the_whole_face(n_el, p):
    import mimi_amd
    dim = len(n_el)
    patch = mimi_amd.BSplinePatch.block(n_el, p)
    axis, side = dim - 1, 1
    whole, pattern = make(patch, axis, side)
    u = smooth_u(patch, seed=21)
    X = patch.control_points[whole.FaceNodes()]
    pressure = 1.0 + 0.2 * X[:, 0]
    whole.SetPressure(pressure)
    r, A = run(whole, pattern, patch, u)
    split = n_el[0] // 2
    r2, A2 = np.zeros_like(r), np.zeros_like(A)
    for b0, e0 in ((0, split), (split, n_el[0])):
        begin, end = [0, 0, 0], list(n_el) + [1] * (3 - dim)
        begin[0], end[0] = b0, e0
        part, _ = make(patch, axis, side, pattern, element_box=(begin, end))
        assert part.n_faces_ < whole.n_faces_
        nodes = part.FaceNodes()
        part.SetPressure(pressure[np.searchsorted(whole.FaceNodes(), nodes)])
        part.AddBoundaryResidualAndGrad(u, 1.0, r2, A2)
    assert np.abs(r2 - r).max() <= 1e-15 * np.abs(r).max()
    assert np.abs(A2 - A).max() <= 1e-15 * np.abs(A).max()


def test_reproducible_bits_and_device_buffers():
    import torch
    import mimi_amd
    from mimi_amd.integrators import CSRPattern
    patch = mimi_amd.BSplinePatch.block((8, 7, 3), 2)
    pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
    fp, _ = make(patch, 2, 1, pattern)
    dev = torch.device("cuda", 0)
    u = torch.from_numpy(smooth_u(patch, seed=9)).to(dev)
    nodal = torch.from_numpy(1.0 + patch.control_points[fp.FaceNodes()][:, 0]).to(dev)
    fp.SetPressure(nodal)
    out = []
    for _ in range(2):
        r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
        A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
        fp.AddBoundaryResidualAndGrad(u, 1.0, r, A)
        torch.cuda.synchronize()
        out.append((r.cpu().numpy(), A.cpu().numpy()))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert np.abs(out[0][0]).max() > 0
    # the same values through host buffers
    pat_h = CSRPattern.of_bspline_patch(patch)
    fh, _ = make(patch, 2, 1, pat_h)
    fh.SetPressure(nodal.cpu().numpy())
    r_h, A_h = run(fh, pat_h, patch, u.cpu().numpy())
    assert np.array_equal(r_h, out[0][0]) and np.array_equal(A_h, out[0][1])


def test_cfg5_top_face_rows_beyond_2_31_entries():
    """256 x 256 x 32 at degree 2, p = 2 on the top face (65 536 faces): the face's rows lie beyond 2^31 matrix entries"""
    import torch
    import mimi_amd
    from mimi_amd import splines
    from mimi_amd.integrators import CSRPattern
    n_el = (256, 256, 32)
    patch = mimi_amd.BSplinePatch.block(n_el, 2)
    pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
    fp, _ = make(patch, 2, 1, pattern)
    assert fp.n_faces_ == 65536
    dev = torch.device("cuda", 0)
    F = np.array([[1.02, 0.01, 0.0], [-0.015, 0.99, 0.02], [0.005, 0.0, 0.97]])
    u_h = homogeneous(patch, F)
    u = torch.from_numpy(u_h).to(dev)
    fp.SetPressure(2.0)
    r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
    A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
    fp.AddBoundaryResidualAndGrad(u, 1.0, r, A)
    fp.BoundaryPostTimeAdvance(u)
    nda = np.linalg.det(F) * np.linalg.inv(F).T @ np.array([0.0, 0.0, 1.0]) * (256.0 * 256.0)
    assert np.abs(fp.last_force_ - (-2.0 * nda)).max() <= 1e-12 * np.abs(2.0 * nda).max()
    # sampled face nodes: their rows against the restatement of the faces around them
    rowptr = pattern.rowptr.cpu().numpy()
    col = pattern.col
    nodes = fp.FaceNodes()
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(nodes, 24, replace=False))
    tables = splines.face_tables(patch, 2, 1)
    dofs = tables[0]
    touch = np.nonzero(np.isin(dofs, sample).any(axis=1))[0]
    sub = tuple(t[touch] for t in tables)
    Re, Ke, _, _ = face_blocks(patch, sub, u_h, 2.0)
    r_ref, A_ref = assemble(patch, sub[0], Re, Ke)
    r_h = r.cpu().numpy()
    scale_r = np.abs(r_ref).max()
    for node in sample:
        for i in range(3):
            row = node * 3 + i
            assert rowptr[row] > 2 ** 31
            assert abs(r_h[row] - r_ref[row]) <= 1e-13 * scale_r
            beg, end = int(rowptr[row]), int(rowptr[row + 1])
            vals = A[beg:end].cpu().numpy()
            cols = col[beg:end].cpu().numpy()
            ref_row = A_ref.getrow(row).toarray().ravel()[cols]
            assert abs(A_ref.getrow(row)).sum() == pytest.approx(np.abs(ref_row).sum(), rel=1e-12)
            assert np.abs(vals - ref_row).max() <= 1e-12 * abs(A_ref).max()
