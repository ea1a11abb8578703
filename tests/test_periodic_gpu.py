"""Periodic boundaries on the device (csrc/fold.hip) and through the facade, and the constant-velocity marker.

The fold is checked against scipy's P^T A P, the whole periodic assembly against the oracle's unwrapped assembly folded
by scipy, and the solver against two closed forms: uniaxial strain of a block periodic in x and y, and the
x-independence of a block periodic in x under a body force."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = os.path.join(HERE, "golden", "meshes")


def p_matrix(node_map, dim):
    """scipy P: unwrapped vdof (n, c) <- folded vdof (node_map[n], c)"""
    n_u = len(node_map) * dim
    rows = np.arange(n_u)
    cols = (np.repeat(node_map, dim) * dim + np.tile(np.arange(dim), len(node_map)))
    return sp.csr_matrix((np.ones(n_u), (rows, cols)), shape=(n_u, int(node_map.max() + 1) * dim))


def make_fold(n_el, p, axes, device_pattern=False):
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, PeriodicFold, periodic_node_map
    patch = mimi_amd.BSplinePatch.block(n_el, p)
    pattern = CSRPattern.of_bspline_patch(patch, on_device=device_pattern)
    nm = periodic_node_map(patch.n_ctrl, axes)
    return patch, pattern, nm, PeriodicFold(pattern, nm, patch.dim).Prepare()


FOLD_CASES = [((4, 3), 1, [0]), ((3, 4), 2, [0, 1]), ((5, 2), 3, [1]), ((1, 3), 2, [0]), ((1, 1), 3, [0, 1]),
              ((3, 2, 2), 1, [0, 1, 2]), ((4, 3, 2), 2, [0]), ((2, 3, 4), 2, [1, 2]), ((1, 3, 2), 2, [0, 2]),
              ((3, 2, 3), 3, [0, 1, 2]), ((1, 1, 1), 2, [0, 1, 2]), ((2, 1, 3), 3, [1])]


@pytest.mark.parametrize("n_el,p,axes", FOLD_CASES, ids=lambda c: str(c).replace(" ", ""))
def test_fold_against_scipy(n_el, p, axes):
    import torch
    patch, pattern, nm, fold = make_fold(n_el, p, axes)
    dim = patch.dim
    P = p_matrix(nm, dim)
    n_u, n_f = P.shape
    rng = np.random.default_rng(11)
    A_u = rng.uniform(0.5, 1.5, pattern.nnz) * rng.choice([-1.0, 1.0], pattern.nnz)
    r_u = rng.standard_normal(n_u)
    Au = sp.csr_matrix((A_u, pattern.col, pattern.rowptr), shape=(n_u, n_u))
    expect = (P.T @ Au @ P).tocsr()
    expect.sort_indices()
    # the structure of P^T A P (every entry of A_u is non-zero and of random sign: no cancellation to exact zero here)
    fp = fold.Pattern()
    assert fp.nnz == expect.nnz == fold.nnz_f_
    assert np.array_equal(fp.rowptr, expect.indptr) and np.array_equal(fp.col, expect.indices)
    assert fold.n_f_ == n_f
    # values: A_f = A_base + P^T A_u P, r_f += P^T r_u
    base = rng.standard_normal(fp.nnz)
    r0 = rng.standard_normal(n_f)
    r_f, A_f = r0.copy(), np.full(fp.nnz, np.nan)
    fold.Add(r_u, r_f, A_u, base, A_f)
    scale = np.abs(expect.data).max()
    assert np.abs(A_f - (base + expect.data)).max() <= 1e-14 * scale
    assert np.abs(r_f - (r0 + P.T @ r_u)).max() <= 1e-14 * np.abs(r_f).max()
    # "+=" (A_base is A_f), overwrite (A_base None), residual only, matrix only
    A2 = base.copy()
    fold.Add(None, None, A_u, A2, A2)
    assert np.array_equal(A2, A_f)
    A3 = np.full(fp.nnz, np.nan)
    fold.Add(None, None, A_u, None, A3)
    assert np.abs(A3 - expect.data).max() <= 1e-14 * scale
    r4 = r0.copy()
    fold.Add(r_u, r4)
    assert np.array_equal(r4, r_f)
    # expand is exact
    u_f = rng.standard_normal(n_f)
    u_u = np.zeros(n_u)
    fold.Expand(u_f, u_u)
    assert np.array_equal(u_u, P @ u_f)
    # device arguments: the same bits, twice
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    outs = []
    for _ in range(2):
        rd, Ad = t(r0), t(base)
        fold.Add(t(r_u), rd, t(A_u), Ad, Ad)
        torch.cuda.synchronize()
        outs.append((rd.cpu().numpy(), Ad.cpu().numpy()))
    for rd, Ad in outs:
        assert np.array_equal(rd, r_f) and np.array_equal(Ad, A_f)
    ud = torch.zeros(n_u, dtype=torch.float64, device=dev)
    fold.Expand(t(u_f), ud)
    assert np.array_equal(ud.cpu().numpy(), u_u)
    # a fold built from device-resident pattern arrays is the same fold
    _, pattern_d, _, fold_d = make_fold(n_el, p, axes, device_pattern=True)
    fpd = fold_d.Pattern()
    assert np.array_equal(fpd.rowptr, fp.rowptr) and np.array_equal(fpd.col, fp.col)
    A5 = np.full(fp.nnz, np.nan)
    fold_d.Add(None, None, A_u, base, A5)
    assert np.array_equal(A5, A_f)
    # the self-overlapping rows (one element along a periodic axis) are the ones added by one lane
    if any(n_el[a] == 1 for a in axes):
        assert fold.Info(4) > 0


@pytest.mark.parametrize("matname", ["neohook", "j2"])
@pytest.mark.parametrize("case", [((3, 4, 2), 2, [0]), ((3, 2, 3), 3, [0, 1]), ((2, 3, 4), 2, [0, 1, 2])],
                         ids=lambda c: str(c).replace(" ", ""))
def test_pipeline_against_oracle(case, matname):
    """the oracle's unwrapped assembly folded by scipy against the tensor path + the device fold"""
    from oracle import ref_path as rp
    from mimi_amd.integrators import PeriodicFold, periodic_node_map
    from test_domain_gpu import make_pair, relmax, synthetic_u
    n_el, p, axes = case
    P, D, G = make_pair(n_el, p, None, matname, "bspline")
    nm = periodic_node_map(G.patch_.n_ctrl, axes)
    fold = PeriodicFold(G.pattern_, nm, P.dim).Prepare()
    Pm = p_matrix(nm, P.dim)
    n_u, n_f = Pm.shape
    dt = 0.5
    D.set_dt(dt)
    G.dt_ = dt
    rng = np.random.default_rng(5)
    if matname == "j2":
        # a committed plastic state (the state lives at the quadrature points: any displacement commits one)
        u0 = synthetic_u(P, scale=0.03, seed=7)
        D.domain_post_time_advance(u0)
        G.DomainPostTimeAdvance(u0)
        assert D.eqps.max() > 1e-4
    u_f = (0.02 if matname == "j2" else 0.05) * rng.standard_normal(n_f)
    u_u = np.zeros(n_u)
    fold.Expand(u_f, u_u)
    gf = 0.37
    r_o, A_o = np.zeros(n_u), np.zeros(D.nnz)
    D.add_domain_residual_and_grad(u_u, gf, r_o, A_o, rp.TANGENT_EXACT)
    Ao = sp.csr_matrix((A_o, G.pattern_.col, G.pattern_.rowptr), shape=(n_u, n_u))
    expect = (Pm.T @ Ao @ Pm).tocsr()
    expect.sort_indices()
    r_u, A_u = np.zeros(n_u), np.zeros(G.pattern_.nnz)
    G.AddDomainResidualAndGrad(u_u, gf, r_u, A_u)
    # periodicity did not push the patch off the two-phase tensor kernels
    assert G.LastKernelFamily() == ("tensor_p2_two_phase" if p == 2 else "tensor_p3_two_phase")
    base = rng.standard_normal(fold.nnz_f_)
    r_f, A_f = np.zeros(n_f), np.zeros(fold.nnz_f_)
    fold.Add(r_u, r_f, A_u, base, A_f)
    fp = fold.Pattern()
    assert np.array_equal(fp.col, expect.indices)
    assert relmax(r_f, Pm.T @ r_o) < 1e-12
    assert relmax(A_f - base, expect.data) < 1e-12


# ---- closed form: uniaxial strain ---------------------------------------------------------------------------------------
def test_uniaxial_strain_periodic_block():
    """3-D p = 2 block periodic in x and y, bottom clamped, follower pressure on top: F = diag(1, 1, lam) with Cauchy
    sigma_zz(lam) = -p, u_z = (lam - 1) Z at every node.  Without the marker the lateral faces are free and it fails."""
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, FollowerPressure, NonlinearSolid, PeriodicFold, periodic_node_map
    from test_closed_form_gpu import pk1
    from scipy.optimize import brentq
    n_el, L = (3, 3, 4), (1.0, 1.2, 0.9)
    patch = mimi_amd.BSplinePatch.block(n_el, 2, L)
    pattern = CSRPattern.of_bspline_patch(patch)
    mat = mimi_amd.CompressibleOgdenNeoHookean()
    mat.density = 1.0
    mat.set_young_poisson(2100, 0.3)
    G = NonlinearSolid("domain", mat, pattern, patch=patch).Prepare()
    fp = FollowerPressure("pressure", pattern, patch, 2, 1).Prepare()
    load = 150.0
    fp.SetPressure(load)
    lam = brentq(lambda l: (pk1("neohookean", np.diag([1.0, 1.0, l])) @ np.diag([1.0, 1.0, l]).T / l)[2, 2] + load, 0.5, 1.0)
    X = patch.control_points.reshape(-1, 3)
    u_exact = np.zeros_like(X)
    u_exact[:, 2] = (lam - 1.0) * X[:, 2]

    def solve(axes):
        nm = periodic_node_map(patch.n_ctrl, axes) if axes else np.arange(patch.n_nodes)
        fold = PeriodicFold(pattern, nm, 3).Prepare()
        Pm = p_matrix(nm, 3)
        n_f = Pm.shape[1]
        fixed = np.unique(nm[patch.boundary_nodes(2, 0)])
        fixed = np.concatenate([fixed * 3 + c for c in range(3)])
        fpat = fold.Pattern()
        u_f = np.zeros(n_f)
        for _ in range(10):
            u_u = np.zeros(patch.n_vdofs)
            fold.Expand(u_f, u_u)
            r_u, A_u = np.zeros(patch.n_vdofs), np.zeros(pattern.nnz)
            G.AddDomainResidualAndGrad(u_u, 1.0, r_u, A_u)
            fp.AddBoundaryResidualAndGrad(u_u, 1.0, r_u, A_u)
            r, A = np.zeros(n_f), np.zeros(fold.nnz_f_)
            fold.Add(r_u, r, A_u, None, A)
            r[fixed] = 0.0
            K = sp.csr_matrix((A, fpat.col, fpat.rowptr), shape=(n_f, n_f)).tolil()
            K[fixed, :] = 0.0
            K[:, fixed] = 0.0
            K[fixed, fixed] = 1.0
            u_f = u_f - spla.spsolve(K.tocsc(), r)
        return (Pm @ u_f).reshape(-1, 3)

    u = solve([0, 1])
    assert np.abs(u - u_exact).max() <= 1e-10 * np.abs(u_exact).max()
    u_free = solve([])
    assert np.abs(u_free - u_exact).max() > 1e-3 * np.abs(u_exact).max()


# ---- facade -------------------------------------------------------------------------------------------------------------
def facade(mesh, matname, pairs, steps=3, cv=None, body=-40.0):
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(mesh if os.path.isabs(mesh) else os.path.join(MESHES, mesh))
    nl.elevate_degrees(1)
    nl.subdivide(2)
    if matname == "neohook":
        mat = mimi.CompressibleOgdenNeoHookean()
        mat.density = 1.0
        mat.set_young_poisson(2100, 0.3)
    else:
        from test_domain_gpu import product_material
        mat = product_material("j2")
    nl.set_material(mat)
    bc = mimi.BoundaryConditions()
    dim = nl.mesh_dim()
    for c in range(dim):
        bc.initial.dirichlet(0, c)                    # attribute 1: the bottom (y = 0 in 2-D, z = 0 in 3-D)
    bc.initial.body_force(dim - 1, body)
    for b0, b1 in pairs.items():
        bc.initial.periodic(b0, b1)
    if cv:
        for bid, comp, value in cv:
            bc.initial.constant_velocity(bid, comp, value)
    nl.boundary_condition = bc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-12, 1e-10, 20, False)
    nl.time_step_size = 0.05
    x = nl.solution_view("displacement", "x")
    for _ in range(steps):
        nl.step_time2()
    return nl, x


def rectangle_mesh(tmp_path):
    """square-nurbs.mesh with the corners of the rectangle [0, 2] x [0, 1] (the golden one is a quadrilateral with a
    slanted side: no field of y alone solves it)"""
    with open(os.path.join(MESHES, "square-nurbs.mesh")) as f:
        lines = f.read().rstrip().split("\n")
    path = os.path.join(str(tmp_path), "rectangle-nurbs.mesh")
    with open(path, "w") as f:
        f.write("\n".join(lines[:-4] + ["0 0", "2 0", "2 1", "0 1"]) + "\n")
    return path


@pytest.mark.parametrize("matname", ["neohook", "j2"])
@pytest.mark.parametrize("mesh,pairs", [("rectangle", {3: 4}), ("cube-nurbs.mesh", {6: 4, 3: 5})])
def test_x_independence_through_the_facade(mesh, pairs, matname, tmp_path):
    if mesh == "rectangle":
        mesh = rectangle_mesh(tmp_path)
    nl, x = facade(mesh, matname, pairs)
    dim = nl.mesh_dim()
    assert nl.fold_ is not None and nl.domain_.LastKernelFamily() != "general"
    assert all(h["converged"] for h in nl.newton_history)
    nm = nl.dof_map("displacement")
    assert len(x) == (nm.max() + 1) * dim
    u = x.reshape(-1, dim)[nm]                       # expanded: every node of the patch
    n_ctrl = nl.patch_.n_ctrl
    grid = u.reshape(tuple(reversed(n_ctrl)) + (dim,))
    last = grid[..., dim - 1]
    scale = np.abs(last).max()
    assert scale > 1e-6
    # every node equals every node of its plane of constant last coordinate; no lateral motion
    plane = last.reshape(n_ctrl[-1], -1)
    assert np.abs(plane - plane[:, :1]).max() <= 1e-10 * scale
    assert np.abs(grid[..., :dim - 1]).max() <= 1e-10 * scale
    # x_ref has the folded size; npz-style output is the expanded vector
    assert len(nl.solution_view("displacement", "x_ref")) == len(x)
    assert len(nl.in_reference_numbering(x)) == nl.patch_.n_vdofs
    # without the marker the profile varies along x (the lateral faces are free)
    nl0, x0 = facade(mesh, matname, {})
    assert nl0.fold_ is None
    g0 = x0.reshape(tuple(reversed(n_ctrl)) + (dim,))[..., dim - 1].reshape(n_ctrl[-1], -1)
    assert np.abs(g0 - g0[:, :1]).max() > 1e-3 * scale


@pytest.mark.parametrize("pairs", [{}, {3: 4}])
def test_constant_velocity(pairs):
    """square, bottom fixed, top (bid 1 = attribute 2) moving up at v: after k steps the top's y-displacement is exactly
    k v dt and its velocity v; the interior moves; the run is bitwise reproducible"""
    v, steps = 0.3, 4
    runs = []
    for _ in range(2):
        nl, x = facade("square-nurbs.mesh", "neohook", pairs, steps=steps, cv=[(1, 1, v)], body=0.0)
        runs.append((x.copy(), nl.solution_view("displacement", "x_dot").copy()))
    (x, xd), (x2, xd2) = runs
    assert np.array_equal(x, x2) and np.array_equal(xd, xd2)
    dim = 2
    top = np.unique(nl._folded_dofs(nl.patch_.boundary_nodes(1, 1), 1))
    expect = 0.0
    for _ in range(steps):
        expect = expect + v * nl.time_step_size       # x + value dt per step, in the solver's own arithmetic
    assert np.array_equal(x[top], np.full(len(top), expect))
    assert np.array_equal(xd[top], np.full(len(top), v))
    interior = np.setdiff1d(np.arange(len(x)), np.concatenate([top, nl.dirichlet_]))
    assert np.abs(x[interior]).max() > 0.1 * steps * v * nl.time_step_size
    assert len(x) == (nl.dof_map("displacement").max() + 1) * dim


def test_northstar_size_seam_rows():
    """128 x 128 x 16, p = 2, periodic along x: sampled seam and interior rows of the folded device values against the
    unwrapped device rows summed over the copies through the node map (the fold at 3 x 10^8 entries, 64-bit offsets)"""
    import torch
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid, PeriodicFold, periodic_node_map
    from _sampling import sample_nodes
    n_el, p = (128, 128, 16), 2
    patch = mimi_amd.BSplinePatch.block(n_el, p, [8.0, 8.0, 1.0])
    pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
    mat = mimi_amd.CompressibleOgdenNeoHookean()
    mat.density = 1.0
    mat.set_young_poisson(2100, 0.3)
    G = NonlinearSolid("domain", mat, pattern, patch=patch).Prepare()
    nm = periodic_node_map(patch.n_ctrl, [0])
    fold = PeriodicFold(pattern, nm, 3).Prepare()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    u_f = torch.from_numpy(0.01 * rng.standard_normal(fold.n_f_)).to(dev)
    u_u = torch.zeros(fold.n_u_, dtype=torch.float64, device=dev)
    fold.Expand(u_f, u_u)
    r_u = torch.zeros_like(u_u)
    A_u = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
    G.AddDomainResidualAndGrad(u_u, 1.0, r_u, A_u)
    assert G.LastKernelFamily() == "tensor_p2_two_phase"
    fp = fold.Pattern(on_device=True)
    r_f = torch.zeros(fold.n_f_, dtype=torch.float64, device=dev)
    A_f = torch.empty(fold.nnz_f_, dtype=torch.float64, device=dev)
    fold.Add(r_u, r_f, A_u, None, A_f)
    torch.cuda.synchronize()
    rp_u, col_u = pattern.rowptr.cpu().numpy(), pattern.col.cpu().numpy()
    rp_f, col_f = fp.rowptr.cpu().numpy(), fp.col.cpu().numpy()
    r_uh, r_fh = r_u.cpu().numpy(), r_f.cpu().numpy()
    n = patch.n_ctrl
    copies = {}
    for k, F in enumerate(nm):
        copies.setdefault(int(F), []).append(k)
    for mi in sample_nodes(n, 12, 9):
        node = mi[0] + n[0] * (mi[1] + n[1] * mi[2])
        F = int(nm[node])
        for c in range(3):
            R = F * 3 + c
            want = {}
            rsum = 0.0
            for src in copies[F]:
                row = src * 3 + c
                b, e = int(rp_u[row]), int(rp_u[row + 1])
                vals = A_u[b:e].cpu().numpy()
                for cu, v in zip(col_u[b:e], vals):
                    cf = int(nm[cu // 3]) * 3 + cu % 3
                    want[cf] = want.get(cf, 0.0) + v
                rsum += r_uh[row]
            b, e = int(rp_f[R]), int(rp_f[R + 1])
            assert list(col_f[b:e]) == sorted(want)
            got = A_f[b:e].cpu().numpy()
            exp = np.array([want[k] for k in sorted(want)])
            assert np.abs(got - exp).max() <= 1e-13 * np.abs(exp).max()
            assert abs(r_fh[R] - rsum) <= 1e-13 * max(abs(rsum), np.abs(r_uh).max())
