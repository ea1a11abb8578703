"""The boundary-face reference (tests/_face_reference.py) against closed forms, and the host code that feeds the three
boundary integrators -- splines.face_tables, oracle.iga.Patch.face_tables, oracle.ContactOracle -- against the reference, on
every face of every patch of tests/_patches.py (non-uniform and repeated knots, a different degree per axis, jittered control
points) at the default quadrature order and at the orders of tests/test_faces_gpu.py.  No GPU.

Every host quantity is held to 1/8 of the bar tests/test_faces_gpu.py holds the kernels to (MARGIN x _face_cases.TOL, relative
to the largest reference entry), so that a kernel comparison never rests on the reference's or the inputs' own error.

Worst host-against-reference figures measured (x86-64, 80-bit long double), with the margin each is held to:
  face tables (product and oracle), numpy restatement in doubles, all cases x faces x orders
    pressure residual 1.3e-15, area 7.0e-16, force 7.8e-16 (1.25e-14); tangent 3.7e-15 (1.25e-13)
    point positions 8.0e-16 (1.25e-15); da 2.6e-15 (1.25e-14)
    unit normals 5.7e-16 (1.25e-15) on every patch but nonuni3d_p3: 2.2e-15, the rounding of the tables themselves at degree
    3 on spans of 0.2 beside coordinates of 4.  That patch's normals are held to 1e-13 here and on the GPU (1.25e-14), the
    finding reported in tests/test_faces_gpu.py; summed plainly, sum_a (X + u)_a dN_a, doubles give 1.4e-14 there.
  oracle.ContactOracle (plane and sphere, exact tangent)
    pressure, residual, tangent, gap norm, force, pressure integral 7.3e-14 (rep2d_p2 at one point per face: |g| = 2e-3 against
    coordinates of 4; <= 2.1e-14 elsewhere) (1.25e-13, tangent and force 1.25e-12); area 1.6e-15 (1.25e-14)
  contact inputs: penetrating share 0.25 .. 0.45 of the points of a face, min |g| 8.3e-4; 23 (face, body) cases on 5 patches
    hold faces whose nodal pressures are all zero
  the reference alone: closed-surface sums 4.4e-19, Nanson 8.2e-18, tangent against difference quotients 1.5e-15.

That the orientation check bites was tried on a scratch copy of splines.face_tables: with the 2-D flip rule inverted all 8
two-dimensional cases of test_face_tables_against_the_reference fail, with the 3-D tangent order swapped all 14
three-dimensional ones; the restatement-based tests of test_pressure_gpu.py / test_coupling_surface_gpu.py read the same tables
as the kernels and cannot see either."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _face_cases as fc
import _face_reference as fr
import _patches
from test_pressure_gpu import assemble, face_blocks

LD = np.longdouble
MARGIN = 0.125
# long-double rounding of a tangent sum_a x_a dN_a: 1.1e-19 x sum |x_a| |dN_a| (|x| <= 5, |dN| <= p / h <= 15 on the finest
# span, at most 16 terms) is 1.3e-16; a wrong table errs by O(1)
ROUNDING = 2e-16
CASES = list(_patches.CASES)
ORDER_CASES = [(c, -1) for c in CASES + fc.BLOCKS] + fc.ORDERS_ALL
CONTACT_CASES = ORDER_CASES + fc.ORDERS_CONTACT


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)).max() / np.abs(np.asarray(b, dtype=LD)).max())


def report(label, **figures):
    print(f"figures {label}: " + " ".join(f"{k}={v:.2e}" for k, v in figures.items()))


# ---- the reference against closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + fc.BLOCKS)
def test_reference_partition_of_unity(case):
    for axis, side in fc.faces(case):
        fb = fc.face_basis(case, axis, side)
        assert np.abs(fb.N.sum(axis=1) - 1).max() <= 1e-17 * 64
        assert np.abs(fb.dN.sum(axis=2)).max() <= 1e-17 * 64 * np.abs(fb.dN).max()
        assert np.all(fb.w > 0)
        # off the face nothing: the end function of an open knot vector is the only one that is not zero there
        nodes = fr.face_node_ids(fb.n_ctrl, axis, side)
        assert np.all(np.delete(fb.N, nodes, axis=1) == 0) and np.all(fb.N[:, nodes].max(axis=0) > 0)


def test_gauss_legendre_in_long_double():
    for n in (1, 2, 5, 8, 21):
        x, w = fr.gauss_legendre(n)
        for k in range(2 * n):                                        # exact for the monomials up to degree 2 n - 1
            exact = LD(2) / (k + 1) if k % 2 == 0 else LD(0)
            assert abs((w * x ** k).sum() - exact) <= 1e-18
        assert np.abs(x.astype(np.float64) - np.polynomial.legendre.leggauss(n)[0]).max() <= 1e-15


@pytest.mark.parametrize("case", CASES)
def test_reference_closed_surface_identities(case):
    """over the 2 dim faces of the deformed patch: sum int n da = 0, sum int x x n da = 0, sum int x . n da = dim V -- the
    rule of p_max + 2 points integrates all three exactly (degree 3 p <= 2 p_max + 3 per direction), so they hold to rounding"""
    B = fc.product_patch(case)
    dim = B.dim
    total, total_abs, moment, moment_abs, flux = 0, 0, 0, 0, 0
    for axis, side in fc.faces(case):
        pts = fc.points(case, axis, side)
        nda = pts.fb.w[:, None] * pts.m
        total, total_abs = total + nda.sum(axis=0), total_abs + pts.da.sum()
        mom = pts.x[:, 0] * nda[:, 1] - pts.x[:, 1] * nda[:, 0] if dim == 2 else np.cross(pts.x, nda)
        moment, moment_abs = moment + mom.sum(axis=0), moment_abs + np.abs(mom).sum()
        flux = flux + np.einsum("qi,qi->", pts.x, nda)
    x = B.control_points.astype(LD) + fc.displacement(case).reshape(-1, dim).astype(LD)
    V = fr.volume(B.degrees, B.knots, x)
    figures = dict(force=float(np.abs(total).max() / total_abs), moment=float(np.abs(moment).max() / moment_abs),
                   volume=float(abs(flux - dim * V) / (dim * V)))
    report(case, **figures)
    assert V > 0 and max(figures.values()) <= 1e-17


def greville(knots, p):
    """in long double: rounded to doubles the abscissae would not reproduce the identity map to better than 1e-16 p / h"""
    knots = np.asarray(knots, dtype=LD)
    return np.array([knots[i + 1:i + p + 1].sum() / p for i in range(len(knots) - p - 1)], dtype=LD)


@pytest.mark.parametrize("case", CASES)
def test_reference_nanson_under_an_affine_map(case):
    """x = F X on the un-jittered Greville patch (X = xi): m w = J F^-T N_0 w at every point, the position is F xi"""
    B = fc.product_patch(case)
    dim = B.dim
    g = [greville(k, p) for k, p in zip(B.knots, B.degrees)]
    X = np.stack([gr.ravel(order="F") for gr in np.meshgrid(*g, indexing="ij")], axis=1)
    F = np.eye(dim) + 0.1 * np.random.default_rng(5).standard_normal((dim, dim))
    F = F.astype(LD)
    # the cofactor matrix J F^-T, written out
    if dim == 2:
        cof = np.array([[F[1, 1], -F[1, 0]], [-F[0, 1], F[0, 0]]], dtype=LD)
    else:
        cof = np.stack([np.cross(F[:, 1], F[:, 2]), np.cross(F[:, 2], F[:, 0]), np.cross(F[:, 0], F[:, 1])], axis=1)
    worst = 0.0
    for axis, side in fc.faces(case):
        fb = fc.face_basis(case, axis, side)
        pts = fr.face_points(fb, X.astype(LD) @ F.T)
        N0 = np.zeros(dim, dtype=LD)
        N0[axis] = 1 if side else -1
        worst = max(worst, float(np.abs(pts.m - cof @ N0).max()))
        ref = fr.face_points(fb, X)
        assert np.abs(ref.m - N0).max() <= ROUNDING and np.abs(pts.x - ref.x @ F.T).max() <= ROUNDING
        area0 = np.prod([B.knots[d][-1] - B.knots[d][0] for d in range(dim) if d != axis])
        assert abs(ref.da.sum() - area0) <= ROUNDING * area0
    report(case, nanson=worst)
    assert worst <= ROUNDING


@pytest.mark.parametrize("case", CASES)
def test_reference_tangent_against_central_differences(case):
    """dense tangent columns against (r(x + h e) - r(x - h e)) / 2 h in long double, to 1e-12 of the largest entry.  The
    residual is quadratic (3-D) or linear (2-D) in x, so the quotient has no truncation error at any step, only the rounding
    eps |r| / (2 h |K|) with eps = 1.1e-19 and |r| / |K| between 1 and 10 here: h = 1e-8 cannot resolve 1e-12 in this format
    (measured 8e-12 .. 1.3e-10 over the 14 patches), h = 2^-10 does."""
    B = fc.product_patch(case)
    dim = B.dim
    x0 = B.control_points.astype(LD) + fc.displacement(case).reshape(-1, dim).astype(LD)
    h = LD(2) ** -10
    worst = 0.0
    for axis, side in fc.faces(case):
        fb = fc.face_basis(case, axis, side)
        nodes = fr.face_node_ids(fb.n_ctrl, axis, side)
        p = fc.nodal_pressure(B, nodes)
        K = fc.pressure_reference(case, axis, side).K
        fd = np.zeros_like(K)
        cols = (nodes[:, None] * dim + np.arange(dim)).ravel()
        for c in nodes * dim + np.arange(len(nodes)) % dim:            # every face node, the components in turn
            out = []
            for s in (1, -1):
                x = x0.copy()
                x[c // dim, c % dim] += s * h
                out.append(fr.follower_pressure(fr.face_points(fb, x), p, nodes, with_tangent=False).r)
            fd[:, c] = (out[0] - out[1]) / (2 * h)
        some = nodes * dim + np.arange(len(nodes)) % dim
        worst = max(worst, float(np.abs(fd[:, some] - K[:, some]).max() / np.abs(K).max()))
        # the frozen-pressure contact tangent is the same sum with the contact pressure and the other sign
        assert np.all(np.delete(K, cols, axis=1) == 0)
    report(case, tangent_fd=worst)
    assert worst <= 1e-12


# ---- the face tables against the reference ---------------------------------------------------------------------------------
def table_points(tables, X, u):
    """x_q, unit normal, w |m| of face tables (dofs, N [f, q, a], dN [f, q, k, a], weight) in numpy doubles.  The tangents
    are summed over X and u apart, each about the face's mean (sum_a dN_a = 0): what is measured is the tables, not the
    cancellation of sum_a (X + u)_a dN_a in doubles, which costs the plain sum up to 1.4e-14 in the normal here."""
    dofs, N, dN, w = tables
    dim = X.shape[1]
    xq = np.einsum("fqa,fai->fqi", N, (X + u)[dofs])
    T = sum(np.einsum("fqka,fai->fqki", dN, v[dofs] - v[dofs].mean(axis=1, keepdims=True)) for v in (X, u))
    m = np.stack([T[:, :, 0, 1], -T[:, :, 0, 0]], axis=-1) if dim == 2 else np.cross(T[:, :, 0, :], T[:, :, 1, :])
    length = np.linalg.norm(m, axis=-1)
    return xq.reshape(-1, dim), (m / length[..., None]).reshape(-1, dim), (w * length).reshape(-1)


def both_tables(case, axis, side, order):
    from mimi_amd import splines
    ft = fc.oracle_patch(case).face_tables(axis, side, order)
    return {"product": splines.face_tables(fc.product_patch(case), axis, side, order),
            "oracle": (ft["conn"], ft["N"], np.ascontiguousarray(np.transpose(ft["dN_dxi"], (0, 1, 3, 2))), ft["weight"])}


@pytest.mark.parametrize("case,order", ORDER_CASES, ids=lambda c: str(c))
def test_face_tables_against_the_reference(case, order):
    """the first test that fails on a wrong span, node id, derivative scale or orientation in the tables"""
    B = fc.product_patch(case)
    dim = B.dim
    u = fc.displacement(case)
    worst = dict(r=0.0, K=0.0, x=0.0, n=0.0, da=0.0, area=0.0, force=0.0)
    for axis, side in fc.faces(case):
        pts = fc.points(case, axis, side, order)
        for who, tables in both_tables(case, axis, side, order).items():
            assert tables[3].shape[1] == pts.fb.n_q_face
            assert np.array_equal(np.unique(tables[0]), fr.face_node_ids(B.n_ctrl, axis, side))
            for kind in ("uniform", "nodal"):
                ref = fc.pressure_reference(case, axis, side, order, kind)
                Re, Ke, area, force = face_blocks(B, tables, u, ref.pressure, ref.nodes)
                r, A = assemble(B, tables[0], Re, Ke)
                worst["r"] = max(worst["r"], rel(r, ref.r))
                worst["K"] = max(worst["K"], rel(A.toarray(), ref.K))
                worst["area"] = max(worst["area"], rel(area.sum(), ref.area))
                worst["force"] = max(worst["force"], rel(force.sum(axis=0), ref.force))
            xq, nq, da = table_points(tables, B.control_points, u.reshape(-1, dim))
            perm, dist = fr.match_points(pts.x, xq)
            worst["x"] = max(worst["x"], rel(xq[perm], pts.x))
            worst["n"] = max(worst["n"], float(np.abs(nq[perm] - pts.n).max()))
            worst["da"] = max(worst["da"], rel(da[perm], pts.da))
    report(f"{case} order {order}", **worst)
    assert worst["r"] <= MARGIN * fc.TOL["pressure_r"] and worst["K"] <= MARGIN * fc.TOL["pressure_K"]
    assert worst["area"] <= MARGIN * fc.TOL["pressure_r"] and worst["force"] <= MARGIN * fc.TOL["pressure_r"]
    assert worst["x"] <= MARGIN * fc.TOL["surface_x"] and worst["n"] <= MARGIN * fc.tol(case, "surface_n")
    assert worst["da"] <= MARGIN * fc.TOL["surface_da"]


def test_face_slab_tables_partition_the_face_on_repeated_knots():
    """element_box slabs along a tangential axis with a repeated interior knot: the slabs' faces are the whole face's, once
    each (face_tables counts elements by patch.n_spans there, not by knot index)"""
    from mimi_amd import splines
    for case, axis, cut_axis in (("rep3d_p2", 2, 0), ("rep2d_p3", 1, 0), ("rep3d_p2", 1, 0)):
        B = fc.product_patch(case)
        whole = splines.face_tables(B, axis, 1)
        m = B.n_spans[cut_axis]
        rows = []
        for b0, e0 in ((0, m // 2), (m // 2, m)):
            begin, end = [0, 0, 0], list(B.n_spans) + [1] * (3 - B.dim)
            begin[cut_axis], end[cut_axis] = b0, e0
            part = splines.face_tables(B, axis, 1, element_box=(begin, end))
            assert 0 < len(part[0]) < len(whole[0])
            rows.append(part)
        for k in range(4):
            joined = np.concatenate([p[k] for p in rows])
            order = np.lexsort(np.concatenate([p[0] for p in rows]).T[::-1])
            assert np.array_equal(joined[order], whole[k][np.lexsort(whole[0].T[::-1])])


# ---- the contact oracle against the reference ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_pattern(case):
    return fc.oracle_patch(case).sparsity()


def oracle_contact(case, axis, side, order, kind):
    """the oracle's residual, exact tangent (dense) and scalars of a contact case"""
    from oracle import ref_path as rp
    P = fc.oracle_patch(case)
    rowptr, col = oracle_pattern(case)
    b = fc.body(case, axis, side, order, kind)
    Cn = rp.ContactOracle(P, axis, side, b, penalty=fc.PENALTY, quadrature_order=order, rowptr=rowptr, col=col)
    u = fc.displacement(case)
    r, A = np.zeros(P.n_vdofs), np.zeros(rowptr[-1])
    Cn.add_boundary_residual_and_grad(u, fc.GRAD_FACTOR, r, A, rp.TANGENT_EXACT)
    K = sp.csr_matrix((A, col, rowptr), shape=(P.n_vdofs, P.n_vdofs)).toarray()
    return Cn, r, K, Cn.gap_norm(u)


@pytest.mark.parametrize("case,order", CONTACT_CASES, ids=lambda c: str(c))
def test_contact_inputs_and_oracle_against_the_reference(case, order):
    """the input conditions on the reference alone (partial contact, no point on the discontinuity), then the oracle"""
    worst = dict(pressure=0.0, r=0.0, K=0.0, gap_norm=0.0, area=0.0, force=0.0, last_pressure=0.0)
    shares, min_g = [], np.inf
    for axis, side in fc.faces(case):
        for kind in ("plane", "sphere"):
            ref = fc.contact_reference(case, axis, side, order, kind)
            share = float((ref.g < 0).mean())
            shares.append(share)
            min_g = min(min_g, float(np.abs(ref.g).min()))
            assert 0.15 <= share <= 0.85, (axis, side, kind, share)
            assert np.abs(ref.g).min() >= 1e-6
            assert ref.pressure.min() < 0 and ref.pressure.max() <= 0
            Cn, r, K, gap_norm = oracle_contact(case, axis, side, order, kind)
            assert np.array_equal(Cn.marked_nodes, ref.nodes)
            worst["pressure"] = max(worst["pressure"], rel(Cn.pressure, ref.pressure))
            worst["r"] = max(worst["r"], rel(r, ref.r))
            worst["K"] = max(worst["K"], rel(K, ref.K))
            worst["gap_norm"] = max(worst["gap_norm"], rel(gap_norm, ref.gap_norm))
            worst["area"] = max(worst["area"], rel(Cn.last_area, ref.last_area))
            worst["force"] = max(worst["force"], rel(Cn.last_force, ref.last_force))
            worst["last_pressure"] = max(worst["last_pressure"], rel(Cn.last_pressure, ref.last_pressure))
    report(f"{case} order {order}", share_min=min(shares), share_max=max(shares), min_abs_g=min_g, **worst)
    T = fc.TOL
    assert worst["pressure"] <= MARGIN * T["contact_pressure"] and worst["r"] <= MARGIN * T["contact_r"]
    assert worst["K"] <= MARGIN * T["contact_K"] and worst["gap_norm"] <= MARGIN * T["contact_gap_norm"]
    assert worst["area"] <= MARGIN * T["contact_area"] and worst["force"] <= MARGIN * T["contact_force"]
    assert worst["last_pressure"] <= MARGIN * T["contact_force"]


def inactive_and_active_faces(case, axis, side, order, kind):
    """(faces whose nodal pressures are all zero, faces with some pressure) of a contact case, by the product's face nodes"""
    from mimi_amd import splines
    ref = fc.contact_reference(case, axis, side, order, kind)
    dofs = splines.face_tables(fc.product_patch(case), axis, side, order)[0]
    p = ref.pressure.astype(np.float64)[np.searchsorted(ref.nodes, dofs)]
    active = (p != 0).any(axis=1)
    return int((~active).sum()), int(active.sum())


def test_contact_cases_hold_active_and_inactive_faces():
    """IsPressureZero (integrator_utils.cpp:112-119) skips a face whose nodal pressures are all zero: the cases must take
    both branches.  Every case has active faces; a face can only be inactive where no point under any of its nodes'
    supports penetrates, which the low-degree and C^0 patches allow."""
    with_inactive = []
    for case, order in CONTACT_CASES:
        for axis, side in fc.faces(case):
            for kind in ("plane", "sphere"):
                off, on = inactive_and_active_faces(case, axis, side, order, kind)
                assert on >= 1
                if off:
                    with_inactive.append((case, order, axis, side, kind))
    print("contact cases with inactive faces:", len(with_inactive), sorted({c[0] for c in with_inactive}))
    assert len({c[0] for c in with_inactive}) >= 3
