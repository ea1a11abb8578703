"""The three boundary integrators -- FollowerPressure (csrc/pressure.hip), CouplingSurface (csrc/surface.hip), MortarContact
(csrc/contact.hip) and the face layer they share (csrc/face_common.hpp, splines.face_tables through _capi.fill_face_tables)
-- on every face of the patches of tests/_patches.py (non-uniform and repeated knots, a different degree per axis, jittered
control points), on 2-D faces of degree 4, 5 and 7, and at quadrature orders of 1, 21, 25 and 64 points per face, against the
long-double reference of tests/_face_reference.py.  No expected value here comes from a face table; the inputs (tests/
_face_cases.py) and the reference are vetted without a GPU in tests/test_faces_cpu.py.

Bars (_face_cases.TOL), those the block tests hold these quantities to, relative to the largest reference entry: pressure
residual / area / force 1e-13, tangent 1e-12; surface positions and normals 1e-14, da and loads 1e-13; contact residual,
pressure, gap norm 1e-12, tangent 1e-11 (reference-FD mode 1e-4), area 1e-13, force and pressure integral 1e-11.

One case needs more than its bar, a finding and not a silent loosening: the unit normals of nonuni3d_p3 (degree 3, spans of 0.2
beside coordinates of 4) are held to 1e-13.  Measured 1.30e-14 on the MI355X (nonuni3d_p2: 8.5e-15, every other case <= 3.0e-15);
the tables alone, summed about the face's mean in doubles on the host, give 2.2e-15 there (tests/test_faces_cpu.py), the plain
double sum sum_a (X + u)_a dN_a the kernels and the block tests' restatement form gives 1.1e-14: terms of |x| p / h = 60 in a sum
of size 1.  Its positions meet 1e-14 (7.0e-16).

Worst figures measured on an MI355X over all cases, faces and orders: pressure residual 1.2e-15, tangent 3.8e-15, area 5.5e-16,
force 6.9e-16; closed surface net force 5.6e-17, column sums 3.5e-15, asymmetry 5.5e-15; surface positions 7.0e-16, da 2.7e-15,
load 1.9e-15; contact residual / pressure / gap norm / tangent / force 5.5e-14 (rep2d_p2, one point per face, sphere; <= 1.9e-14
elsewhere), area 4.8e-16, reference-FD tangent 2.6e-6; slabs against the whole face 3.9e-17 (pressure), 1.9e-16 (contact)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _face_cases as fc
import _face_reference as fr
import _patches

pytestmark = pytest.mark.gpu
T = fc.TOL
CASES = list(_patches.CASES)
ALL = [(c, -1) for c in CASES + fc.BLOCKS] + fc.ORDERS_ALL
N_Q = {1: 1, 9: 25, 15: 64, 41: 21}          # points per face of the non-default orders (3-D, 3-D, 3-D, 2-D)


def rel(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


def report(label, **figures):
    print(f"figures {label}: " + " ".join(f"{k}={v:.2e}" for k, v in figures.items()))


@functools.lru_cache(maxsize=None)
def pattern_of(case):
    """(CSRPattern, row of every entry) from the oracle's PrepareSparsity: valid for repeated knots and mixed degrees"""
    from mimi_amd.integrators import CSRPattern
    rowptr, col = fc.oracle_patch(case).sparsity()
    return CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), rowptr[-1]), np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def dense(case, values):
    pattern, _ = pattern_of(case)
    n = len(pattern.rowptr) - 1
    return sp.csr_matrix((values, pattern.col, pattern.rowptr), shape=(n, n)).toarray()


@functools.lru_cache(maxsize=None)
def prefill(case):
    pattern, _ = pattern_of(case)
    n = len(pattern.rowptr) - 1
    r0, A0 = np.random.default_rng(5).standard_normal(n), np.random.default_rng(6).standard_normal(pattern.nnz)
    r0.setflags(write=False)
    A0.setflags(write=False)
    return r0, A0


def assert_only_the_face_changed(case, nodes, r, A):
    """entries outside the rows / columns of the face nodes keep the bits of the pre-filled vectors"""
    pattern, entry_row = pattern_of(case)
    r0, A0 = prefill(case)
    dim = fc.product_patch(case).dim
    vd = (np.asarray(nodes)[:, None] * dim + np.arange(dim)).ravel()
    off = np.ones(len(r0), bool)
    off[vd] = False
    assert np.array_equal(r[off], r0[off])
    if A is not None:
        outside = off[entry_row] | off[pattern.col]
        assert np.array_equal(A[outside], A0[outside])


def expect_points(case, order):
    fb = fc.face_basis(case, 0, 0, order)
    if order in N_Q:
        assert fb.n_q_face == N_Q[order]
    return fb.n_q_face


# ---- follower pressure -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,order", ALL, ids=lambda c: str(c))
def test_follower_pressure(case, order):
    from mimi_amd.integrators import FollowerPressure
    B, u = fc.product_patch(case), fc.displacement(case)
    pattern, _ = pattern_of(case)
    r0, A0 = prefill(case)
    expect_points(case, order)
    worst = dict(r=0.0, K=0.0, area=0.0, force=0.0)
    for axis, side in fc.faces(case):
        fp = FollowerPressure("pressure", pattern, B, axis, side, quadrature_order=order).Prepare()
        nodes = fr.face_node_ids(B.n_ctrl, axis, side)
        assert np.array_equal(fp.FaceNodes(), nodes)
        for kind in ("uniform", "nodal"):
            ref = fc.pressure_reference(case, axis, side, order, kind)
            fp.SetPressure(ref.pressure)
            runs = []
            for _ in range(2):
                r, A = r0.copy(), A0.copy()
                fp.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
                fp.BoundaryPostTimeAdvance(u)
                runs.append((r, A, fp.last_area_, tuple(fp.last_force_)))
            r, A = runs[0][:2]
            assert np.array_equal(runs[1][0], r) and np.array_equal(runs[1][1], A) and runs[1][2:] == runs[0][2:]
            r2 = r0.copy()
            fp.AddBoundaryResidual(u, r2)
            assert np.array_equal(r2, r)
            assert_only_the_face_changed(case, nodes, r, A)
            worst["r"] = max(worst["r"], rel(r - r0, ref.r))
            worst["K"] = max(worst["K"], rel(dense(case, A - A0), fc.GRAD_FACTOR * ref.K))
            worst["area"] = max(worst["area"], rel(fp.last_area_, ref.area))
            worst["force"] = max(worst["force"], rel(fp.last_force_, ref.force))
    report(f"pressure {case} order {order}", **worst)
    assert worst["r"] <= T["pressure_r"] and worst["K"] <= T["pressure_K"]
    assert worst["area"] <= T["pressure_r"] and worst["force"] <= T["pressure_r"]


@pytest.mark.parametrize("case", CASES)
def test_uniform_pressure_on_the_closed_surface(case):
    """all 2 dim faces into one CSR: no net force, the column sums of every component zero (the block test's bars), and the
    summed tangent symmetric to 1e-11 of its largest entry -- uniform pressure on a closed surface has the potential p V"""
    from mimi_amd.integrators import FollowerPressure
    B, u = fc.product_patch(case), fc.displacement(case)
    dim = B.dim
    pattern, _ = pattern_of(case)
    r, A, abs_r = np.zeros(B.n_vdofs), np.zeros(pattern.nnz), np.zeros(B.n_vdofs)
    for axis, side in fc.faces(case):
        fp = FollowerPressure("pressure", pattern, B, axis, side).Prepare()
        fp.SetPressure(2.5)
        ri = np.zeros(B.n_vdofs)
        fp.AddBoundaryResidualAndGrad(u, 1.0, ri, A)
        r += ri
        abs_r += np.abs(ri)
    M = dense(case, A)
    net = max(abs(r.reshape(-1, dim)[:, i].sum()) for i in range(dim)) / abs_r.sum()
    cols = max(np.abs(M[i::dim].sum(axis=0)).max() for i in range(dim)) / np.abs(A).max()
    skew = np.abs(M - M.T).max() / np.abs(M).max()
    report(f"closed {case}", net=net, cols=cols, skew=skew)
    assert np.abs(r).max() > 0 and net <= 1e-12 and cols <= 1e-11 and skew <= 1e-11


# ---- coupling surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,order", ALL, ids=lambda c: str(c))
def test_coupling_surface(case, order):
    from mimi_amd.integrators import CouplingSurface
    B, u = fc.product_patch(case), fc.displacement(case).copy()
    n_q = expect_points(case, order)
    base = prefill(case)[0]
    worst = dict(x=0.0, n=0.0, da=0.0, load=0.0)
    for axis, side in fc.faces(case):
        s = CouplingSurface(B, axis, side, quadrature_order=order).Prepare()
        ref = fc.surface_reference(case, axis, side, order)
        assert s.n_q_ == n_q and s.n_points_ == s.n_faces_ * n_q == len(ref.pts.x)
        x, n, w = [t.cpu().numpy() for t in s.points(u)]
        perm, _ = fr.match_points(ref.pts.x, x)
        worst["x"] = max(worst["x"], rel(x[perm], ref.pts.x))
        worst["n"] = max(worst["n"], float(np.abs(n[perm] - ref.pts.n.astype(np.float64)).max()))
        worst["da"] = max(worst["da"], rel(w[perm], ref.pts.da))
        t = np.empty_like(ref.t)
        t[perm] = ref.t
        loads = []
        for _ in range(2):
            out = base.copy()
            s.AddLoad(u, t, out)
            loads.append(out)
        assert np.array_equal(loads[0], loads[1])
        assert_only_the_face_changed(case, fr.face_node_ids(B.n_ctrl, axis, side), loads[0], None)
        worst["load"] = max(worst["load"], rel(loads[0] - base, ref.load))
        s.set_traction(t, u)
        assert np.array_equal(base + s.load_.cpu().numpy(), loads[0])
    report(f"surface {case} order {order}", **worst)
    assert worst["x"] <= T["surface_x"] and worst["n"] <= fc.tol(case, "surface_n")
    assert worst["da"] <= T["surface_da"] and worst["load"] <= T["surface_load"]


# ---- mortar contact --------------------------------------------------------------------------------------------------------
def contact_handle(case, axis, side, order, kind, **kw):
    from mimi_amd.integrators import MortarContact
    body = fc.product_body(fc.body(case, axis, side, order, kind))
    return MortarContact(body, "contact", pattern_of(case)[0], fc.product_patch(case), axis, side, quadrature_order=order, **kw).Prepare()


def history(G, u):
    G.BoundaryPostTimeAdvance(u)
    return G.last_area_, tuple(G.last_force_), G.last_pressure_, G.GapNorm(u), G.AveragePressure().tobytes()


@pytest.mark.parametrize("kind", ["plane", "sphere"])
@pytest.mark.parametrize("case,order", ALL + fc.ORDERS_CONTACT, ids=lambda c: str(c))
def test_mortar_contact(case, order, kind):
    B, u = fc.product_patch(case), fc.displacement(case)
    r0, A0 = prefill(case)
    expect_points(case, order)
    worst = dict(r=0.0, pressure=0.0, gap_norm=0.0, K=0.0, area=0.0, force=0.0, last_pressure=0.0)
    for axis, side in fc.faces(case):
        ref = fc.contact_reference(case, axis, side, order, kind)
        G = contact_handle(case, axis, side, order, kind)
        assert np.array_equal(G.MarkedNodes(), ref.nodes)
        runs = []
        for _ in range(2):
            r, A = r0.copy(), A0.copy()
            G.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
            runs.append((r, A, history(G, u)))
        r, A = runs[0][:2]
        assert np.array_equal(runs[1][0], r) and np.array_equal(runs[1][1], A) and runs[1][2] == runs[0][2]
        r2 = r0.copy()
        G.AddBoundaryResidual(u, r2)
        assert np.array_equal(r2, r) and history(G, u) == runs[0][2]
        assert_only_the_face_changed(case, ref.nodes, r, A)
        worst["r"] = max(worst["r"], rel(r - r0, ref.r))
        worst["K"] = max(worst["K"], rel(dense(case, A - A0), ref.K))
        worst["pressure"] = max(worst["pressure"], rel(G.AveragePressure(), ref.pressure))
        worst["gap_norm"] = max(worst["gap_norm"], rel(G.GapNorm(u), ref.gap_norm))
        worst["area"] = max(worst["area"], rel(G.last_area_, ref.last_area))
        worst["force"] = max(worst["force"], rel(G.last_force_, ref.last_force))
        worst["last_pressure"] = max(worst["last_pressure"], rel(G.last_pressure_, ref.last_pressure))
    report(f"contact {case} order {order} {kind}", **worst)
    assert worst["r"] <= T["contact_r"] and worst["pressure"] <= T["contact_pressure"] and worst["gap_norm"] <= T["contact_gap_norm"]
    assert worst["K"] <= T["contact_K"] and worst["area"] <= T["contact_area"]
    assert worst["force"] <= T["contact_force"] and worst["last_pressure"] <= T["contact_force"]


@pytest.mark.parametrize("case", ["rep2d_p3", "mix3d_211"])
def test_mortar_contact_reference_fd_tangent(case):
    """MIMI_HIP_TANGENT_REFERENCE_FD (mortar_contact.cpp:263-295) against the reference's exact frozen-pressure tangent"""
    u = fc.displacement(case)
    r0, A0 = prefill(case)
    worst = 0.0
    for axis, side in fc.faces(case):
        ref = fc.contact_reference(case, axis, side, -1, "sphere")
        G = contact_handle(case, axis, side, -1, "sphere")
        G.SetTangentMode(1)
        r, A = r0.copy(), A0.copy()
        G.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
        assert rel(r - r0, ref.r) <= T["contact_r"]
        assert_only_the_face_changed(case, ref.nodes, r, A)
        worst = max(worst, rel(dense(case, A - A0), ref.K))
    report(f"contact fd {case}", K=worst)
    assert worst <= T["contact_K_fd"]


# ---- create-time refusals --------------------------------------------------------------------------------------------------
def test_refusals_of_face_sizes_and_a_valid_handle_after_each():
    import mimi_amd
    from mimi_amd.integrators import CouplingSurface, CSRPattern, FollowerPressure, MortarContact, RigidPlane
    wide = mimi_amd.BSplinePatch.block((1, 1, 1), (4, 4, 1))                # the face {xi_2 = 1} has 25 nodes
    pattern = CSRPattern.of_bspline_patch(wide)
    plane = RigidPlane([0.5, 0.5, 0.9], [0.0, 0.0, -1.0], 1e4)
    u = np.zeros(wide.n_vdofs)
    for make, run in (
            (lambda axis, **kw: FollowerPressure("pressure", pattern, wide, axis, 1, **kw), lambda h, r: h.AddBoundaryResidual(u, r)),
            (lambda axis, **kw: MortarContact(plane, "contact", pattern, wide, axis, 1, **kw), lambda h, r: h.AddBoundaryResidual(u, r)),
            (lambda axis, **kw: CouplingSurface(wide, axis, 1, **kw), lambda h, r: h.AddLoad(u, np.ones((h.n_points_, 3)), r))):
        with pytest.raises(RuntimeError, match=r"face n_dof 25 out of range \[1,16\]"):
            make(2).Prepare()
        h = make(0, quadrature_order=5).Prepare()                           # 10 nodes, 9 points
        if isinstance(h, FollowerPressure):
            h.SetPressure(1.0)
        r = np.zeros(wide.n_vdofs)
        run(h, r)
        if not isinstance(h, MortarContact):                                # (the plane does not reach the face xi_0 = 1)
            assert np.abs(r).max() > 0
    case = "mix3d_211"
    B, u = fc.product_patch(case), fc.displacement(case).copy()
    pattern = pattern_of(case)[0]
    with pytest.raises(RuntimeError, match=r"face quadrature points 36 out of range \[1,25\]"):
        FollowerPressure("pressure", pattern, B, 2, 1, quadrature_order=11).Prepare()
    with pytest.raises(RuntimeError, match=r"face quadrature points 36 out of range \[1,25\]"):
        CouplingSurface(B, 2, 1, quadrature_order=11).Prepare()
    with pytest.raises(RuntimeError, match=r"face quadrature points 81 out of range \[1,64\]"):
        contact_handle(case, 2, 1, 17, "plane")
    fp = FollowerPressure("pressure", pattern, B, 2, 1).Prepare()
    fp.SetPressure(fc.UNIFORM_P)
    r = np.zeros(B.n_vdofs)
    fp.AddBoundaryResidual(u, r)
    assert rel(r, fc.pressure_reference(case, 2, 1, -1, "uniform").r) <= T["pressure_r"]
    G = contact_handle(case, 2, 1, -1, "plane")
    r = np.zeros(B.n_vdofs)
    G.AddBoundaryResidual(u, r)
    assert rel(r, fc.contact_reference(case, 2, 1, -1, "plane").r) <= T["contact_r"]
    s = CouplingSurface(B, 2, 1).Prepare()
    assert rel(s.points(u)[2].cpu().numpy().sum(), fc.points(case, 2, 1).da.sum()) <= T["surface_da"]


# ---- element slabs on repeated knots ---------------------------------------------------------------------------------------
SLABS = [("rep3d_p2", 2, 0), ("rep2d_p3", 1, 0)]       # (case, face axis, tangential axis with a repeated knot that is cut)


def slab_boxes(B, cut_axis):
    m = B.n_spans[cut_axis]
    for b0, e0 in ((0, m // 2), (m // 2, m)):
        begin, end = [0, 0, 0], list(B.n_spans) + [1] * (3 - B.dim)
        begin[cut_axis], end[cut_axis] = b0, e0
        yield begin, end


@pytest.mark.parametrize("case,axis,cut_axis", SLABS)
def test_pressure_slabs_sum_to_the_whole_face(case, axis, cut_axis):
    """the assertion of test_pressure_gpu.py::test_element_slabs_sum_to_the_whole_face; the whole face against the reference"""
    from mimi_amd.integrators import FollowerPressure
    B, u = fc.product_patch(case), fc.displacement(case)
    pattern = pattern_of(case)[0]
    ref = fc.pressure_reference(case, axis, 1, -1, "nodal")
    whole = FollowerPressure("pressure", pattern, B, axis, 1).Prepare()
    whole.SetPressure(ref.pressure)
    r, A = np.zeros(B.n_vdofs), np.zeros(pattern.nnz)
    whole.AddBoundaryResidualAndGrad(u, 1.0, r, A)
    assert rel(r, ref.r) <= T["pressure_r"] and rel(dense(case, A), ref.K) <= T["pressure_K"]
    r2, A2 = np.zeros_like(r), np.zeros_like(A)
    for box in slab_boxes(B, cut_axis):
        part = FollowerPressure("pressure", pattern, B, axis, 1, element_box=box).Prepare()
        assert 0 < part.n_faces_ < whole.n_faces_
        part.SetPressure(ref.pressure[np.searchsorted(ref.nodes, part.FaceNodes())])
        part.AddBoundaryResidualAndGrad(u, 1.0, r2, A2)
    report(f"pressure slabs {case}", r=rel(r2, r), A=rel(A2, A))
    assert np.abs(r2 - r).max() <= 1e-15 * np.abs(r).max()
    assert np.abs(A2 - A).max() <= 1e-15 * np.abs(A).max()


@pytest.mark.parametrize("case,axis,cut_axis", SLABS)
def test_contact_slabs_sum_to_the_whole_face(case, axis, cut_axis):
    """element slabs of the contact face as ShardedContact runs them: pass 1 per slab, the nodal area / gap summed over the
    slabs, pass 2 per slab from the sums; the whole face against the reference"""
    B, u = fc.product_patch(case), fc.displacement(case)
    pattern = pattern_of(case)[0]
    ref = fc.contact_reference(case, axis, 1, -1, "sphere")
    whole = contact_handle(case, axis, 1, -1, "sphere")
    r, A = np.zeros(B.n_vdofs), np.zeros(pattern.nnz)
    whole.AddBoundaryResidualAndGrad(u, fc.GRAD_FACTOR, r, A)
    assert rel(r, ref.r) <= T["contact_r"] and rel(dense(case, A), ref.K) <= T["contact_K"]
    parts = [contact_handle(case, axis, 1, -1, "sphere", element_box=box) for box in slab_boxes(B, cut_axis)]
    total = np.zeros((2, len(ref.nodes)))
    slots = []
    for part in parts:
        assert 0 < part.n_marked_boundaries_ < whole.n_marked_boundaries_
        slots.append(np.searchsorted(ref.nodes, part.MarkedNodes()))
        area, gap = np.zeros(len(slots[-1])), np.zeros(len(slots[-1]))
        part.GapArea(u)
        part.GetNodal(area, gap)
        total[0, slots[-1]] += area
        total[1, slots[-1]] += gap
    assert rel(total[0], ref.area) <= T["contact_area"] and rel(total[1], ref.gap) <= T["contact_pressure"]
    r2, A2 = np.zeros_like(r), np.zeros_like(A)
    for part, slot in zip(parts, slots):
        part.SetNodal(total[0, slot].copy(), total[1, slot].copy())
        part.AddBoundaryResidualFromNodal(u, fc.GRAD_FACTOR, r2, A2)
    report(f"contact slabs {case}", r=rel(r2, r), A=rel(A2, A))
    assert np.abs(r2 - r).max() <= 1e-15 * np.abs(r).max()
    assert np.abs(A2 - A).max() <= 1e-15 * np.abs(A).max()
