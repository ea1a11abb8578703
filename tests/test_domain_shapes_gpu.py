"""The domain integrator (through the C ABI) on patches that are not Patch.block -- non-uniform knots, repeated interior knots,
a different degree per axis, quadrature orders other than the default -- and on flat tables of 25, 36 and 64 nodes per
element, against the oracle on the same inputs (tests/_patches.py; the inputs themselves are vetted without a GPU in
tests/test_domain_shapes_cpu.py).  Every assembly asserts the kernel family it ran on.  The oracle is not the only reference
under these inhomogeneous fields: tests/test_domain_reference_gpu.py holds the same kernel families to the long-double element
sum of tests/_domain_reference.py, and tests/test_domain_reference_cpu.py pins the oracle to it.

Bars, those of test_domain_gpu.py / test_materials_gpu.py / test_fields_gpu.py: residual 1e-12 relative (max-norm); analytic
tangent 1e-11 (1e-10 for the record materials); reference-FD tangent 5e-4; committed state rtol 1e-9, atol 1e-13; temperature
1e-12; fields 1e-11."""
import numpy as np
import pytest

import _fields
import _patches
from _cases import product_material
from _patches import DT, GRAD_FACTOR

pytestmark = pytest.mark.gpu


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def tangent_bar(matname):
    return 1e-10 if matname == "j2simo" else 1e-11


def oracle_pattern(D):
    from mimi_amd.integrators import CSRPattern
    return CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)


def bspline_handle(B, D, matname, **kw):
    from mimi_amd.integrators import NonlinearSolid
    pattern = kw.pop("pattern", None) or oracle_pattern(D)
    G = NonlinearSolid("domain", product_material(matname), pattern, patch=B, **kw).Prepare()
    G.dt_ = DT
    return G


def tables_handle(D, matname, with_N=False):
    from mimi_amd.integrators import NonlinearSolid
    P = D.patch
    tables = dict(dim=P.dim, n_nodes=P.n_nodes, dofs=D.conn, dN_dX=D.dN_dX, weight_det=D.weight * D.det)
    if with_N:
        tables["N"] = D.tables["N"]
    G = NonlinearSolid("domain", product_material(matname), oracle_pattern(D), tables=tables).Prepare()
    G.dt_ = DT
    return G


def commit_and_compare(G, ref, select=None):
    """DomainPostTimeAdvance(u0) as the oracle did, and the committed state against the oracle's (of the elements `select`)"""
    D = ref.D
    if not D.has_states:
        return
    G.DomainPostTimeAdvance(ref.u0)
    pick = (lambda a: a) if select is None else (lambda a: a[select])
    assert D.eqps.max() > 1e-4
    assert np.allclose(G.State("accumulated_plastic_strain"), pick(D.eqps), rtol=1e-9, atol=1e-13)
    assert np.allclose(G.State("temperature"), pick(D.temperature), rtol=1e-12, atol=1e-12)
    assert np.allclose(G.State("plastic_strain"), pick(D.plastic_strain), rtol=1e-9, atol=1e-13)
    if G.material_._kind == 4:      # J2Simo: the second state matrix
        assert np.allclose(G.State("state2"), pick(D.state2), rtol=1e-9, atol=1e-13)


def check_assemblies(G, ref, matname, family, label):
    """residual-only, then residual + tangent twice, all in accumulate form on random r0 / A0: the increments against the
    oracle's, the family of every call, the two tangent assemblies bit-equal"""
    n, nnz = ref.r.size, ref.A.size
    r0 = np.random.default_rng(3).standard_normal(n)
    A0 = np.random.default_rng(4).standard_normal(nnz)
    r_g = r0.copy()
    G.AddDomainResidual(ref.u, r_g)
    assert G.LastKernelFamily() == family
    e_r0 = relmax(r_g - r0, ref.r0)
    runs = []
    for _ in range(2):
        r_g, A_g = r0.copy(), A0.copy()
        G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
        assert G.LastKernelFamily() == family
        runs.append((r_g, A_g))
    e_r, e_A = relmax(runs[0][0] - r0, ref.r), relmax(runs[0][1] - A0, ref.A)
    print(f"{label} {matname} [{family}]: residual-only {e_r0:.2e} residual {e_r:.2e} tangent {e_A:.2e}")
    assert e_r0 < 1e-12 and e_r < 1e-12
    assert e_A < tangent_bar(matname)
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][0], runs[1][0])


# ---- a. residual, residual + tangent, state commit ------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", _patches.PARITY, ids=lambda v: v)
def test_residual_tangent_and_commit_parity(case, matname):
    ref = _patches.reference(case, matname)
    P, B = _patches.patches(case)
    G = bspline_handle(B, ref.D, matname)
    family = _patches.family_of(case)
    assert G.path_ == (0 if family == "general" else 1)
    assert (G.n_elements_, G.n_quad_, G.n_dof_) == (P.n_el, ref.D.weight.shape[1], P.n_dof)
    commit_and_compare(G, ref)
    check_assemblies(G, ref, matname, family, case)


# ---- b. the reference's forward-difference tangent ------------------------------------------------------------------------
FD_CASES = [c for c in _patches.CASES if c != "nonuni3d_p2"]      # (at most 32 elements)


@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case", FD_CASES)
def test_reference_fd_tangent_parity(case, matname):
    P, B = _patches.patches(case)
    assert P.n_el <= 32
    ref = _patches.reference_fd(case, matname)
    G = bspline_handle(B, ref.D, matname)
    commit_and_compare(G, ref)
    G.SetTangentMode(1)
    r0 = np.random.default_rng(3).standard_normal(P.n_vdofs)
    A0 = np.random.default_rng(4).standard_normal(ref.D.nnz)
    r_g, A_g = r0.copy(), A0.copy()
    G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
    assert G.LastKernelFamily() == "general"            # (the GRAD == 2 kernel, whatever the handle's route)
    e_r, e_A = relmax(r_g - r0, ref.r), relmax(A_g - A0, ref.A)
    print(f"{case} {matname}: FD mode residual {e_r:.2e} tangent {e_A:.2e}")
    assert e_r < 1e-12
    # (forward differences with steps down to 1e-10 on both sides: see test_domain_gpu.py)
    assert e_A < 5e-4
    # and back: the analytic tangent of the handle's own route
    G.SetTangentMode(0)
    r_g, A_g = r0.copy(), A0.copy()
    G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
    assert G.LastKernelFamily() == _patches.family_of(case)


# ---- c. quadrature order -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case,order,n_quad", _patches.ORDERS, ids=lambda v: str(v))
def test_quadrature_orders(case, order, n_quad, matname):
    ref = _patches.reference(case, matname, order)
    P, B = _patches.patches(case)
    G = bspline_handle(B, ref.D, matname, quadrature_order=order)
    assert G.n_quad_ == n_quad == ref.D.weight.shape[1]
    assert G.path_ == 0
    commit_and_compare(G, ref)
    check_assemblies(G, ref, matname, "general", f"{case} order {order}")


def test_sizes_out_of_range_are_refused():
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    mat = product_material("neohook")
    P, B = _patches.patches("nonuni3d_p3")
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), int(rowptr[-1]))
    with pytest.raises(RuntimeError, match="n_quad 216"):          # order 11: 6^3 points, the limit is 125
        NonlinearSolid("domain", mat, pattern, patch=B, quadrature_order=11).Prepare()
    NonlinearSolid("domain", mat, pattern, patch=B, quadrature_order=9).Prepare()      # 125 points: taken
    p4 = mimi_amd.BSplinePatch.block((2, 2), 4)
    with pytest.raises(RuntimeError, match="degree 4 unsupported"):
        NonlinearSolid("domain", mat, CSRPattern.of_bspline_patch(p4), patch=p4).Prepare()
    mixed = mimi_amd.BSplinePatch.block((2, 2, 2), (2, 4, 1))
    with pytest.raises(RuntimeError, match="degree 4 unsupported"):
        NonlinearSolid("domain", mat, CSRPattern.of_bspline_patch(mixed), patch=mixed).Prepare()
    tables = dict(dim=2, n_nodes=65, dofs=np.arange(65, dtype=np.int32)[None, :], dN_dX=np.zeros((1, 1, 2, 65)),
                  weight_det=np.ones((1, 1)))
    dense = CSRPattern(np.arange(131, dtype=np.int64) * 130, np.tile(np.arange(130, dtype=np.int32), 130), 130 * 130)
    with pytest.raises(RuntimeError, match="n_dof 65 out of range"):
        NonlinearSolid("domain", mat, dense, tables=tables).Prepare()


# ---- d. flat tables of 25, 36 and 64 nodes per element ---------------------------------------------------------------------
@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("n_el,p", _patches.BLOCKS, ids=lambda v: str(v))
def test_flat_tables_of_high_degree(n_el, p, matname):
    """2-D degree 4 (25 nodes: the 256-thread kernel), 5 and 7 (36 and 64 nodes: the 512-thread vector-pipe kernel)"""
    ref = _patches.block_reference(n_el, p, matname)
    G = tables_handle(ref.D, matname)
    assert G.path_ == 0 and (G.n_dof_, G.n_quad_) == ((p + 1) ** 2, (p + 2) ** 2)
    commit_and_compare(G, ref)
    check_assemblies(G, ref, matname, "general", f"block {n_el} p{p}")


# ---- e. the caller's CSR ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case", ["rep3d_p2", "mix3d_231"])
def test_closed_form_window_pattern(case, matname):
    """CSRPattern.of_bspline_patch: the (2 p + 1) window per axis.  With a doubled knot it is strictly wider than the union
    of the element blocks; the assembly fills the entries of that union and leaves the rest of A alone."""
    from mimi_amd.integrators import CSRPattern
    ref = _patches.reference(case, matname)
    P, B = _patches.patches(case)
    D = ref.D
    pat = CSRPattern.of_bspline_patch(B)
    if case == "rep3d_p2":
        assert pat.nnz > D.nnz
    else:
        assert pat.nnz == D.nnz
    n = P.n_vdofs
    key_pat = np.repeat(np.arange(n, dtype=np.int64), np.diff(pat.rowptr)) * n + pat.col
    key_o = np.repeat(np.arange(n, dtype=np.int64), np.diff(D.rowptr)) * n + D.col
    assert np.all(np.diff(key_pat) > 0)
    dst = np.searchsorted(key_pat, key_o)
    assert np.array_equal(key_pat[dst], key_o)            # every entry of the oracle's pattern is in the window pattern
    G = bspline_handle(B, D, matname, pattern=pat)
    assert G.path_ == 0 and G.nnz_ == pat.nnz
    commit_and_compare(G, ref)
    r0 = np.random.default_rng(3).standard_normal(n)
    A0 = np.random.default_rng(4).standard_normal(pat.nnz)      # garbage
    r_g, A_g = r0.copy(), A0.copy()
    G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
    assert G.LastKernelFamily() == "general"
    assert relmax(r_g - r0, ref.r) < 1e-12
    assert relmax((A_g - A0)[dst], ref.A) < 1e-11
    other = np.ones(pat.nnz, dtype=bool)
    other[dst] = False
    assert other.sum() == pat.nnz - D.nnz
    assert np.array_equal(A_g[other], A0[other])


# ---- f. element boxes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case,axis,cut", [("rep3d_p2", 0, 2), ("rep2d_p2", 0, 3), ("mix3d_322", 2, 1)])
def test_element_boxes_add_up_to_the_whole(case, axis, cut, matname):
    """two boxes [0, cut) and [cut, m) along `axis`: box_begin + el indexes first[]; on rep3d_p2 and rep2d_p2 the second box
    starts at a span whose first function is not the span's index"""
    ref = _patches.reference(case, matname)
    P, B = _patches.patches(case)
    family = _patches.family_of(case)
    if case.startswith("rep"):
        assert P.spans[axis][cut] - P.p[axis] != cut
    em = P.element_multi_index()
    r_g, A_g, r_only = np.zeros(P.n_vdofs), np.zeros(ref.D.nnz), np.zeros(P.n_vdofs)
    for b, e in ((0, cut), (cut, P.m[axis])):
        begin, end = [0, 0, 0], list(P.m) + [1] * (3 - P.dim)
        begin[axis], end[axis] = b, e
        G = bspline_handle(B, ref.D, matname, element_box=(begin, end))
        assert G.path_ == (0 if family == "general" else 1)
        own = np.nonzero((em[axis] >= b) & (em[axis] < e))[0]
        assert G.n_elements_ == len(own)
        commit_and_compare(G, ref, select=own)
        G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
        assert G.LastKernelFamily() == family
        G.AddDomainResidual(ref.u, r_only)
        assert G.LastKernelFamily() == family
    assert relmax(r_g, ref.r) < 1e-12
    assert relmax(A_g, ref.A) < 1e-11
    assert relmax(r_only, ref.r0) < 1e-12


# ---- g. permuted node numbering ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case", ["rep3d_p2", "mix3d_221"])
def test_permuted_node_numbering(case, matname):
    """node_ids = lexicographic -> caller's node id, as in test_domain_gpu.py: u, r and the CSR in the caller's numbering; a
    doubled knot / mixed degrees keep the handle on the general kernels"""
    import scipy.sparse as sp
    ref = _patches.reference(case, matname)
    P, B = _patches.patches(case)
    D = ref.D
    perm = np.random.default_rng(11).permutation(P.n_nodes).astype(np.int64)
    dofperm = (perm[:, None] * 3 + np.arange(3)[None, :]).ravel()          # lexicographic dof -> caller's dof
    rows_o = np.repeat(np.arange(P.n_vdofs), np.diff(D.rowptr))
    S = sp.coo_matrix((np.arange(1, D.nnz + 1, dtype=np.float64), (dofperm[rows_o], dofperm[D.col])),
                      shape=(P.n_vdofs, P.n_vdofs)).tocsr()
    S.sort_indices()
    dst = np.empty(D.nnz, dtype=np.int64)
    dst[(S.data - 1).astype(np.int64)] = np.arange(D.nnz)
    from mimi_amd.integrators import CSRPattern
    pattern = CSRPattern(S.indptr.astype(np.int64), S.indices.astype(np.int32), D.nnz)
    G = bspline_handle(B, D, matname, pattern=pattern, node_ids=perm)
    assert G.path_ == 0
    u_p, u0_p = np.empty_like(ref.u), np.empty_like(ref.u0)
    u_p[dofperm], u0_p[dofperm] = ref.u, ref.u0
    if D.has_states:
        G.DomainPostTimeAdvance(u0_p)
        assert np.allclose(G.State("accumulated_plastic_strain"), D.eqps, rtol=1e-9, atol=1e-13)
    r_g, A_g = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    G.AddDomainResidualAndGrad(u_p, GRAD_FACTOR, r_g, A_g)
    assert G.LastKernelFamily() == "general"
    assert relmax(r_g[dofperm], ref.r) < 1e-12
    assert relmax(A_g[dst], ref.A) < 1e-11
    r_g[:] = 0.0
    G.AddDomainResidual(u_p, r_g)
    assert G.LastKernelFamily() == "general"
    assert relmax(r_g[dofperm], ref.r0) < 1e-12


# ---- h. field output -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case", ["rep2d_p2", "mix3d_231"])
def test_field_output(case, matname):
    """rep2d_p2: the tensor field kernel with first != span (no per-point table is built); mix3d_231: the general field
    kernel and the shape values expanded from the 1-D tables.  Bars of test_fields_gpu.py (1e-11)."""
    ref = _patches.reference(case, matname)
    P, B = _patches.patches(case)
    D = ref.D
    G = bspline_handle(B, D, matname)
    commit_and_compare(G, ref)
    pts = _fields.point_fields(D, ref.u, DT)
    for name in _fields.FIELDS:
        if name not in pts:
            with pytest.raises(RuntimeError, match="no state"):
                G.PointField(name, None)
            continue
        a = G.PointField(name, ref.u)
        assert a.shape == pts[name].shape
        s_o, w_o = _fields.nodal_sums(D.tables, P.n_nodes, pts[name])
        s, w = np.zeros_like(s_o), np.zeros_like(w_o)
        G.NodalField(name, ref.u, s, w)
        e_pt, e_s, e_w = relmax(a, pts[name]), relmax(s, s_o), relmax(w, w_o)
        print(f"{case} {matname} {name}: points {e_pt:.2e} nodal sum {e_s:.2e} weight {e_w:.2e}")
        assert e_pt <= 1e-11 and e_s <= 1e-11 and e_w <= 1e-11
        assert w.min() > 0
        if name in ("accumulated_plastic_strain", "temperature"):
            assert np.array_equal(a[..., 0], G.State(name))
    if case == "rep2d_p2":
        assert G.path_ == 1 and not G.HoldsGradientTables()
    else:
        assert G.path_ == 0
