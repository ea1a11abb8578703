"""The mass, damping and body-force forms on the device (mimi_hip_domain_add_mass / _add_diffusion / _add_body_force,
csrc/kernels_forms.hpp) and the facade's set-up in HBM (mimi_amd/solid.py).

References, all CPU code: oracle.harness.assemble_mass / assemble_viscosity / assemble_body_force on any pattern, and the
facade's host pass.  Tolerance of every comparison: 1e-13 x the largest absolute reference entry -- what
tests/test_solid_setup_cpu.py uses between those two references, about 20 x their worst disagreement (4.2e-15)."""
import functools
import os
import types

import numpy as np
import pytest

import _patches
from _cases import oracle_material, product_material

pytestmark = pytest.mark.gpu

TOL = 1e-13
RHO, NU, B3 = 1.7, 0.3, np.array([0.4, -9.81, 2.5])
BLOCKS = [((5, 4, 3), 2), ((4, 3, 3), 3), ((7, 5), 2), ((3, 2, 2), 1),
          ((1, 1, 1), 2), ((2, 1, 3), 2), ((1, 2, 1), 3), ((3, 1), 2), ((1, 1), 1)]


def close(got, ref):
    err, bound = np.abs(got - ref).max(), TOL * np.abs(ref).max()
    print(f"max |got - ref| = {err:.3e}, bound {bound:.3e}")
    return err <= bound


def oracle_forms(P):
    """the three references of an oracle patch on its own pattern, from zero; computed once per patch by the callers"""
    from oracle import harness as hz, ref_path as rp
    D = rp.DomainOracle(P, oracle_material("neohook"), n_threads=2)
    b = B3[:P.dim]
    ref = types.SimpleNamespace(P=P, D=D, b=b, M=hz.assemble_mass(P, D.tables, RHO, D.rowptr, D.col),
                                C=hz.assemble_viscosity(P, D.tables, NU, D.rowptr, D.col),
                                f=hz.assemble_body_force(P, D.tables, b),
                                volume=float((D.tables["weight"] * D.tables["det"]).sum()))
    for a in (ref.M, ref.C, ref.f):
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def block_ref(n_el, p):
    from oracle import iga
    return oracle_forms(iga.Patch.block(n_el, p))


@functools.lru_cache(maxsize=None)
def case_ref(case):
    return oracle_forms(_patches.patches(case)[0])


@functools.lru_cache(maxsize=None)
def rational_ref(tensor_product):
    """the patches of test_domain_gpu.py::test_tensor_product_nurbs_weights / ::test_rational_weights_general_path"""
    from oracle import iga
    n_el, p = (4, 3, 3), 2
    P0 = iga.Patch.block(n_el, p)
    if tensor_product:
        rng = np.random.default_rng(5)
        w1d = [1.0 + 0.4 * rng.uniform(-1, 1, n) for n in P0.n]
        w = w1d[0]
        for d in range(1, len(n_el)):
            w = np.multiply.outer(w1d[d], w)
        weights = 0.7 * w.ravel()
    else:
        rng = np.random.default_rng(21)
        weights = 1.0 + 0.3 * rng.uniform(-1, 1, P0.n_nodes)
    ctrl = np.asarray(P0.ctrl, dtype=np.float64).reshape(P0.n_nodes, -1) + 0.05 * rng.standard_normal((P0.n_nodes, len(n_el)))
    return oracle_forms(iga.Patch(P0.p, P0.knots, ctrl, weights))


def pattern_of(D):
    from mimi_amd.integrators import CSRPattern
    return CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)


def product_patch(P):
    import mimi_amd
    ctrl = np.asarray(P.ctrl, dtype=np.float64).reshape(P.n_nodes, -1)
    return mimi_amd.BSplinePatch(P.p, P.knots, ctrl, None if np.all(P.weights == 1.0) else P.weights)


def patch_handle(ref, **kw):
    from mimi_amd.integrators import NonlinearSolid
    return NonlinearSolid("domain", product_material("neohook"), kw.pop("pattern", None) or pattern_of(ref.D),
                          patch=product_patch(ref.P), **kw).Prepare()


def flat_handle(ref, patch=None, shape_values=True):
    """the flat-table creator; tables (and N) from solid._element_tables when the product patch is given, the oracle's
    otherwise (a patch the B-spline tables cannot describe)"""
    from mimi_amd import solid
    from mimi_amd.integrators import NonlinearSolid
    P, D = ref.P, ref.D
    if patch is not None:
        N, wd, conn, dN_dX = solid._element_tables(patch, with_gradients=True)
        t = dict(dim=P.dim, n_nodes=P.n_nodes, dofs=conn.astype(np.int32), dN_dX=np.ascontiguousarray(dN_dX),
                 weight_det=np.ascontiguousarray(wd))
    else:
        N = D.tables["N"]
        t = dict(dim=P.dim, n_nodes=P.n_nodes, dofs=D.conn, dN_dX=D.dN_dX, weight_det=D.weight * D.det)
    if shape_values:
        t["N"] = np.ascontiguousarray(N)
    return NonlinearSolid("domain", product_material("neohook"), pattern_of(D), tables=t).Prepare()


def forms(G, ref, M=None, C=None, f=None):
    M = np.zeros(ref.D.nnz) if M is None else M
    C = np.zeros(ref.D.nnz) if C is None else C
    f = np.zeros(ref.P.n_vdofs) if f is None else f
    G.AddMass(RHO, M)
    G.AddDiffusion(NU, C)
    G.AddBodyForce(ref.b, f)
    return M, C, f


def check_parity(G, ref):
    M, C, f = forms(G, ref)
    assert close(M, ref.M)
    assert close(C, ref.C)
    assert close(f, ref.f)


def tensor_usable(G):
    """the handle's assemblies run on a tensor kernel family (domain_dispatch.hpp): then the forms must not have built the
    per-point gradient tables"""
    u, r = np.zeros(G.n_vdofs_), np.zeros(G.n_vdofs_)
    G.AddDomainResidual(u, r)
    return G.LastKernelFamily() != "general"


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_el,p", BLOCKS, ids=lambda v: str(v).replace(" ", ""))
def test_parity_on_blocks(n_el, p):
    ref = block_ref(n_el, p)
    G = patch_handle(ref)
    held = G.HoldsGradientTables()
    check_parity(G, ref)
    assert G.path_ == 1 and G.HoldsGradientTables() == held and not held


@pytest.mark.parametrize("creator", ["patch", "flat"])
@pytest.mark.parametrize("case", list(_patches.CASES))
def test_parity_on_non_block_patches(case, creator):
    ref = case_ref(case)
    if creator == "flat":
        check_parity(flat_handle(ref, _patches.patches(case)[1]), ref)
        return
    G = patch_handle(ref)
    held = G.HoldsGradientTables()
    check_parity(G, ref)
    if _patches.family_of(case) != "general":
        assert not held and not G.HoldsGradientTables()     # mimi_hip_domain_info(h, 8): still no per-point gradient table
        assert tensor_usable(G)


def test_parity_with_tensor_product_weights():
    ref = rational_ref(True)
    G = patch_handle(ref)
    check_parity(G, ref)
    assert G.path_ == 1 and not G.HoldsGradientTables()


def test_parity_with_general_weights():
    ref = rational_ref(False)
    check_parity(flat_handle(ref), ref)


@pytest.mark.parametrize("n_el,p", [((5, 4, 3), 2), ((4, 3, 3), 3), ((3, 2, 2), 1)], ids=["p2", "p3", "p1"])
def test_parity_with_permuted_node_ids(n_el, p):
    """node_ids as in test_domain_gpu.py::test_permuted_node_numbering: the CSR and r in the caller's numbering"""
    import scipy.sparse as sp
    from mimi_amd import _capi
    from mimi_amd.integrators import CSRPattern
    ref = block_ref(n_el, p)
    P, D = ref.P, ref.D
    perm = np.random.default_rng(11).permutation(P.n_nodes).astype(np.int64)
    dofperm = (perm[:, None] * 3 + np.arange(3)[None, :]).ravel()
    rows_o = np.repeat(np.arange(P.n_vdofs), np.diff(D.rowptr))
    S = sp.coo_matrix((np.arange(1, D.nnz + 1, dtype=np.float64), (dofperm[rows_o], dofperm[D.col])),
                      shape=(P.n_vdofs, P.n_vdofs)).tocsr()
    S.sort_indices()
    dst = np.empty(D.nnz, dtype=np.int64)
    dst[(S.data - 1).astype(np.int64)] = np.arange(D.nnz)
    G = patch_handle(ref, pattern=CSRPattern(S.indptr.astype(np.int64), S.indices.astype(np.int32), D.nnz), node_ids=perm)
    if p > 1:
        assert _capi.lib().mimi_hip_domain_info(G._h, 6) == 2
    M, C, f = forms(G, ref)
    assert close(M[dst], ref.M)
    assert close(C[dst], ref.C)
    assert close(f[dofperm], ref.f)
    assert not G.HoldsGradientTables()


# ---- 2. accumulation, 3. reproducibility -----------------------------------------------------------------------------------
def handles_of_every_route():
    yield "p2", block_ref((5, 4, 3), 2), patch_handle(block_ref((5, 4, 3), 2))
    yield "2d", block_ref((7, 5), 2), patch_handle(block_ref((7, 5), 2))
    yield "general", case_ref("rep3d_p2"), patch_handle(case_ref("rep3d_p2"))
    yield "flat", block_ref((3, 2, 2), 1), flat_handle(block_ref((3, 2, 2), 1), product_patch(block_ref((3, 2, 2), 1).P))


def test_outputs_are_accumulated_and_off_diagonal_components_untouched():
    rng = np.random.default_rng(3)
    for name, ref, G in handles_of_every_route():
        D, dim = ref.D, ref.P.dim
        M0, C0, f0 = rng.standard_normal(D.nnz), rng.standard_normal(D.nnz), rng.standard_normal(ref.P.n_vdofs)
        M, C, f = forms(G, ref, M0.copy(), C0.copy(), f0.copy())
        rows = np.repeat(np.arange(ref.P.n_vdofs), np.diff(D.rowptr))
        off = (rows % dim) != (np.asarray(D.col) % dim)
        # (before + factor x reference, to the tolerance plus the rounding of that one addition)
        for got, before, want in ((M, M0, ref.M), (C, C0, ref.C)):
            assert np.abs(got - (before + want)).max() <= TOL * np.abs(want).max() + 4 * np.finfo(float).eps * np.abs(before).max(), name
            assert np.array_equal(got[off], before[off]), name
        assert np.abs(f - (f0 + ref.f)).max() <= TOL * np.abs(ref.f).max() + 4 * np.finfo(float).eps * np.abs(f0).max(), name


def test_two_calls_and_both_residences_give_equal_bytes():
    import torch
    for name, ref, G in handles_of_every_route():
        a, b = forms(G, ref), forms(G, ref)
        dev = [torch.zeros(ref.D.nnz, dtype=torch.float64, device="cuda"), torch.zeros(ref.D.nnz, dtype=torch.float64, device="cuda"),
               torch.zeros(ref.P.n_vdofs, dtype=torch.float64, device="cuda")]
        forms(G, ref, *dev)
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, dev):
            assert np.array_equal(x, y), name
            assert np.array_equal(x, z.cpu().numpy()), name


# ---- 4. element boxes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n_el,p", [((5, 4, 3), 2), ((4, 3, 3), 3)], ids=["p2", "p3"])
def test_element_boxes_add_up_to_the_whole(n_el, p, axis):
    ref = block_ref(n_el, p)
    M, C, f = np.zeros(ref.D.nnz), np.zeros(ref.D.nnz), np.zeros(ref.P.n_vdofs)
    for b, e in ((0, 2), (2, n_el[axis])):
        begin, end = [0, 0, 0], list(n_el)
        begin[axis], end[axis] = b, e
        forms(patch_handle(ref, element_box=(begin, end)), ref, M, C, f)
    assert close(M, ref.M)
    assert close(C, ref.C)
    assert close(f, ref.f)


@pytest.mark.parametrize("n_el,p", [((5, 4, 3), 2), ((4, 3, 3), 3)], ids=["p2", "p3"])
def test_element_boxes_on_row_slices(n_el, p):
    """each box on the mimi_hip_bspline_sparsity_rows slice of the nodes it touches (device arrays, as the multi-GPU path
    holds them): the rows of the slices, put back where they belong, add up to the whole"""
    import torch
    from mimi_amd.integrators import CSRPattern
    ref = block_ref(n_el, p)
    patch = product_patch(ref.P)
    full = np.diff(ref.D.rowptr)
    M, C = np.zeros(ref.D.nnz), np.zeros(ref.D.nnz)
    for b, e in ((0, 2), (2, n_el[2])):
        lo, hi = [0, 0, 0], [n + p for n in n_el]
        lo[2], hi[2] = b, e + p
        part = CSRPattern.of_bspline_patch(patch, on_device=True, node_box=(lo, hi))
        rp_s = part.rowptr.cpu().numpy()
        held = np.nonzero(np.diff(rp_s))[0]
        assert np.array_equal(np.diff(rp_s)[held], full[held])
        where = np.concatenate([np.arange(ref.D.rowptr[r], ref.D.rowptr[r + 1]) for r in held])
        G = patch_handle(ref, pattern=part, element_box=([0, 0, b], [n_el[0], n_el[1], e]))
        m, c = torch.zeros(part.nnz, dtype=torch.float64, device="cuda"), torch.zeros(part.nnz, dtype=torch.float64, device="cuda")
        G.AddMass(RHO, m)
        G.AddDiffusion(NU, c)
        M[where] += m.cpu().numpy()
        C[where] += c.cpu().numpy()
    assert close(M, ref.M)
    assert close(C, ref.C)


# ---- 5. closed forms, no reference in the loop -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["greville", "rational"])
def test_closed_forms(which):
    import scipy.sparse as sp
    ref = case_ref("nonuni3d_p2") if which == "greville" else rational_ref(True)
    D, n, dim = ref.D, ref.P.n_vdofs, ref.P.dim
    M, C, f = forms(patch_handle(ref), ref)
    Mm = sp.csr_matrix((M, D.col, D.rowptr), shape=(n, n))
    Cm = sp.csr_matrix((C, D.col, D.rowptr), shape=(n, n))
    ones = np.ones(n)
    per_component = (Mm @ ones).reshape(-1, dim).sum(axis=0)
    assert np.allclose(per_component, RHO * ref.volume, rtol=1e-12, atol=0.0)
    assert np.abs(Cm @ ones).max() <= 1e-12 * np.abs(C).max()
    assert abs(Mm - Mm.T).max() <= TOL * np.abs(M).max()
    assert abs(Cm - Cm.T).max() <= TOL * np.abs(C).max()
    assert np.allclose(f.reshape(-1, dim).sum(axis=0), ref.b * ref.volume, rtol=1e-12, atol=0.0)


# ---- 6. error paths --------------------------------------------------------------------------------------------------------
def test_error_paths():
    from mimi_amd import _capi
    L = _capi.lib()
    ref = block_ref((3, 2, 2), 1)
    G = flat_handle(ref, product_patch(ref.P), shape_values=False)
    M, f = np.zeros(ref.D.nnz), np.zeros(ref.P.n_vdofs)
    with pytest.raises(RuntimeError, match="mimi_hip_domain_set_shape_values"):
        G.AddMass(RHO, M)
    with pytest.raises(RuntimeError, match="mimi_hip_domain_set_shape_values"):
        G.AddBodyForce(ref.b, f)
    assert not M.any() and not f.any()
    C = G.AddDiffusion(NU, np.zeros(ref.D.nnz))        # needs no shape values
    assert close(C, ref.C)
    b = np.ascontiguousarray(ref.b)
    assert L.mimi_hip_domain_add_mass(None, 1.0, _capi.fptr(M)) != 0 and b"null" in L.mimi_hip_last_error()
    assert L.mimi_hip_domain_add_diffusion(None, 1.0, _capi.fptr(M)) != 0
    assert L.mimi_hip_domain_add_body_force(None, _capi.fptr(b), _capi.fptr(f)) != 0
    assert L.mimi_hip_domain_add_mass(G._h, 1.0, None) != 0 and b"null" in L.mimi_hip_last_error()
    assert L.mimi_hip_domain_add_diffusion(G._h, 1.0, None) != 0
    assert L.mimi_hip_domain_add_body_force(G._h, None, _capi.fptr(f)) != 0
    assert L.mimi_hip_domain_add_body_force(G._h, _capi.fptr(b), None) != 0
    G.Synchronize()


# ---- 7. / 8. facade --------------------------------------------------------------------------------------------------------
MESH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "cube-nurbs.mesh")


def facade(host, periodic=False, order=None, rational=False, body=-20.0, body1=None, iterative=True):
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(MESH)
    nl.elevate_degrees(1)
    nl.subdivide(1)
    if rational:
        rng = np.random.default_rng(9)
        nl._nurbs.weights = 1.0 + 0.3 * rng.random(nl._nurbs.weights.shape)
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1.3
    mat.viscosity = 0.2
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    face = {f: a - 1 for a, f in nl._faces.items()}
    bc = mimi.BoundaryConditions()
    clamp, loaded = face[(0, 0)], face[(0, 1)]
    bc.initial.dirichlet(clamp, 0).dirichlet(clamp, 1).dirichlet(clamp, 2)
    bc.initial.body_force(2, body)
    if body1 is not None:
        bc.initial.body_force(1, body1)
    if not rational:                                       # (faces of rational patches are refused by the traction)
        bc.initial.traction(loaded, 1, 3.5)
    if periodic:
        bc.initial.periodic(face[(1, 0)] + 1, face[(1, 1)] + 1)
    nl.boundary_condition = bc
    rc = mimi.RuntimeCommunication()
    rc.set_int("host_setup", 1 if host else 0)
    rc.set_int("use_iterative_solver", 1 if iterative else 0)
    if order is not None:
        rc.set_int("nonlinear_solid_quadrature_order", order)
    nl.runtime_communication = rc
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-12, 1e-9, 20, False)
    nl.time_step_size = 0.05
    return nl


@pytest.mark.parametrize("variant", ["plain", "periodic", "order5", "rational"])
def test_facade_set_up_on_the_device(variant):
    kw = dict(periodic=variant == "periodic", order=5 if variant == "order5" else None, rational=variant == "rational")
    dev, host = facade(False, **kw), facade(True, **kw)
    assert not dev.host_setup_ and host.host_setup_
    assert dev.host_nnz_arrays_ == 0 and dev._mass_host is None and dev._visc_host is None     # nothing of nnz doubles on the host
    assert host.host_nnz_arrays_ == 2
    assert close(dev.d_mass_.cpu().numpy(), host.d_mass_.cpu().numpy())
    assert close(dev.d_visc_.cpu().numpy(), host.d_visc_.cpu().numpy())
    assert close(dev.rhs_, host.rhs_)
    # the traction part: the components the body force does not load hold the traction alone
    t_dev, t_host = dev.rhs_.reshape(-1, 3)[:, :2], host.rhs_.reshape(-1, 3)[:, :2]
    assert np.array_equal(t_dev, t_host) and (variant == "rational" or np.abs(t_dev).max() > 0)
    dev.step_time2()                                       # iterative route: still no download
    assert dev.host_nnz_arrays_ == 0 and dev._mass_host is None
    assert np.array_equal(dev.mass_, dev.d_mass_.cpu().numpy()) and dev.host_nnz_arrays_ == 1
    assert dev.mass_ is dev.mass_


def test_host_setup_by_environment(monkeypatch):
    monkeypatch.setenv("MIMI_HIP_HOST_SETUP", "1")
    assert facade(False).host_setup_


def test_set_body_force():
    a, b = facade(False, body=-20.0), facade(False, body=-20.0)
    view = a.linear_form_view2("rhs")
    a.step_time2()
    b.step_time2()
    assert np.array_equal(a.x, b.x)
    a.set_body_force(1, 35.0)
    assert a.linear_form_view2("rhs") is view and a.rhs_ is view
    assert np.array_equal(a.rhs_, facade(False, body=-20.0, body1=35.0).rhs_)     # a fresh solid set up with that force
    a.step_time2()
    b.step_time2()
    assert np.abs(a.x - b.x).max() > 1e-8 * np.abs(b.x).max()


def test_set_body_force_makes_a_right_hand_side():
    import mimi_amd as mimi
    nl = mimi.NonlinearSolid()
    nl.read_mesh(MESH)
    nl.elevate_degrees(1)
    mat = mimi.CompressibleOgdenNeoHookean()
    mat.density = 1
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    bc = mimi.BoundaryConditions()
    bc.initial.dirichlet(0, 0).dirichlet(0, 1).dirichlet(0, 2)
    nl.boundary_condition = bc
    nl.setup(1)
    assert not nl.has_rhs_ and not nl.rhs_.any()
    nl.set_body_force(2, -9.81)
    assert nl.has_rhs_ and nl.rhs_.any() and nl.linear_form_view2("rhs") is nl.rhs_
    assert not nl.rhs_[nl.dirichlet_].any() and not nl.rhs_.reshape(-1, 3)[:, :2].any()
