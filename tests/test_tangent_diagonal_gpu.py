"""The node-block diagonal of the matrix-free tangent (csrc/kernels_diagonal.hpp) through the C ABI:
NonlinearSolid.TangentDiagonal.

(1) blocks and diagonal of the stiffness term on one case per way the kernel can go wrong (CASES below) x neohook, stvk, j2
    against the long-double tangent of tests/_domain_reference.py -- dP/dF at every point from the unit directions e_j (x) e_L,
    the node blocks sum_q w det d_J N_A (dP_iJ/dF_jL) d_L N_A cut out in numpy -- within dc.tangent_bar, relative to the
    largest entry (the normalisation of test_matrix_free_gpu.py::test_stiffness_action_against_the_reference);
(2) J2Simo and J2Log against the node blocks of the handle's own assembled tangent within dc.TANGENT_BAR, and on the same
    cases against the long-double node blocks of (1) within dc.tangent_bar;
(3) the mass and viscosity terms against the node blocks of the device-assembled AddMass / AddDiffusion within dc.FORMS_BAR;
(4) against the action itself, no matrix anywhere: column j of block A is rows (A, .) of ApplyTangent(e_(A, j));
(5) symmetry of the hyperelastic blocks within dc.SYMMETRY_BAR;
(6) the contract: += into a prefilled array, equal bytes from two calls and from a device tensor, block=False equal TO THE
    BIT to the diagonal of block=True (both modes run one instruction stream per component), element boxes add up, the
    snapshot survives a commit, another dt and an overwritten u, the two refusals."""
import numpy as np
import pytest
import scipy.sparse as sp

import _domain_cases as dc
from _cases import product_material
from _domain_cases import DT, f64
from test_matrix_free_gpu import action, handle, linearized, relmax

pytestmark = pytest.mark.gpu

CASES = ["one2d_p1", "one3d_p2",      # single element, no neighbour sums
         "rep2d_p3",                  # tensor_small, repeated knots
         "col8_p2",                   # four elements per workgroup, uneven tail (32 elements -> 8 workgroups; the boxes: 12 and 20)
         "col5_p3",                   # 125 points, two waves per element
         "mix3d_231",                 # general route, mixed degrees
         "nurbs_tp_p2",               # rational tensor-product weights
         "nurbs_flat_p2",             # flat tables
         "rep3d_p2_o3"]               # non-default rule
MATERIALS = ["neohook", "stvk", "j2"]


reference_blocks = dc.reference_blocks          # D[A, i, j] of the stiffness term in long double (tests/_domain_cases.py)


def diagonal(G, n_nodes, dim, block, **coefficients):
    """TangentDiagonal into zeros: [A, i, j] or [A, i]"""
    out = np.zeros(n_nodes * dim * (dim if block else 1))
    G.TangentDiagonal(out, block=block, **coefficients)
    return out.reshape((n_nodes, dim, dim) if block else (n_nodes, dim))


def csr_blocks(vals, case):
    """the node blocks [A, i, j] of CSR values on the case's pattern (an entry the pattern lacks is zero)"""
    a = dc.arrays(case)
    rowptr, col, _ = dc.pattern(case)
    K = sp.csr_matrix((vals, col, rowptr), shape=(a.n_vdofs, a.n_vdofs)).toarray()
    return np.stack([K[A * a.dim:(A + 1) * a.dim, A * a.dim:(A + 1) * a.dim] for A in range(a.n_nodes)])


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", MATERIALS)
@pytest.mark.parametrize("case", CASES)
def test_blocks_and_diagonal_against_the_reference(case, matname):
    a = dc.arrays(case)
    G, r = linearized(case, matname)
    want = reference_blocks(case, matname)
    blocks = diagonal(G, a.n_nodes, a.dim, True)
    diag = diagonal(G, a.n_nodes, a.dim, False)
    dev_b = relmax(blocks, want)
    dev_d = relmax(diag, np.einsum("Aii->Ai", want))
    print(f"\n{case} {matname} [{a.family}]: blocks deviate {dev_b:.2e}, diagonal {dev_d:.2e} (bar {dc.tangent_bar(matname):.2e})")
    assert dev_b <= dc.tangent_bar(matname) and dev_d <= dc.tangent_bar(matname)
    assert np.einsum("Aii->Ai", blocks).tobytes() == diag.tobytes()


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["j2simo", "j2log"])
@pytest.mark.parametrize("case", list(dc.EXTRA.values()))
def test_finite_strain_laws_against_the_assembled_tangent(case, model):
    a = dc.arrays(case)
    u0, u = dc.inputs(case, "j2")
    G = handle(case, product_material(model))
    G.DomainPostTimeAdvance(u0)
    vals = np.zeros(len(dc.pattern(case)[1]))
    G.AddDomainResidualAndGrad(np.array(u), 1.0, np.zeros(a.n_vdofs), vals)
    G.Linearize(np.array(u))
    want = csr_blocks(vals, case)
    dev = relmax(diagonal(G, a.n_nodes, a.dim, True), want)
    print(f"\n{case} {model} [{a.family}]: blocks deviate {dev:.2e} from the assembled tangent's (bar {dc.TANGENT_BAR:.2e})")
    assert dev <= dc.TANGENT_BAR
    # independently: the same model at its own inputs (dc.SEEDS) against the long-double node blocks
    G, r = linearized(case, model)
    want = reference_blocks(case, model)
    dev_b = relmax(diagonal(G, a.n_nodes, a.dim, True), want)
    dev_d = relmax(diagonal(G, a.n_nodes, a.dim, False), np.einsum("Aii->Ai", want))
    print(f"{case} {model} [{a.family}]: blocks deviate {dev_b:.2e}, diagonal {dev_d:.2e} from the reference's (bar {dc.tangent_bar(model):.2e})")
    assert dev_b <= dc.tangent_bar(model) and dev_d <= dc.tangent_bar(model)


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.FORMS_CASES)
def test_mass_and_viscosity_terms(case):
    a = dc.arrays(case)
    G = handle(case, "neohook")
    nnz = len(dc.pattern(case)[1])
    mass = csr_blocks(G.AddMass(dc.RHO, np.zeros(nnz)), case)
    visc = csr_blocks(G.AddDiffusion(dc.NU, np.zeros(nnz)), case)
    fig = {}
    for block in (True, False):
        cut = (lambda B: B) if block else (lambda B: np.einsum("Aii->Ai", B))
        m = diagonal(G, a.n_nodes, a.dim, block, stiffness=0.0, density=dc.RHO)          # (no Linearize: stiffness 0 needs none)
        c = diagonal(G, a.n_nodes, a.dim, block, stiffness=0.0, viscosity=dc.NU)
        both = diagonal(G, a.n_nodes, a.dim, block, stiffness=0.0, density=dc.RHO, viscosity=dc.NU)
        fig[block] = (relmax(m, cut(mass)), relmax(c, cut(visc)), relmax(both, cut(mass + visc)))
    print(f"\n{case}: " + ", ".join(f"block={k}: mass {m:.2e} viscosity {c:.2e} sum {b:.2e}" for k, (m, c, b) in fig.items()))
    assert max(max(v) for v in fig.values()) <= dc.FORMS_BAR
    # the three terms in one call, each within its own bar
    r = dc.reference(case, "neohook")
    G.Linearize(np.array(r.u))
    whole = diagonal(G, a.n_nodes, a.dim, True, stiffness=1.0, density=dc.RHO, viscosity=dc.NU)
    K = f64(reference_blocks(case, "neohook"))
    bar = dc.FORMS_BAR * (np.abs(mass).max() + np.abs(visc).max()) + dc.tangent_bar("neohook") * np.abs(K).max()
    assert np.abs(whole - (mass + visc + K)).max() <= bar


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", MATERIALS)
@pytest.mark.parametrize("case", ["one3d_p2", "rep2d_p2"])
def test_against_the_action(case, matname):
    a = dc.arrays(case)
    G, r = linearized(case, matname)
    coefficients = dict(stiffness=0.8, density=dc.RHO, viscosity=dc.NU)
    blocks = diagonal(G, a.n_nodes, a.dim, True, **coefficients)
    from_action = np.zeros_like(blocks)
    for A in range(a.n_nodes):
        for j in range(a.dim):
            e = np.zeros(a.n_vdofs)
            e[A * a.dim + j] = 1.0
            from_action[A, :, j] = action(G, e, **coefficients)[A * a.dim:(A + 1) * a.dim]
    dev = relmax(blocks, from_action)
    print(f"\n{case} {matname}: blocks deviate {dev:.2e} from the action's columns (bar {dc.tangent_bar(matname):.2e})")
    assert dev <= dc.tangent_bar(matname)


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", ["neohook", "stvk"])
@pytest.mark.parametrize("case", ["rep2d_p3", "col8_p2", "col5_p3", "mix3d_231"])
def test_hyperelastic_blocks_are_symmetric(case, matname):
    a = dc.arrays(case)
    G, r = linearized(case, matname)
    B = diagonal(G, a.n_nodes, a.dim, True)
    asym = np.abs(B - np.swapaxes(B, 1, 2)).max() / np.abs(B).max()
    print(f"\n{case} {matname}: asymmetry {asym:.2e}")
    assert asym <= dc.SYMMETRY_BAR


# ---- (6) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", [("col8_p2", "neohook"), ("col8_p2", "j2"), ("rep2d_p3", "j2"), ("mix3d_231", "stvk"),
                                          ("nurbs_flat_p2", "neohook")])
def test_accumulation_equal_bytes_and_the_snapshot(case, matname):
    import torch
    a = dc.arrays(case)
    G, r = linearized(case, matname)
    coefficients = dict(stiffness=1.0, density=dc.RHO, viscosity=dc.NU)
    for block in (True, False):
        first = diagonal(G, a.n_nodes, a.dim, block, **coefficients)
        assert np.isfinite(first).all() and np.abs(first).max() > 0
        assert diagonal(G, a.n_nodes, a.dim, block, **coefficients).tobytes() == first.tobytes()
        # += : the increment on a prefilled array is the value on zeros, up to the rounding of the one addition
        d0 = np.random.default_rng(3).standard_normal(first.size)
        d = d0.copy()
        G.TangentDiagonal(d, block=block, **coefficients)
        assert np.abs((d - d0) - first.ravel()).max() <= 4 * np.finfo(float).eps * (np.abs(d0).max() + np.abs(first).max())
        # a device tensor: the bytes of the host call
        d_dev = torch.zeros(first.size, dtype=torch.float64, device=torch.device("cuda", 0))
        G.TangentDiagonal(d_dev, block=block, **coefficients)
        G.Synchronize()
        assert d_dev.cpu().numpy().tobytes() == first.tobytes()
        # the snapshot: the caller's u overwritten, another dt, a commit at another displacement
        G2 = handle(case, matname)
        if r.mat.stateful:
            G2.DomainPostTimeAdvance(r.u0)
        u = np.array(r.u)
        G2.Linearize(u)
        u[:] = np.nan
        G2.dt_ = 0.25 * DT
        G2._push_dt()
        G2.DomainPostTimeAdvance(np.array(r.u))
        assert diagonal(G2, a.n_nodes, a.dim, block, **coefficients).tobytes() == first.tobytes()


@pytest.mark.parametrize("matname", ["neohook", "j2"])
def test_element_boxes_add_up(matname):
    case = dc.BOX_CASE
    a = dc.arrays(case)
    boxes = [linearized(case, matname, element_box=box)[0] for box in dc.BOXES]
    want = reference_blocks(case, matname)
    total = sum(diagonal(G, a.n_nodes, a.dim, True) for G in boxes)
    assert relmax(total, want) <= dc.tangent_bar(matname)
    total = sum(diagonal(G, a.n_nodes, a.dim, False) for G in boxes)
    assert relmax(total, np.einsum("Aii->Ai", want)) <= dc.tangent_bar(matname)
    # the mass term of the boxes is the whole's
    whole = diagonal(handle(case, matname), a.n_nodes, a.dim, False, stiffness=0.0, density=dc.RHO)
    parts = sum(diagonal(G, a.n_nodes, a.dim, False, stiffness=0.0, density=dc.RHO) for G in boxes)
    assert relmax(parts, whole) <= dc.FORMS_BAR


def test_stiffness_before_linearize_is_refused():
    a = dc.arrays("rep2d_p2")
    G = handle("rep2d_p2", "neohook")
    with pytest.raises(RuntimeError, match="before any mimi_hip_domain_linearize"):
        G.TangentDiagonal(np.zeros(a.n_vdofs))
    with pytest.raises(RuntimeError, match="before any mimi_hip_domain_linearize"):
        G.TangentDiagonal(np.zeros(a.n_vdofs * a.dim), block=True)
    G.TangentDiagonal(np.zeros(a.n_vdofs), stiffness=0.0, density=1.0)


def test_mass_term_on_flat_tables_needs_shape_values():
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    case = "flat2d_p4"
    a = dc.arrays(case)
    rowptr, col, _ = dc.pattern(case)
    tables = dict(dc.flat_tables(case))
    tables.pop("N")
    G = NonlinearSolid("domain", dc.product_material("neohook"), CSRPattern(np.array(rowptr), np.array(col, dtype=np.int32), len(col)),
                       tables=tables).Prepare()
    with pytest.raises(RuntimeError, match="set_shape_values"):
        G.TangentDiagonal(np.zeros(a.n_vdofs), stiffness=0.0, density=1.0)
    G.TangentDiagonal(np.zeros(a.n_vdofs), stiffness=0.0, viscosity=1.0)
