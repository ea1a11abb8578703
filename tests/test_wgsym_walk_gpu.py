"""The multi-unit walk of the symmetric-half degree-2 kernel (csrc/kernels_tensor_wgsym.hpp: a workgroup walks cols_per_wg
units -- element columns or column segments -- back to back, every unit from empty carries: the register carries and the riders'
second value in the per-lane LDS slots off_cp), at sizes where a reference sees every entry, and at the smallest shapes that
reach the shipped thresholds.  Every test asserts the launch geometry it was written to reach (mimi_hip_domain_info 11 / 12,
NonlinearSolid.LastWalkGeometry); tests/test_wgsym_geometry_cpu.py holds the arithmetic behind the numbers used here.

1. Walks at <= 48 elements, reached through MIMI_HIP_WGSYM_MIN_WGS (read at create): the cases of _domain_cases.WALKS against
   the long-double reference of tests/_domain_reference.py at the bars of its family (residual 1e-12 per row, K v 1e-11), whole,
   with permuted node ids, and through two element boxes cut in x.
2. Bit equality: residual and tangent of every such launch equal those of the same case with the switch unset (one unit per
   workgroup).  The switch changes only which workgroup walks a unit; a unit starts from zero carries, every element's pieces
   land in its own scratch block, phase 2 is untouched.
3. More segment shapes (switch unset) on non-uniform jittered patches against the oracle at 1e-12 / 1e-11: nseg 4, seg_len 5
   and 6, and a cut box that begins inside the column (phase 2 finds segment ends by (ez - box_begin[2]) % seg_len).
4. The shipped thresholds, switch unset, non-uniform jittered patches: 65 x 65 x 1 (2 per workgroup, last one 1),
   79 x 79 x 1 (3, 1), 91 x 93 x 1 (4, 3), 64 x 64 x 5 (2, exact, two-step carry): complete CSR rows and residual entries of
   sampled nodes -- corners, edges, faces, random ones, and nodes whose elements lie in the units of two workgroups (the first
   such boundary, one in the middle, one where the column index wraps from the end of an x-row to the next y, and the columns of
   the last workgroup) -- against the oracle's element blocks at 1e-12 / 1e-11, and EVERY entry bit for bit against a second
   handle that walks one unit per workgroup.

Measured on the MI355X (-s prints every figure): see DESIGN.md, "The multi-unit walk, tested"."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _domain_cases as dc
import _domain_reference as dr
import _patches
from _cases import oracle_material, product_material, synthetic_u
from _domain_cases import DT, GRAD_FACTOR, f64
from _sampling import SampledRows, sample_nodes

pytestmark = pytest.mark.gpu

SWITCH = "MIMI_HIP_WGSYM_MIN_WGS"
FAMILY = "tensor_p2_two_phase"
MAT = dc.WALK_MATERIAL


def relmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max() / max(np.abs(f64(b)).max(), 1e-300))


def same_bits(label, got, want):
    """np.array_equal, with the figures of a difference printed first"""
    for name, a, b in zip(("residual", "tangent"), got, want):
        differ = a != b
        if differ.any():
            print(f"{label}: {int(differ.sum())} of {a.size} {name} entries differ from the one-unit walk, by at most "
                  f"{np.abs(a - b).max() / np.abs(b).max():.2e} of the largest")
    return all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- 1., 2. the walks of _domain_cases.WALKS ---------------------------------------------------------------------------------
def handle(case, element_box=None, node_ids=None, pattern=None):
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    if pattern is None:
        rowptr, col, _ = dc.pattern(case)
        pattern = CSRPattern(np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), len(col))
    G = NonlinearSolid("domain", dc.product_material(MAT), pattern, patch=dc.product_patch(case), element_box=element_box,
                       node_ids=node_ids).Prepare()
    G.dt_ = DT
    assert G.path_ == 1
    return G


def assemble(G, u, geometry):
    """(r, A) of one tangent assembly from zero on a fresh handle; the launch had `geometry` = (seg_len, cols_per_wg)"""
    assert G.LastWalkGeometry() == (0, 0)
    r, A = np.zeros(u.size), np.zeros(G.nnz_)
    G.AddDomainResidualAndGrad(u, GRAD_FACTOR, r, A)
    assert G.LastKernelFamily() == FAMILY
    assert G.LastWalkGeometry() == geometry
    return r, A


def check(case, r, A, label, mask=None):
    """r, A (lexicographic numbering) against the reference restricted to the points of `mask`"""
    ref = dc.reference(case, MAT)
    geo = ref.geo
    want_r = f64(ref.asm.r if mask is None else dr.nodal(geo, ref.asm.pt.P, mask))
    want_Kv = [f64(k) if mask is None else f64(dr.nodal(geo, dP, mask)) for k, dP in zip(ref.asm.Kv, ref.asm.pt.dP)]
    rowptr, col, _ = dc.pattern(case)
    K = sp.csr_matrix((A, col, rowptr), shape=(r.size, r.size))
    er = float((np.abs(r - want_r) / dc.residual_bar(ref, mask)).max())
    eA = max(relmax(K @ v, GRAD_FACTOR * Kv) for v, Kv in zip(ref.vectors, want_Kv))
    print(f"{label}: residual {er:.2e} of the row bar (relative {relmax(r, want_r):.2e}), tangent {eA:.2e}")
    assert np.abs(want_r).max() > 0 and all(np.abs(k).max() > 0 for k in want_Kv)
    assert er <= 1.0
    assert eA <= dc.tangent_bar(MAT)


@functools.lru_cache(maxsize=None)
def one_unit_walk(case, seg_len):
    """(r, A) of the case with the switch unset -- one unit per workgroup, asserted -- checked against the reference; computed
    once, shared, never written to"""
    assert SWITCH not in os.environ
    r, A = assemble(handle(case), dc.reference(case, MAT).u, (seg_len, 1))
    check(case, r, A, f"{case} one unit per workgroup")
    for x in (r, A):
        x.setflags(write=False)
    return r, A


WALK_PARAMS = [pytest.param(case, seg_len, value, cols, id=f"{case}-{value}") for case, _, seg_len, walks in dc.WALKS
               for value, cols, _ in walks]


@pytest.mark.parametrize("case,seg_len,value,cols", WALK_PARAMS)
def test_walk_against_the_reference_and_the_one_unit_walk(monkeypatch, case, seg_len, value, cols):
    base = one_unit_walk(case, seg_len)
    monkeypatch.setenv(SWITCH, str(value))
    r, A = assemble(handle(case), dc.reference(case, MAT).u, (seg_len, cols))
    check(case, r, A, f"{case} {SWITCH}={value}: {cols} units per workgroup")
    assert same_bits(f"{case} {value}", (r, A), base)


@functools.lru_cache(maxsize=None)
def permuted(case):
    """a random renumbering of the nodes: (perm, lexicographic dof -> caller's dof, the caller's CSR arrays, where entry k of the
    lexicographic pattern lies in the caller's)"""
    rowptr, col, _ = dc.pattern(case)
    a = dc.arrays(case)
    perm = np.random.default_rng(11).permutation(a.n_nodes).astype(np.int64)
    dofperm = (perm[:, None] * 3 + np.arange(3)[None, :]).ravel()
    rows = np.repeat(np.arange(a.n_vdofs), np.diff(rowptr))
    S = sp.coo_matrix((np.arange(1, len(col) + 1, dtype=np.float64), (dofperm[rows], dofperm[col])), shape=(a.n_vdofs, a.n_vdofs)).tocsr()
    S.sort_indices()
    dst = np.empty(len(col), dtype=np.int64)
    dst[(S.data - 1).astype(np.int64)] = np.arange(len(col))
    return perm, dofperm, (S.indptr.astype(np.int64), S.indices.astype(np.int32)), dst


def test_walk_with_permuted_node_ids(monkeypatch):
    """walk335_p2, four units per workgroup and a last workgroup of one, the rows gathered at the caller's node ids"""
    from mimi_amd import _capi
    from mimi_amd.integrators import CSRPattern
    case, seg_len = "walk335_p2", 5
    base = one_unit_walk(case, seg_len)
    perm, dofperm, (rowptr, col), dst = permuted(case)
    u = dc.reference(case, MAT).u
    u_p = np.empty_like(u)
    u_p[dofperm] = u
    out = {}
    for value, cols in ((None, 1), (2, 4)):
        if value is None:
            assert SWITCH not in os.environ
        else:
            monkeypatch.setenv(SWITCH, str(value))
        G = handle(case, node_ids=perm, pattern=CSRPattern(rowptr, col, len(col)))
        assert _capi.lib().mimi_hip_domain_info(G._h, 6) == 2
        r, A = assemble(G, u_p, (seg_len, cols))
        check(case, r[dofperm], A[dst], f"{case} permuted, {cols} units per workgroup")
        out[cols] = (r, A)
    assert same_bits(f"{case} permuted", out[4], out[1])
    # and the permutation only moves the entries
    assert same_bits(f"{case} permuted against lexicographic", (out[1][0][dofperm], out[1][1][dst]), base)


def test_walk_through_element_boxes_cut_in_x(monkeypatch):
    """walk335_p2 as the boxes x in [0, 1) and [1, 3): the second one's box_begin[0] = 1 enters the spans of the walk (its six
    units: one workgroup of four, one of two); each box against the reference restricted to its parameter range, the sum
    against the whole, and every box bit for bit against its own one-unit walk"""
    case, seg_len = dc.WALK_BOX_CASE, 5
    ref = dc.reference(case, MAT)
    out = {}
    for value in (None, 1):
        if value is None:
            assert SWITCH not in os.environ
        else:
            monkeypatch.setenv(SWITCH, str(value))
        for box, cols in dc.WALK_BOXES:
            cols = cols if value else 1
            r, A = assemble(handle(case, element_box=box), ref.u, (seg_len, cols))
            check(case, r, A, f"{case} box {box}, {cols} units per workgroup", mask=dr.in_box(ref.geo.sp, *box))
            out[(value, tuple(box[0]))] = (r, A)
    for box, _ in dc.WALK_BOXES:
        assert same_bits(f"{case} box {box}", out[(1, tuple(box[0]))], out[(None, tuple(box[0]))])
    r_sum, A_sum = (sum(out[(1, tuple(box[0]))][k] for box, _ in dc.WALK_BOXES) for k in (0, 1))
    check(case, r_sum, A_sum, f"{case} boxes summed")


def test_the_switch_is_read_at_create_and_nowhere_else(monkeypatch):
    """a handle keeps the value of its create: changing or removing the variable afterwards changes nothing on it"""
    case, seg_len = "walk761_p2", 1
    u = dc.reference(case, MAT).u
    monkeypatch.setenv(SWITCH, "14")
    G = handle(case)
    monkeypatch.delenv(SWITCH)
    assemble(G, u, (seg_len, 3))
    G1 = handle(case)
    monkeypatch.setenv(SWITCH, "21")
    assemble(G1, u, (seg_len, 1))
    # the residual-only assembly is another kernel: it leaves the recorded geometry alone
    G1.AddDomainResidual(u, np.zeros(u.size))
    assert G1.LastKernelFamily() == FAMILY and G1.LastWalkGeometry() == (seg_len, 1)


# ---- 3. more segment shapes ----------------------------------------------------------------------------------------------------
def nonuniform_knots(n_el, seed):
    """open degree-2 knot vectors with spans drawn from [0.6, 1.4]"""
    rng = np.random.default_rng(seed)
    return [_patches.open_knots(2, np.cumsum(rng.uniform(0.6, 1.4, m))[:-1] if m > 1 else []) for m in n_el]


@functools.lru_cache(maxsize=None)
def jittered(n_el, seed=2):
    """(oracle patch, product patch, u) of a non-uniform Greville patch of n_el spans, the jitter and the displacement scaled by
    the smallest span"""
    knots = nonuniform_knots(n_el, seed)
    h = min(float(np.diff(np.unique(k)).min()) for k in knots)
    P, B = _patches.greville_patch((2, 2, 2), knots, jitter=0.04 * h, seed=seed)
    assert tuple(P.m) == tuple(n_el)
    u = synthetic_u(P, scale=0.05 * min(1.0, h))
    u.setflags(write=False)
    return P, B, u


@functools.lru_cache(maxsize=None)
def whole_oracle(n_el):
    """(oracle integrator, residual, tangent) of jittered(n_el): computed once, shared, never written to"""
    from oracle import ref_path as rp
    P, _, u = jittered(n_el)
    D = rp.DomainOracle(P, oracle_material("neohook"), n_threads=2)
    D.set_dt(DT)
    r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    D.add_domain_residual_and_grad(u, 1.0, r, A, rp.TANGENT_EXACT)
    for x in (r, A):
        x.setflags(write=False)
    return D, r, A


def oracle_handle(n_el, D, element_box=None):
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    pattern = CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=jittered(n_el)[1], element_box=element_box).Prepare()
    assert G.path_ == 1
    G.dt_ = DT
    return G


@pytest.mark.parametrize("n_el,seg_len", [((2, 2, 16), 4), ((3, 3, 10), 5), ((3, 3, 12), 6)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_segment_shapes_against_the_oracle(n_el, seg_len):
    """2 x 2 x 16: four segments of four; 3 x 3 x 10: two of five, the two-step carry meets a segment end; 3 x 3 x 12: two of six"""
    assert SWITCH not in os.environ
    P, _, u = jittered(n_el)
    D, r_o, A_o = whole_oracle(n_el)
    G = oracle_handle(n_el, D)
    r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
    assert G.LastKernelFamily() == FAMILY and G.LastWalkGeometry() == (seg_len, 1)
    er, eA = relmax(r, r_o), relmax(A, A_o)
    print(f"{n_el}: segments of {seg_len}: residual {er:.2e} tangent {eA:.2e}")
    assert er < 1e-12
    assert eA < 1e-11


def test_segments_of_a_box_that_begins_inside_the_column():
    """3 x 3 x 10 through the boxes z in [0, 1), [1, 9), [9, 10): the middle one is cut into two segments of four with
    box_begin[2] == 1, so a segment end is at ez = 4 and 8 of the patch, not 3 and 7"""
    assert SWITCH not in os.environ
    n_el = (3, 3, 10)
    P, _, u = jittered(n_el)
    D, r_o, A_o = whole_oracle(n_el)
    r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    for z0, z1, seg_len in ((0, 1, 1), (1, 9, 4), (9, 10, 1)):
        G = oracle_handle(n_el, D, element_box=([0, 0, z0], [3, 3, z1]))
        G.AddDomainResidualAndGrad(u, 1.0, r, A)
        assert G.LastKernelFamily() == FAMILY and G.LastWalkGeometry() == (seg_len, 1)
    er, eA = relmax(r, r_o), relmax(A, A_o)
    print(f"boxes of {n_el}: residual {er:.2e} tangent {eA:.2e}")
    assert er < 1e-12
    assert eA < 1e-11


# ---- 4. the shipped thresholds ---------------------------------------------------------------------------------------------------
def boundary_nodes(n_el, cols_per_wg):
    """multi-indices of nodes whose elements lie in the units of two workgroups, and those of the last workgroup's columns.
    Columns are numbered x fastest (ColumnWalk::begin_unit), workgroup w walks the columns [w c, (w + 1) c); the node
    (cx + 1, cy + 1, .) is in the elements of the columns cx - 1 .. cx + 1 of the rows cy - 1 .. cy + 1."""
    n0, n1, n2 = n_el
    units = n0 * n1
    grid = -(-units // cols_per_wg)
    k = (n2 + 2) // 2
    first = cols_per_wg
    middle = (grid // 2) * cols_per_wg
    if middle % n0 == 0:
        middle += cols_per_wg
    wrap = next(b for b in range(cols_per_wg, units, cols_per_wg) if b % n0 == 0)
    assert 0 < first % n0 and 0 < middle % n0 and first < middle < units and wrap // n0 >= 1
    picks = [(b % n0 + 1, b // n0 + 1, k) for b in (first, middle)]
    # the wrap: column wrap - 1 ends the row cy - 1, column wrap begins the row cy; both ends of the node row between them
    picks += [(n0 + 1, wrap // n0 + 1, k), (0, wrap // n0 + 1, k), (n0, wrap // n0, k)]
    picks += [(c % n0 + 1, c // n0 + 1, k) for c in range((grid - 1) * cols_per_wg, units)]
    return sorted(set(picks))


THRESHOLDS = [((65, 65, 1), 2, 1), ((79, 79, 1), 3, 1), ((91, 93, 1), 4, 3), ((64, 64, 5), 2, 2)]


@pytest.mark.parametrize("n_el,cols,tail", THRESHOLDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_shipped_thresholds(monkeypatch, n_el, cols, tail):
    import torch
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    assert SWITCH not in os.environ
    units = n_el[0] * n_el[1]
    assert units // 2048 == cols and units - (-(-units // cols) - 1) * cols == tail       # (the table of the module docstring)
    P, B, u_host = jittered(n_el)
    dev = torch.device("cuda", 0)
    pattern = CSRPattern.of_bspline_patch(B, on_device=True)
    u = torch.from_numpy(np.array(u_host)).to(dev)

    def run(geometry):
        G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
        G.dt_ = DT
        assert G.path_ == 1 and G.LastWalkGeometry() == (0, 0)
        r = torch.zeros(B.n_vdofs, dtype=torch.float64, device=dev)
        A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
        G.AddDomainResidualAndGrad(u, 1.0, r, A)
        G.Synchronize()
        assert G.LastKernelFamily() == FAMILY and G.LastWalkGeometry() == geometry
        return r, A

    r, A = run((n_el[2], cols))
    monkeypatch.setenv(SWITCH, str(2 ** 30))
    r1, A1 = run((n_el[2], 1))
    # every entry against the one-unit walk
    differ = int((A != A1).sum()), int((r != r1).sum())
    print(f"{n_el}: {differ[0]} of {A.numel()} tangent and {differ[1]} of {r.numel()} residual entries differ from the one-unit walk")
    assert torch.equal(r, r1) and torch.equal(A, A1)

    # sampled rows against the oracle's element blocks
    nodes = sorted(set(sample_nodes(P.n, 24, seed=5)) | set(boundary_nodes(n_el, cols)))
    S = SampledRows(P, oracle_material("neohook"), nodes, u_host, dt=DT)
    rowptr = pattern.rowptr if isinstance(pattern.rowptr, torch.Tensor) else torch.from_numpy(np.asarray(pattern.rowptr))
    col = pattern.col if isinstance(pattern.col, torch.Tensor) else torch.from_numpy(np.asarray(pattern.col))
    scale_r = float(r.abs().max())
    worst_r = worst_A = scale_A = 0.0
    for k, node in enumerate(S.node_ids):
        for i in range(3):
            row = node * 3 + i
            lo, hi = int(rowptr[row]), int(rowptr[row + 1])
            exp, r_exp = S.row(k, i, col[lo:hi].cpu().numpy())
            got = A[lo:hi].cpu().numpy()
            scale_A = max(scale_A, float(np.abs(exp).max()))
            worst_A = max(worst_A, float(np.abs(got - exp).max()))
            worst_r = max(worst_r, abs(float(r[row]) - r_exp))
    print(f"{n_el}: {len(nodes)} nodes, {len(S.elements)} elements: residual {worst_r / scale_r:.2e} tangent {worst_A / scale_A:.2e}")
    assert len(nodes) >= 50
    assert worst_r / scale_r < 1e-12
    assert worst_A / scale_A < 1e-11
