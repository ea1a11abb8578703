"""The packed S3 tiles of the symmetric-half degree-2 kernel (csrc/p2_tile_map.hpp: the three chains of a b1 in two tiles, the
rider's rows moved into idle operand rows, its results stored and carried from where they lie) against the CPU oracle, at the bars
of the degree-2 parity tests (test_domain_gpu.py: residual 1e-12, analytic tangent 1e-11, relative in the max-norm).

Columns of 1 / 2 / 5 elements: no carry, the one-step carry only, the two-step carry (2,2) -> (1,1) -> (0,0) that the rider's
pair 8 starts from the second tile.  5 x 4 x 9: columns longer than a segment; cut into the boxes z < 8 and z >= 8 the first
box is small enough for the segment path (two segments of four elements: a segment end stores the carried rows of hosts and
riders).  Every launch here walks ONE unit per workgroup (20 columns are far below the 4096 at which a workgroup gets a second
one: asserted through NonlinearSolid.LastWalkGeometry); the walk across unit boundaries with packed tiles live is
tests/test_wgsym_walk_gpu.py."""
import numpy as np
import pytest

from _cases import oracle_material, product_material, synthetic_u

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 1), (3, 3, 2), (3, 3, 5), (5, 4, 9)]


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


_oracle = {}


def oracle(n_el, matname):
    """(patch, oracle integrator, u, residual, tangent) of the whole block: computed once, shared, never written to."""
    key = (n_el, matname)
    if key not in _oracle:
        from oracle import iga, ref_path as rp
        P = iga.Patch.block(n_el, 2)
        D = rp.DomainOracle(P, oracle_material(matname), n_threads=2)
        D.set_dt(0.5)
        u = synthetic_u(P, scale=0.05 if matname == "neohook" else 0.02)
        r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
        D.add_domain_residual_and_grad(u, 1.0, r, A, rp.TANGENT_EXACT)
        for x in (u, r, A):
            x.setflags(write=False)
        _oracle[key] = (P, D, u, r, A)
    return _oracle[key]


def product(n_el, D, matname, element_box=None):
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    pattern = CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)
    G = NonlinearSolid("domain", product_material(matname), pattern, patch=mimi_amd.BSplinePatch.block(n_el, 2),
                       element_box=element_box).Prepare()
    assert G.path_ == 1
    G.dt_ = 0.5
    return G


@pytest.mark.parametrize("n_el", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_oracle(n_el):
    P, D, u, r_o, A_o = oracle(n_el, "neohook")
    G = product(n_el, D, "neohook")
    r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
    assert G.LastWalkGeometry() == (n_el[2], 1)              # whole columns, one per workgroup
    er, eA = relmax(r, r_o), relmax(A, A_o)
    print(f"{n_el}: residual {er:.2e} tangent {eA:.2e}")
    assert er < 1e-12
    assert eA < 1e-11


def test_segment_path_on_a_small_box():
    n_el = (5, 4, 9)
    P, D, u, r_o, A_o = oracle(n_el, "neohook")
    r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    # 5 x 4 x 8: 20 columns, cut into two segments of four elements each (WGSYM_SPLIT_BELOW); then the last layer
    for begin, end, seg_len in (([0, 0, 0], [5, 4, 8], 4), ([0, 0, 8], [5, 4, 9], 1)):
        G = product(n_el, D, "neohook", element_box=(begin, end))
        G.AddDomainResidualAndGrad(u, 1.0, r, A)
        assert G.LastWalkGeometry() == (seg_len, 1)
    er, eA = relmax(r, r_o), relmax(A, A_o)
    print(f"boxes of {n_el}: residual {er:.2e} tangent {eA:.2e}")
    assert er < 1e-12
    assert eA < 1e-11


def test_assembled_matrix_is_symmetric_to_the_bit():
    """Every entry the kernel stores twice from ONE computed value equals its mirror bitwise: the blocks of two different
    components i != j (off-diagonal blocks, stored as computed and transposed) and, inside a diagonal block i == j, the node pairs
    on different y-planes (chains a1 != b1: only a1 > b1 is contracted).  What is left, i == j with both nodes on one y-plane
    (chains a1 == b1), is computed on both sides of the diagonal, the two table variants D.B and B.D summed in exchanged order:
    equal to rounding, not to the bit -- measured before and after the packed tiles alike on this block: 2452 of 94221 entries
    differ from their mirror, by at most 7.6e-17 of max|A|, all of them of that kind; none of the entries above does.  The
    bound for them: two sums of the same <= 8 x 64 x 9 products in another order, each within a few units of 2^-53 max|A|."""
    n_el = (3, 3, 5)
    P, D, u, _, _ = oracle(n_el, "neohook")
    A = np.zeros(D.nnz)
    G = product(n_el, D, "neohook")
    G.AddDomainResidualAndGrad(u, 1.0, np.zeros(P.n_vdofs), A)
    assert G.LastWalkGeometry() == (5, 1)
    n = len(D.rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(D.rowptr))
    cols = D.col.astype(np.int64)
    by_entry, by_mirror = np.argsort(rows * n + cols), np.argsort(cols * n + rows)
    assert np.array_equal(rows[by_entry], cols[by_mirror]) and np.array_equal(cols[by_entry], rows[by_mirror])   # (the pattern is)
    assert np.abs(A).max() > 0
    a, b = A[by_entry], A[by_mirror]
    r, c = rows[by_entry], cols[by_entry]
    nodes_x, nodes_y = n_el[0] + 2, n_el[1] + 2
    y_plane = lambda v: (v // 3 // nodes_x) % nodes_y                      # vdof = 3 node + component, node = x + nx (y + ny z)
    stored_twice = (r % 3 != c % 3) | (y_plane(r) != y_plane(c))
    print(f"stored twice {int(stored_twice.sum())} of {A.size}; elsewhere {int((a != b).sum())} differ from their mirror by "
          f"<= {np.abs(a - b).max() / np.abs(A).max():.2e} max|A|")
    assert stored_twice.sum() > A.size // 2
    assert np.array_equal(a[stored_twice], b[stored_twice])
    assert np.abs(a - b).max() <= 8 * 2.0 ** -53 * np.abs(A).max()


def test_nine_block_kernel_j2():
    """The other materials' kernel shares the contraction text and keeps a tile per chain."""
    n_el = (3, 3, 5)
    P, D, u, r_o, A_o = oracle(n_el, "j2")
    G = product(n_el, D, "j2")
    r, A = np.zeros(P.n_vdofs), np.zeros(D.nnz)
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
    assert G.LastKernelFamily() == "tensor_p2_two_phase" and G.LastWalkGeometry() == (0, 0)     # not the symmetric-half kernel
    er, eA = relmax(r, r_o), relmax(A, A_o)
    print(f"j2 {n_el}: residual {er:.2e} tangent {eA:.2e}")
    assert er < 1e-12
    assert eA < 1e-11
