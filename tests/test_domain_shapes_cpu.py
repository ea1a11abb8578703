"""The inputs of tests/test_domain_shapes_gpu.py, vetted on the oracle alone (no GPU): every patch of tests/_patches.py has
a positive geometry determinant at every point, the oracle's exact tangent is the derivative of its own residual there, the
displacements keep det F positive, and the J2 commit leaves a mixed elastic / plastic state -- so a parity test on the device
cannot pass on a degenerate input, and its reference is itself checked at these shapes."""
import numpy as np
import pytest
import scipy.sparse as sp

import _fields
import _patches
from _patches import CASES


@pytest.mark.parametrize("case", list(CASES))
def test_patch_is_what_its_name_says(case):
    degrees, inner, _ = CASES[case]
    P, B = _patches.patches(case)
    assert P.p == list(degrees) == B.degrees
    assert P.n == B.n_ctrl and P.m == B.n_spans and P.n_el == B.n_elements
    assert np.array_equal(P.ctrl, B.control_points)
    for d, (p, k) in enumerate(zip(degrees, inner)):
        assert np.array_equal(P.knots[d], np.array([0.0] * (p + 1) + list(k) + [(max(k) + 1 if len(k) else 1.0)] * (p + 1)))
    # repeated interior knots <=> the first function of some span is not the span's index
    first_is_span = all(np.array_equal(P.spans[d] - P.p[d], np.arange(P.m[d])) for d in range(P.dim))
    assert first_is_span == (not case.startswith(("rep2d", "rep3d_p2", "rep3d_p3", "mix2d_31")))
    # an interior element along every axis that has room for one, and at most 125 points per element
    assert max(P.m) >= 3 or case.startswith("mix3d_3")
    assert int(np.prod(P.quad_points_per_dir())) <= 125


def vet(ref, case, matname):
    P, D = ref.P, ref.D
    assert D.det.min() > 0.0
    print(f"{case} {matname}: {P.n_el} elements, {D.weight.shape[1]} points, min det {D.det.min():.3f}")
    # the displacements keep every point away from inversion (both laws are singular at det F = 0: a quarter of the
    # undeformed volume leaves 1 / det F and log det F of order one)
    for u in (ref.u0, ref.u):
        detF = np.linalg.det(_fields.deformation_gradients(D.tables, u, P.dim))
        assert detF.min() > 0.25
    if D.has_states:
        share = float((D.eqps > 0).mean())
        print(f"{case} {matname}: plastic share {share:.2f}")
        assert 0.1 < share < 0.9
    # exact tangent times a random vector == central difference of the residual (grad_factor folded out)
    rows = np.repeat(np.arange(P.n_vdofs), np.diff(D.rowptr))
    K = sp.csr_matrix((ref.A / _patches.GRAD_FACTOR, (rows, D.col)), shape=(P.n_vdofs, P.n_vdofs))
    v = np.random.default_rng(5).standard_normal(P.n_vdofs)
    # step: 1e-7 of the largest displacement -- the difference quotient's round-off is ~ 1e-16 / 1e-7 = 1e-9 of the result,
    # its truncation error ~ 1e-14; and the shorter the step the less likely a J2 point crosses the yield surface inside it
    # (the residual has a kink there: mix3d_211 at order 5 has a point that a step of 1e-6 crosses)
    h = 1e-7 * np.abs(ref.u).max()
    rp_, rm_ = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs)
    D.add_domain_residual(ref.u + h * v, rp_)
    D.add_domain_residual(ref.u - h * v, rm_)
    fd = (rp_ - rm_) / (2 * h)
    err = np.abs(K @ v - fd).max() / np.abs(fd).max()
    print(f"{case} {matname}: tangent vs central difference {err:.2e}")
    assert err < 1e-6
    # the residual-only call and the residual of the tangent call are one function
    assert np.abs(ref.r - ref.r0).max() <= 1e-13 * np.abs(ref.r0).max()


@pytest.mark.parametrize("case,matname", _patches.PARITY, ids=lambda v: v)
def test_inputs_are_valid_on_the_oracle(case, matname):
    vet(_patches.reference(case, matname), case, matname)


@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("case,order,n_quad", _patches.ORDERS, ids=lambda v: str(v))
def test_quadrature_orders_are_valid_on_the_oracle(case, order, n_quad, matname):
    ref = _patches.reference(case, matname, order)
    assert ref.D.weight.shape[1] == n_quad != int(np.prod([p + 2 for p in ref.P.p]))
    vet(ref, f"{case} order {order}", matname)


@pytest.mark.parametrize("matname", _patches.MATERIALS)
@pytest.mark.parametrize("n_el,p", _patches.BLOCKS, ids=lambda v: str(v))
def test_flat_table_blocks_are_valid_on_the_oracle(n_el, p, matname):
    ref = _patches.block_reference(n_el, p, matname)
    assert ref.P.n_dof == (p + 1) ** 2 and ref.D.weight.shape[1] == (p + 2) ** 2
    vet(ref, f"block {n_el} p{p}", matname)
