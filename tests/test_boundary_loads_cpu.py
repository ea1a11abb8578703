"""Traction and pressure markers of the facade (no GPU): the reference's BCMarker shapes (utils/boundary_conditions.cpp:
43-69), the C ABI of the follower-pressure integrator, and the host traction right-hand side in closed form.

On an open-uniform B-spline block with control points at the Greville abscissae the face is a rectangle and dA0 is
constant, so int N_a dA0 = prod over the face's directions d of L_d (t_(i+p+1) - t_i) / (p + 1): the integral of one
B-spline of the knot vector t on [0, 1]."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_markers_chain_and_store_the_reference_shapes():
    from mimi_amd.solid import BoundaryConditions
    bc = BoundaryConditions()
    out = bc.initial.traction(2, 0, 1.5).traction(2, 1, -0.25).traction(3, 2, 4.0).pressure(1, 7.0).pressure(4, -2.0)
    assert out is bc.initial
    assert bc.initial.traction_ == {2: {0: 1.5, 1: -0.25}, 3: {2: 4.0}}
    assert bc.initial.pressure_ == {1: 7.0, 4: -2.0}
    # the value of a later call replaces the earlier one (std::map assignment)
    bc.initial.traction(2, 0, 3.0).pressure(1, 8.0)
    assert bc.initial.traction_[2][0] == 3.0 and bc.initial.pressure_[1] == 8.0
    with pytest.raises(RuntimeError, match="only available for initial config"):
        bc.current.traction(0, 0, 1.0)
    with pytest.raises(RuntimeError, match="only available for initial config"):
        bc.current.pressure(0, 1.0)
    assert bc.current.traction_ == {} and bc.current.pressure_ == {}
    # the markers that existed before keep working on both configurations
    bc.current.contact(1, object())
    bc.initial.dirichlet(0, 1).body_force(1, -9.81)


def test_header_declares_and_library_exports_the_pressure_entries():
    from mimi_amd import build, _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mimi_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mimi_hip_pressure_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(["mimi_hip_pressure_create", "mimi_hip_pressure_destroy", "mimi_hip_pressure_set_stream",
                               "mimi_hip_pressure_synchronize", "mimi_hip_pressure_set_value",
                               "mimi_hip_pressure_face_nodes", "mimi_hip_pressure_set_nodal",
                               "mimi_hip_pressure_add_residual", "mimi_hip_pressure_add_residual_and_grad",
                               "mimi_hip_pressure_last_history"])
    assert set(declared) <= set(_capi.EXPORTS)
    import torch  # noqa: F401  (torch's HIP runtime first, as _capi.lib() loads it)
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in declared)
    # the Python struct matches the header's field list
    body = re.search(r"typedef struct mimi_hip_pressure_tables \{(.*?)\} mimi_hip_pressure_tables;", text, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert [f[0] for f in _capi.PressureTables._fields_] == fields


def bspline_integrals(n_el, p, L):
    """int_0^L of every B-spline of the open-uniform knot vector with n_el spans on [0, L]"""
    k = np.concatenate([np.zeros(p), np.arange(n_el + 1) / n_el, np.ones(p)])
    n = len(k) - p - 1
    return L * np.array([(k[i + p + 1] - k[i]) / (p + 1) for i in range(n)])


BLOCKS = [((4, 3), 1, (2.5, 0.7)), ((5, 3), 2, (1.5, 3.2)), ((3, 4), 3, (0.6, 2.0)),
          ((3, 2, 4), 1, (1.3, 2.2, 0.9)), ((4, 3, 2), 2, (2.0, 0.5, 1.7)), ((2, 3, 3), 3, (0.8, 1.9, 2.6))]
FACES3 = {1: (0, 0), 2: (0, 1), 3: (1, 0), 4: (1, 1), 5: (2, 0), 6: (2, 1)}


@pytest.mark.parametrize("n_el,p,lengths", BLOCKS, ids=lambda c: str(c).replace(" ", ""))
def test_traction_rhs_closed_form(n_el, p, lengths):
    import mimi_amd
    from mimi_amd import solid
    from oracle import iga
    dim = len(n_el)
    patch = mimi_amd.BSplinePatch.block(n_el, p, lengths)
    faces = {k: v for k, v in FACES3.items() if v[0] < dim}
    rng = np.random.default_rng(7)
    for bid in range(2 * dim):
        axis, side = faces[bid + 1]
        t = rng.uniform(-2.0, 2.0, dim)
        f = solid.traction_vector(patch, axis, side, {i: t[i] for i in range(dim)}).reshape(-1, dim)
        area0 = np.prod([lengths[d] for d in range(dim) if d != axis])
        # per component the entries sum to t A0
        assert np.allclose(f.sum(axis=0), t * area0, rtol=1e-13, atol=0)
        # each node: t int N_a dA0 from the 1-D integrals; zero off the face
        ints = [bspline_integrals(n_el[d], p, lengths[d]) for d in range(dim)]
        mi = patch.node_multi_index()
        on = mi[axis] == (0 if side == 0 else patch.n_ctrl[axis] - 1)
        expect = np.ones(patch.n_nodes)
        for d in range(dim):
            if d != axis:
                expect *= ints[d][mi[d]]
        expect[~on] = 0.0
        assert np.abs(f - expect[:, None] * t[None, :]).max() <= 1e-14 * np.abs(t).max() * expect.max()
    # the facade's right-hand side: body force + traction, Dirichlet dofs zero, the body force unchanged
    rowptr, _ = iga.Patch.block(n_el, p, lengths).sparsity()
    rowptr = np.asarray(rowptr, dtype=np.int64)
    body = {dim - 1: -9.81}
    dirichlet = np.unique(np.concatenate([patch.boundary_nodes(a, 0) * dim + a for a in range(dim)]))
    traction = {2 * dim - 1: {0: 0.75, dim - 1: -3.0}}          # bid 2 dim - 1 -> attribute 2 dim: the face {xi_last = 1}
    _, _, rhs_body = solid._assemble_mass_viscosity_rhs(patch, rowptr, 1.0, -1.0, body)
    rhs_b = solid._load_vector(patch, faces, {}, rhs_body.copy(), dirichlet)
    rhs_t = solid._load_vector(patch, faces, traction, np.zeros(patch.n_vdofs), dirichlet)
    rhs_bt = solid._load_vector(patch, faces, traction, rhs_body.copy(), dirichlet)
    assert np.all(rhs_bt[dirichlet] == 0.0) and np.all(rhs_t[dirichlet] == 0.0)
    assert np.any(rhs_t != 0.0)
    tv = solid.traction_vector(patch, dim - 1, 1, traction[2 * dim - 1])
    tv[dirichlet] = 0.0
    assert np.array_equal(rhs_t, tv)
    assert np.abs(rhs_bt - rhs_t - rhs_b).max() <= 1e-14 * np.abs(rhs_bt).max()
    # no traction: the body-force vector alone, as before the markers existed
    ref = rhs_body.copy()
    ref[dirichlet] = 0.0
    assert np.array_equal(rhs_b, ref)


def test_traction_refuses_a_rational_patch():
    import mimi_amd
    from mimi_amd import solid
    patch = mimi_amd.BSplinePatch.block((2, 2), 2)
    rational = mimi_amd.BSplinePatch(patch.degrees, patch.knots, patch.control_points, np.ones(patch.n_nodes))
    with pytest.raises(RuntimeError, match="rational patch"):
        solid.traction_vector(rational, 0, 1, {0: 1.0})


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not __import__("shutil").which("hipcc"),
                    reason="no hipcc: nothing to compile")
def test_pressure_kernels_spill_no_register():
    from mimi_amd import isa_lint as L
    spills = {n: c for n, c in L.spill_counts(L.assembly("pressure.hip")).items() if "pressure" in n or "face_" in n}
    # face kernels and the shared row gather (face_common.hpp) for DIM 2 / 3 with and without the tangent, the shared
    # fixed-order sum and pair positions
    assert len(spills) == 10, sorted(spills)
    assert all(c == 0 for c in spills.values()), spills
