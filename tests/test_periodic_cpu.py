"""Periodic and constant-velocity markers of the facade (no GPU): the reference's BCMarker shapes
(utils/boundary_conditions.cpp:127-159), the refusals of setup(), the periodic node map and the C ABI of the fold."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = os.path.join(ROOT, "tests", "golden", "meshes")


def test_markers_chain_and_store_the_reference_shapes():
    from mimi_amd.solid import BoundaryConditions
    bc = BoundaryConditions()
    out = bc.initial.periodic(6, 4).periodic(3, 5).constant_velocity(1, 2, 0.5).constant_velocity(1, 0, -1.0)
    assert out is bc.initial
    assert bc.initial.periodic_boundaries_ == {6: 4, 3: 5}
    assert bc.initial.constant_velocity_ == {1: {2: 0.5, 0: -1.0}}
    # constant_velocity implies the Dirichlet marker (boundary_conditions.cpp:132)
    assert bc.initial.dirichlet_ == [(1, 2), (1, 0)]
    bc.initial.constant_velocity(1, 2, 0.75)
    assert bc.initial.constant_velocity_[1][2] == 0.75
    with pytest.raises(RuntimeError, match="PeriodicBoundary boundary condition is currently only available for initial"):
        bc.current.periodic(1, 2)
    with pytest.raises(RuntimeError, match="ConstantVelocity boundary condition is currently only available for initial"):
        bc.current.constant_velocity(0, 0, 1.0)
    assert bc.current.periodic_boundaries_ == {} and bc.current.constant_velocity_ == {} and bc.current.dirichlet_ == []


def solid(mesh, setup_bc):
    import mimi_amd
    nl = mimi_amd.NonlinearSolid()
    nl.read_mesh(os.path.join(MESHES, mesh))
    nl.elevate_degrees(1)
    mat = mimi_amd.CompressibleOgdenNeoHookean()
    mat.density = 1.0
    mat.set_young_poisson(2100, 0.3)
    nl.set_material(mat)
    bc = mimi_amd.BoundaryConditions()
    setup_bc(bc)
    nl.boundary_condition = bc
    return nl


# cube-nurbs.mesh: attribute -> (axis, side) = {1: (2, 0), 2: (2, 1), 3: (1, 0), 4: (0, 1), 5: (1, 1), 6: (0, 0)}
@pytest.mark.parametrize("marks,match", [
    (lambda bc: bc.initial.periodic(6, 1), "not the two opposite faces"),
    (lambda bc: bc.initial.periodic(6, 6), "appears in two pairs"),
    (lambda bc: bc.initial.periodic(7, 4), "no boundary attribute 7"),
    (lambda bc: bc.initial.periodic(0, 4), "no boundary attribute 0"),
    (lambda bc: bc.initial.periodic(6, 4).periodic(4, 6), "appears in two pairs"),
    (lambda bc: bc.initial.periodic(6, 4).pressure(3, 1.0), "pressure marker on boundary 3"),
    (lambda bc: bc.initial.periodic(6, 4).traction(5, 0, 1.0), "traction marker on boundary 5"),
    (lambda bc: (bc.initial.periodic(3, 5), bc.current.contact(2, object())), "contact marker on boundary 2"),
])
def test_setup_refuses(marks, match):
    nl = solid("cube-nurbs.mesh", marks)
    with pytest.raises(RuntimeError, match=match):
        nl.setup(1)


def test_periodic_takes_one_based_attributes():
    # attribute 6 / 4 are x = 0 / x = 1: the 0-based reading (faces 7 / 5) would be refused or join y
    nl = solid("cube-nurbs.mesh", lambda bc: bc.initial.periodic(6, 4))
    assert nl._periodic_axes(nl.boundary_condition) == [0]
    nl = solid("cube-nurbs.mesh", lambda bc: bc.initial.periodic(1, 2).periodic(3, 5))
    assert nl._periodic_axes(nl.boundary_condition) == [1, 2]
    # a pressure on a face that is not joined stays allowed
    nl = solid("cube-nurbs.mesh", lambda bc: bc.initial.periodic(6, 4).pressure(1, 2.0))
    assert nl._periodic_axes(nl.boundary_condition) == [0]


GRIDS = [((5, 4), [0]), ((5, 4), [1]), ((5, 4), [0, 1]), ((3, 3), [0, 1]), ((2, 4), [0]),
         ((5, 4, 3), [0]), ((5, 4, 3), [0, 2]), ((5, 4, 3), [0, 1, 2]), ((4, 4, 4), [1]), ((2, 3, 2), [0, 1, 2])]


@pytest.mark.parametrize("n,axes", GRIDS, ids=lambda c: str(c).replace(" ", ""))
def test_node_map(n, axes):
    from mimi_amd.integrators import periodic_node_map
    nm = periodic_node_map(n, axes)
    assert nm.shape == (int(np.prod(n)),)
    n_f = int(np.prod([n[d] - (1 if d in axes else 0) for d in range(len(n))]))
    # onto [0, n_f)
    assert nm.min() == 0 and nm.max() == n_f - 1 and len(np.unique(nm)) == n_f
    # a node merges with 2^(number of periodic axes on whose last plane or first plane it lies)
    mi = np.array(np.unravel_index(np.arange(len(nm)), tuple(reversed(n))))[::-1]
    seam = sum(((mi[d] == 0) | (mi[d] == n[d] - 1)).astype(int) for d in axes)
    counts = np.bincount(nm)[nm]
    assert np.array_equal(counts, 2 ** seam)
    # merged nodes face each other across the seam, and a folded node has the index of its lowest copy
    for d in axes:
        first, last = mi[d] == 0, mi[d] == n[d] - 1
        assert np.array_equal(nm[first], nm[last])
    _, lowest = np.unique(nm, return_index=True)
    reduced = tuple(reversed([n[d] - (1 if d in axes else 0) for d in range(len(n))]))
    assert np.array_equal(np.ravel_multi_index(tuple(mi[::-1][:, lowest]), reduced), np.arange(n_f))


@pytest.mark.parametrize("mesh,pairs,axes", [("square-nurbs.mesh", {3: 4}, [0]), ("square-nurbs.mesh", {3: 4, 1: 2}, [0, 1]),
                                             ("cube-nurbs.mesh", {6: 4}, [0]), ("cube-nurbs.mesh", {6: 4, 3: 5}, [0, 1]),
                                             ("cube-nurbs.mesh", {6: 4, 3: 5, 1: 2}, [0, 1, 2])])
def test_dof_map_of_the_facade(mesh, pairs, axes):
    from mimi_amd.integrators import periodic_node_map

    def marks(bc):
        for b0, b1 in pairs.items():
            bc.initial.periodic(b0, b1)
    nl = solid(mesh, marks)
    nl.subdivide(1)
    dm = nl.dof_map("displacement")
    n_ctrl = nl.patch().n_ctrl
    assert np.array_equal(dm, periodic_node_map(n_ctrl, axes))
    assert len(np.unique(dm)) == int(np.prod([n_ctrl[d] - (1 if d in axes else 0) for d in range(len(n_ctrl))]))
    # without the marker: the identity
    plain = solid(mesh, lambda bc: None)
    assert np.array_equal(plain.dof_map("displacement"), np.arange(plain.patch().n_nodes))


FOLD_ENTRIES = ["mimi_hip_fold_create", "mimi_hip_fold_destroy", "mimi_hip_fold_info", "mimi_hip_fold_pattern",
                "mimi_hip_fold_set_stream", "mimi_hip_fold_synchronize", "mimi_hip_fold_expand", "mimi_hip_fold_add"]


def test_header_declares_and_library_exports_the_fold_entries():
    from mimi_amd import build, _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mimi_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mimi_hip_fold_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(FOLD_ENTRIES)
    assert set(declared) <= set(_capi.EXPORTS)
    assert "#define MIMI_HIP_ABI_VERSION 12" in text
    import torch  # noqa: F401  (torch's HIP runtime first, as _capi.lib() loads it)
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in declared)
    assert lib.mimi_hip_abi_version() == 12
    assert "fold.hip" in build.SOURCES


def test_fold_kernels_spill_no_register():
    from mimi_amd import isa_lint as L
    spills = {n: c for n, c in L.spill_counts(L.assembly("fold.hip")).items() if "fold" in n}
    # pattern (count, fill), matrix (with / without residual), residual, expand
    assert len(spills) == 6, sorted(spills)
    assert all(c == 0 for c in spills.values()), spills
