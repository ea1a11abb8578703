"""Field output without a GPU: the C surface (header, export list, the library built here), the component counts, the
facade's name validation, the node-order helper for scalar fields, the yardstick of tests/test_fields_gpu.py pinned
against closed forms (tests/_fields.py), and the kernels' per-point routine compiled for the host (tests/host_fields.hip)
against that yardstick."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _fields
from test_abi_cpu import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mimi_hip_field_components", "mimi_hip_domain_point_field", "mimi_hip_domain_nodal_field",
       "mimi_hip_domain_set_shape_values"]


def test_header_and_export_list_declare_the_field_entries():
    from mimi_amd import _capi
    names = declared_functions()
    for n in NEW:
        assert n in names and n in _capi.EXPORTS
    text = open(os.path.join(ROOT, "include", "mimi_hip.h")).read()
    # the fifth entry: the enum with its five ids
    for k, name in enumerate(("CAUCHY", "VON_MISES", "DET_F", "EQPS", "TEMPERATURE")):
        assert f"MIMI_HIP_FIELD_{name} = {k}" in text
    assert "enum mimi_hip_field {" in text
    assert "#define MIMI_HIP_ABI_VERSION 12" in text


def test_library_exports_the_field_entries_and_counts_components():
    from mimi_amd import build
    path = build.build()
    import torch  # noqa: F401  (before the library, as _capi.lib() does)
    lib = ctypes.CDLL(path)
    for n in NEW:
        assert hasattr(lib, n)
    assert lib.mimi_hip_abi_version() == 12
    fc = lib.mimi_hip_field_components
    fc.argtypes = [ctypes.c_int, ctypes.c_int]
    for dim in (2, 3):
        assert [fc(f, dim) for f in range(5)] == [dim * dim, 1, 1, 1, 1]
        assert fc(5, dim) == -1 and fc(-1, dim) == -1 and fc(100, dim) == -1


def test_facade_validates_names_before_anything_else():
    import mimi_amd
    from mimi_amd.integrators import NonlinearSolid
    assert tuple(NonlinearSolid.FIELDS) == _fields.FIELDS
    assert [NonlinearSolid.FIELDS[n] for n in _fields.FIELDS] == [0, 1, 2, 3, 4]
    G = NonlinearSolid("domain", None, None)
    with pytest.raises(ValueError, match="unknown field"):
        G.PointField("mises", None)
    with pytest.raises(ValueError, match="unknown field"):
        G.NodalField("stress", None, None)
    nl = mimi_amd.NonlinearSolid()
    with pytest.raises(ValueError, match="unknown field"):
        nl.field("sigma")
    with pytest.raises(ValueError, match="where"):
        nl.field("von_mises_stress", where="cells")
    with pytest.raises(RuntimeError, match="setup"):
        nl.field("von_mises_stress")


def test_reference_numbering_of_a_scalar_nodal_field():
    import mimi_amd
    nl = mimi_amd.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "balken.mesh"))
    nl.elevate_degrees(2)
    nl.subdivide(1)
    dim = nl.mesh_dim()
    n = nl.n_vertices()
    rng = np.random.default_rng(5)
    s = rng.standard_normal(n)
    v = rng.standard_normal((n, dim))
    v[:, 1] = s
    ref_v = nl.in_reference_numbering(v.ravel())
    ref_s = nl.in_reference_numbering(s, ncomp=1)
    assert ref_s.shape == (n,)
    assert np.array_equal(ref_s, ref_v.reshape(-1, dim)[:, 1])
    assert not np.array_equal(ref_s, s)                      # (the order is not the identity on this mesh)
    t = rng.standard_normal((n, dim * dim))
    ref_t = nl.in_reference_numbering(t, ncomp=dim * dim).reshape(n, dim * dim)
    assert np.array_equal(ref_t, t[nl.mfem_node_order()])
    # the default is unchanged: dim components per node
    assert np.array_equal(nl.in_reference_numbering(v.ravel()), v[nl.mfem_node_order()].ravel())


@pytest.mark.parametrize("n_el,p", [((3, 4), 2), ((3, 2, 2), 2)], ids=["2d", "3d"])
def test_yardstick_reproduces_closed_forms(n_el, p):
    """homogeneous F0: the yardstick's neo-Hookean sigma is mu/J (F0 F0^T - I) + lambda (J - 1) I at every point, and the
    lumped projection of a constant is that constant at every node.  1e-13 relative to the largest entry: the closed form
    and the oracle's material are a handful of fp64 operations each on numbers of one magnitude."""
    from _cases import oracle_material
    from oracle import iga, ref_path as rp
    P = iga.Patch.block(n_el, p)
    dim = P.dim
    D = rp.DomainOracle(P, oracle_material("neohook"))
    F0 = _fields.homogeneous_F(dim)
    u = _fields.homogeneous_u(P.ctrl, F0)
    F = _fields.deformation_gradients(D.tables, u, dim)
    assert np.abs(F - F0).max() < 1e-13
    pts = _fields.point_fields(D, u, 0.05)
    sig = _fields.closed_form_sigma("neohook", F0)
    scale = np.abs(sig).max()
    assert np.abs(pts["cauchy_stress"] - sig.ravel(order="F")).max() <= 1e-13 * scale
    assert np.abs(sig - sig.T).max() <= 1e-13 * scale
    q = _fields.von_mises_of(sig)
    assert np.abs(pts["von_mises_stress"] - q).max() <= 1e-13 * q
    assert np.abs(pts["det_F"] - np.linalg.det(F0)).max() <= 1e-13
    const = np.full(pts["det_F"].shape, 3.25)
    s, w = _fields.nodal_sums(D.tables, P.n_nodes, const)
    assert w.min() > 0
    assert np.abs(s[:, 0] / w - 3.25).max() <= 1e-13 * 3.25
    nod = _fields.nodal_fields(D.tables, P.n_nodes, pts)
    assert np.abs(nod["cauchy_stress"] - sig.ravel(order="F")).max() <= 1e-13 * scale
    # the weights are a partition of the volume
    assert abs(w.sum() - np.prod(n_el)) <= 1e-12 * np.prod(n_el)


@pytest.fixture(scope="module")
def host_fields():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = os.path.join(ROOT, "tests", "_build", "libhost_fields.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result",
                           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "host_fields.hip")])
    return ctypes.CDLL(out)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", _fields.MATERIALS)
def test_point_routine_on_host_against_the_yardstick(host_fields, name, dim):
    """what a lane of the field kernels computes at its point (field_at_point, compiled for the host), every field of every
    material, fresh and advanced states, against the yardstick's sigma = P F^T / det F from the oracle's P.  1e-11 relative
    to the largest stress component, the bar of the device parity test (measured here: 2e-14 for J2Linear, 2e-15 else)."""
    from _cases import oracle_material, product_material
    from oracle import ref_path as rp
    from test_materials_host_cpu import ptr, random_state
    mo, mp = oracle_material(name), product_material(name)._c_struct()
    rng = np.random.default_rng(7 + dim)
    for trial in range(60):
        F = np.eye(dim) + 10 ** rng.uniform(-2.5, -1.2) * rng.standard_normal((dim, dim))
        m1, m2, eqps = random_state(name, dim, rng, fresh=trial % 2 == 0)
        Po, _ = rp.point_pk1(mo, F, dt=0.05, plastic_strain=m1, eqps=eqps, temperature=20.0, state2=m2)
        sig = _fields.cauchy_of(Po, F)
        expect = {0: sig.ravel(order="F"), 1: np.array([_fields.von_mises_of(sig)]), 2: np.array([np.linalg.det(F)]),
                  3: np.array([eqps]), 4: np.array([20.0])}
        Fc = np.ascontiguousarray(F.T).ravel()
        a1, a2 = np.ascontiguousarray(m1.T).ravel().copy(), np.ascontiguousarray(m2.T).ravel().copy()
        for field, value in expect.items():
            f = np.full(dim * dim, np.nan)
            st = host_fields.host_field(ctypes.byref(mp), dim, ctypes.c_double(0.05), field, ptr(Fc), ptr(a1), ptr(a2),
                                        ctypes.c_double(eqps), ctypes.c_double(20.0), ptr(f))
            assert st == 0
            scale = np.abs(sig).max() if field < 2 else max(np.abs(value).max(), 1e-300)
            assert np.abs(f[:len(value)] - value).max() <= 1e-11 * scale, (trial, field)
            if field >= 3:
                assert f[0] == value[0]                  # the state comes back as it is
        assert np.array_equal(a1, np.ascontiguousarray(m1.T).ravel()) and np.array_equal(a2, np.ascontiguousarray(m2.T).ravel())
