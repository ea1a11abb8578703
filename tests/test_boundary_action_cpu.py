"""The matrix-free action of the contact and follower-pressure tangents (csrc/kernels_face_action.hpp), without a GPU:
(1) include/mimi_hip.h declares the entries and says what they stand in for, the library exports them, mimi_amd._capi.EXPORTS
    matches the header, the ABI version has not moved (entries were added, none changed), null handles are errors;
(2) the new kernels spill no register in contact.hip and pressure.hip, and pressure.hip still holds its 10 face symbols;
(3) the inputs of tests/test_boundary_action_gpu.py: on every face of every case the long-double reference's |K| |v| is not
    zero for the vectors used there (that contact is partial on these bodies is tests/test_faces_cpu.py's assertion)."""
import ctypes
import functools
import os
import re
import shutil
import zlib

import numpy as np
import pytest

import _face_cases as fc
import _patches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACE_ENTRIES = tuple(f"mimi_hip_{kind}_{what}" for kind in ("contact", "follower") for what in ("linearize", "apply_tangent", "action_info"))
ENTRIES = FACE_ENTRIES + ("mimi_hip_linear_add_boundary_operator",)
ALL = [(c, -1) for c in list(_patches.CASES) + fc.BLOCKS] + fc.ORDERS_ALL
PRESSURE_KINDS, CONTACT_KINDS = ("uniform", "nodal"), ("plane", "sphere")
N_VECTORS = 2
HAVE_HIPCC = os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")


@functools.lru_cache(maxsize=None)
def vectors(case, axis, side):
    """the two standard normal vectors of a face of a case, shared and read-only"""
    seed = zlib.crc32(f"{case} {axis} {side}".encode())
    v = np.random.default_rng(seed).standard_normal((N_VECTORS, fc.product_patch(case).n_vdofs))
    v.setflags(write=False)
    return v


def reference_products(ref_K, v):
    """(K v, |K| |v|) of the long-double reference, in doubles"""
    K = np.asarray(ref_K)
    Kv = (K @ v.astype(K.dtype).T).T
    scale = (np.abs(K) @ np.abs(v).astype(K.dtype).T).T
    return np.asarray(Kv, dtype=np.float64), np.asarray(scale, dtype=np.float64)


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
def header():
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        return f.read()


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mimi_hip_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_entries_and_what_they_stand_in_for():
    names = declared_functions()
    text = header()
    for entry in ENTRIES:
        assert entry in names
    for entry in ("mimi_hip_contact_linearize", "mimi_hip_follower_linearize", "mimi_hip_linear_add_boundary_operator"):
        before = text[:text.index("int " + entry)]
        comment = before[before.rindex("/*"):]
        assert "MortarContact::AddBoundaryResidualAndGrad" in comment and "mortar_contact.cpp:353-421" in comment, entry
        assert "SparseMatrix::Mult" in comment, entry
    assert re.search(r"^#define MIMI_HIP_ABI_VERSION 12$", text, flags=re.M)


def test_library_exports_the_entries_and_null_handles_are_errors():
    from mimi_amd import _capi, build
    path = build.build()
    import torch  # noqa: F401  (ahead of the library, as _capi.lib() loads it)
    lib = ctypes.CDLL(path)
    for entry in ENTRIES:
        assert hasattr(lib, entry), entry
        assert entry in _capi.EXPORTS
    lib.mimi_hip_abi_version.restype = ctypes.c_int
    assert lib.mimi_hip_abi_version() == 12
    assert sorted(_capi.EXPORTS) == declared_functions()
    lib.mimi_hip_last_error.restype = ctypes.c_char_p
    x = (ctypes.c_double * 4)()
    for kind in ("contact", "follower"):
        lin, app, info = (getattr(lib, f"mimi_hip_{kind}_{what}") for what in ("linearize", "apply_tangent", "action_info"))
        lin.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        app.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        info.argtypes, info.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int64
        assert lin(None, x) != 0 and b"null" in lib.mimi_hip_last_error()
        assert app(None, 1.0, x, x) != 0 and b"null" in lib.mimi_hip_last_error()
        assert info(None, 0) == -1
    add = lib.mimi_hip_linear_add_boundary_operator
    add.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double]
    assert add(None, 0, None, 1.0) != 0 and b"null" in lib.mimi_hip_last_error()


def test_python_front_ends_carry_the_methods():
    from mimi_amd.integrators import FollowerPressure, MortarContact
    from mimi_amd.linear import LinearSolver
    for cls in (MortarContact, FollowerPressure):
        for method in ("Linearize", "ApplyTangent", "LinearizationBytes"):
            assert callable(getattr(cls, method))
    assert (MortarContact._operator_kind, FollowerPressure._operator_kind) == (0, 1)
    assert callable(LinearSolver.AddBoundaryOperator)


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc: nothing to compile")
@pytest.mark.parametrize("source", ["contact.hip", "pressure.hip"])
def test_action_kernels_spill_no_register(source):
    from mimi_amd import isa_lint as L
    counts = L.spill_counts(L.assembly(source))
    new = {n: c for n, c in counts.items() if "boundary_action_kernel" in n or "boundary_linearize_kernel" in n}
    assert len(new) == 4, sorted(new)                      # the two kernels for DIM 2 / 3
    assert all(c == 0 for c in new.values()), new
    assert not any("pressure" in n or "face_" in n for n in new)
    if source == "pressure.hip":
        assert len({n for n in counts if "pressure" in n or "face_" in n}) == 10


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,order", ALL + fc.ORDERS_CONTACT, ids=lambda c: str(c))
def test_reference_products_are_not_zero_on_any_face(case, order):
    contact_only = (case, order) in fc.ORDERS_CONTACT
    for axis, side in fc.faces(case):
        v = vectors(case, axis, side)
        refs = [fc.contact_reference(case, axis, side, order, kind) for kind in CONTACT_KINDS]
        if not contact_only:
            refs += [fc.pressure_reference(case, axis, side, order, kind) for kind in PRESSURE_KINDS]
        for ref in refs:
            Kv, scale = reference_products(ref.K, v)
            assert np.isfinite(Kv).all() and (scale.max(axis=1) > 0).all() and (np.abs(Kv).max(axis=1) > 0).all()
