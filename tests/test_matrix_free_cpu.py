"""The C surface of the matrix-free tangent action, without a GPU: include/mimi_hip.h declares the three entries, the library
exports them, the ABI version has not moved (entries were added, none changed), and mimi_amd._capi.EXPORTS matches the header."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mimi_hip_domain_linearize", "mimi_hip_domain_apply_tangent", "mimi_hip_linear_set_operator")


def header():
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        return f.read()


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mimi_hip_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_entries_and_what_they_stand_in_for():
    names = declared_functions()
    for entry in ENTRIES:
        assert entry in names
    text = header()
    for entry in ENTRIES:
        # the comment in front of the declaration names the reference's routines the entry stands in for
        before = text[:text.index("int " + entry)]
        comment = before[before.rindex("/*"):]
        assert "AddMultGrad" in comment and "SparseMatrix::Mult" in comment, entry
    assert re.search(r"^#define MIMI_HIP_ABI_VERSION 12$", text, flags=re.M)


def test_library_exports_the_entries_and_the_abi_is_still_12():
    from mimi_amd import _capi, build
    path = build.build()
    import torch  # noqa: F401  (ahead of the library, as _capi.lib() loads it)
    lib = ctypes.CDLL(path)
    for entry in ENTRIES:
        assert hasattr(lib, entry), entry
    lib.mimi_hip_abi_version.restype = ctypes.c_int
    assert lib.mimi_hip_abi_version() == 12
    assert sorted(_capi.EXPORTS) == declared_functions()
    for entry in ENTRIES:
        assert entry in _capi.EXPORTS
