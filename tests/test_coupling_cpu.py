"""The partitioned-coupling surface without a GPU: the C ABI of the coupling surface (include/mimi_hip.h:
mimi_hip_surface_*), its kernels' register budget, and the facade's refusals that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SURFACE_ENTRIES = ["mimi_hip_surface_create", "mimi_hip_surface_destroy", "mimi_hip_surface_set_stream",
                   "mimi_hip_surface_synchronize", "mimi_hip_surface_n_points", "mimi_hip_surface_points",
                   "mimi_hip_surface_add_load"]


def test_header_declares_and_library_exports_the_surface_entries():
    from mimi_amd import build, _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mimi_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mimi_hip_surface_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(SURFACE_ENTRIES)
    assert set(declared) <= set(_capi.EXPORTS)
    assert "#define MIMI_HIP_ABI_VERSION 12" in text
    assert "surface.hip" in build.SOURCES
    import torch  # noqa: F401  (torch's HIP runtime first, as _capi.lib() loads it)
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in declared)
    lib.mimi_hip_abi_version.restype = ctypes.c_int
    assert lib.mimi_hip_abi_version() == 12
    # a null handle: -1 points, an error status for every call that needs one
    lib.mimi_hip_surface_n_points.restype = ctypes.c_int64
    lib.mimi_hip_surface_n_points.argtypes = [ctypes.c_void_p]
    assert lib.mimi_hip_surface_n_points(None) == -1
    lib.mimi_hip_surface_add_load.argtypes = [ctypes.c_void_p] * 4
    assert lib.mimi_hip_surface_add_load(None, None, None, None) != 0


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not __import__("shutil").which("hipcc"),
                    reason="no hipcc: nothing to compile")
def test_surface_kernels_spill_no_register():
    from mimi_amd import isa_lint as L
    spills = {n: c for n, c in L.spill_counts(L.assembly("surface.hip")).items() if "surface" in n}
    # face pass (points / load) for DIM 2 / 3, the node gather
    assert len(spills) == 5, sorted(spills)
    assert all(c == 0 for c in spills.values()), spills
    # the pressure kernels keep their count beside the shared header (none of the surface kernels is named after them)
    assert not any("pressure" in n for n in spills)
    assert len({n for n in L.spill_counts(L.assembly("pressure.hip")) if "pressure" in n or "face_" in n}) == 10


def test_coupling_entries_before_setup():
    import mimi_amd
    nl = mimi_amd.NonlinearSolid()
    nl.read_mesh(os.path.join(ROOT, "tests", "golden", "meshes", "balken.mesh"))
    with pytest.raises(RuntimeError, match="setup"):
        nl.coupling_surface(0)
    with pytest.raises(KeyError):
        nl.linear_form_view2("rhs")
    with pytest.raises(KeyError):
        nl.newton_final_norms("contact")
    assert nl.newton_final_norms("nonlinear_solid") == (0.0, 0.0)
