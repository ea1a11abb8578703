"""The C ABI of the mass, damping and body-force forms without a device: declarations, exports, the unchanged ABI version,
the loud failure, and the product's independence of the oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mimi_hip_domain_add_mass", "mimi_hip_domain_add_diffusion", "mimi_hip_domain_add_body_force")


def test_header_declares_and_capi_exports_the_entries():
    from mimi_amd import _capi
    header = open(os.path.join(ROOT, "include", "mimi_hip.h")).read()
    L = _capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*mimi_hip_domain_t\b" % name, header), name
        assert name in _capi.EXPORTS
        assert getattr(L, name).argtypes is not None


def test_abi_version_is_still_12():
    from mimi_amd import _capi
    assert _capi._header_abi_version() == 12
    assert _capi.lib().mimi_hip_abi_version() == 12


def test_no_cpu_fallback_without_a_device():
    import mimi_amd
    from mimi_amd import _capi
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    L = _capi.lib()
    if L.mimi_hip_device_count() > 0:
        pytest.skip("a HIP device is visible")
    patch = mimi_amd.BSplinePatch.block((2, 2), 2)
    mat = mimi_amd.CompressibleOgdenNeoHookean()
    mat.set_young_poisson(2100, 0.3)
    pat = CSRPattern(np.zeros(patch.n_vdofs + 1, dtype=np.int64), np.zeros(1, dtype=np.int32), 0)
    G = NonlinearSolid("domain", mat, pat, patch=patch)
    calls = {"mimi_hip_domain_add_mass": lambda g: g.AddMass(1.0, np.zeros(1)),
             "mimi_hip_domain_add_diffusion": lambda g: g.AddDiffusion(1.0, np.zeros(1)),
             "mimi_hip_domain_add_body_force": lambda g: g.AddBodyForce([0.0, 1.0], np.zeros(patch.n_vdofs))}
    for name in ENTRIES:
        # no handle can exist: creating one says why, and the entry itself refuses the handle it was not given
        with pytest.raises(RuntimeError, match="no HIP device"):
            calls[name](G.Prepare())
        with pytest.raises(RuntimeError, match="Prepare"):
            calls[name](G)


def test_product_does_not_import_the_oracle():
    code = ("import sys; sys.path.insert(0, %r); import mimi_amd, mimi_amd.integrators, mimi_amd.solid, mimi_amd.linear; "
            "assert not [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')], 'oracle imported'" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
    for name in ("solid.py", "integrators.py", "_capi.py"):
        assert not re.search(r"^\s*(from|import)\s+oracle\b", open(os.path.join(ROOT, "mimi_amd", name)).read(), re.M)
