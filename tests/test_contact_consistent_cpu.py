"""The consistent mortar-contact tangent as a matrix-free action (csrc/kernels_face_consistent.hpp), without a GPU:
(1) include/mimi_hip.h and mimi_amd._capi carry mimi_hip_contact_set_consistent_tangent, the library exports it, the ABI
    version is still 12, a null handle is an error;
(2) the new kernels spill no register in contact.hip, and none of them carries the names the frozen action's kernels are
    counted by (tests/test_boundary_action_cpu.py);
(3) mimi_amd.solid.resolve_route: "contact_consistent_tangent" needs "matrix_free_boundary" (the message says why), is
    refused with "explicit_dynamics", and resolves beside the matrix-free flags;
(4) the reference of tests/_contact_consistent_reference.py is vetted: on every face of every case, plane and sphere, its K v
    against the central difference of tests/_face_reference.py's residual in long double with a step at which no point can
    change side (g is 1-Lipschitz), on the scale max_i (K_abs |v|)_i;
(5) the inputs are not void: the new part's K_new v is not zero on any face;
(6) the same difference in float64 with h = 1e-6: the bar of the device's own difference quotient.

Measured here (x86-64, 80-bit long double): (4) worst 1.27e-11 on mix2d_23 / plane, most faces near 1e-12
(_contact_consistent_cases.LD_WORST; the bar is 10 x it); (6) worst 9.42e-11 on rep3d_p2 / plane, 4.7e-11 to 8.0e-11 on the other
three (_contact_consistent_cases.F64_WORST = 9.5e-11)."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import _contact_consistent_cases as cc
import _face_cases as fc
from test_boundary_action_cpu import vectors

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mimi_hip_contact_set_consistent_tangent"
HAVE_HIPCC = os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
def test_header_and_capi_carry_the_entry():
    from mimi_amd import _capi
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        text = f.read()
    assert re.search(r"^int " + ENTRY + r"\(mimi_hip_contact_t h, int on\);$", text, flags=re.M)
    before = text[:text.index("int " + ENTRY)]
    comment = before[before.rindex("/*"):]
    assert "mortar_contact.cpp:281-294" in comment and "friction" in comment and "next linearize" in comment
    assert re.search(r"^#define MIMI_HIP_ABI_VERSION 12$", text, flags=re.M)
    assert ENTRY in _capi.EXPORTS


def test_library_exports_the_entry_and_a_null_handle_is_an_error():
    from mimi_amd import build
    path = build.build()
    import torch  # noqa: F401  (ahead of the library, as _capi.lib() loads it)
    lib = ctypes.CDLL(path)
    lib.mimi_hip_abi_version.restype = ctypes.c_int
    assert lib.mimi_hip_abi_version() == 12
    lib.mimi_hip_last_error.restype = ctypes.c_char_p
    fn = getattr(lib, ENTRY)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert fn(None, 1) != 0 and b"null" in lib.mimi_hip_last_error()
    info = lib.mimi_hip_contact_action_info
    info.argtypes, info.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int64
    assert info(None, 2) == -1


def test_python_front_end_carries_the_methods():
    from mimi_amd.integrators import MortarContact
    assert callable(MortarContact.SetConsistentTangent) and callable(MortarContact.HoldsConsistentRecord)
    assert "own faces" in MortarContact.SetConsistentTangent.__doc__


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc: nothing to compile")
def test_consistent_kernels_spill_no_register():
    from mimi_amd import isa_lint as L
    counts = L.spill_counts(L.assembly("contact.hip"))
    new = {n: c for n, c in counts.items() if "contact_consistent_" in n}
    # record, rates and action for DIM 2 / 3, and the nodal kernel
    assert len(new) == 7, sorted(new)
    assert all(c == 0 for c in new.values()), new
    assert not any("boundary_action_kernel" in n or "boundary_linearize_kernel" in n for n in new)
    assert not any("contact_consistent_" in n for n in L.spill_counts(L.assembly("pressure.hip")))


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
def test_route_rules():
    from mimi_amd import solid
    from test_nonlinear_solid import beam

    def resolve(flags):
        nl = beam("neohook", runtime=[(f, 1) for f in flags], finish=False)
        return solid.resolve_route(nl.runtime_communication, nl.boundary_condition, [])

    solver = ("use_iterative_solver", "use_kronecker_preconditioner")
    for flags in (("contact_consistent_tangent",), solver + ("contact_consistent_tangent",),
                  solver + ("matrix_free", "contact_consistent_tangent")):
        with pytest.raises(RuntimeError, match="contact_consistent_tangent needs matrix_free_boundary.*leaves the CSR pattern"):
            resolve(flags)
    with pytest.raises(RuntimeError, match="contact_consistent_tangent cannot be combined with explicit_dynamics"):
        resolve(("explicit_dynamics", "contact_consistent_tangent"))
    route = resolve(solver + ("matrix_free", "matrix_free_boundary", "contact_consistent_tangent"))
    assert route.consistent_contact and route.boundary_actions and route.matrix_free
    route = resolve(solver + ("matrix_free", "matrix_free_boundary"))
    assert not route.consistent_contact and route.boundary_actions
    assert not solid.Route().consistent_contact


# ---- (4) - (6) ---------------------------------------------------------------------------------------------------------------
def central_difference(case, axis, side, order, kind, v, h, dtype):
    x = cc.configuration(case)
    step = (LD(h) * v.astype(LD)).reshape(x.shape)
    if dtype is np.float64:                      # the inputs a double-precision evaluation sees
        plus = (x.astype(np.float64) + np.float64(h) * v.reshape(x.shape)).astype(LD)
        minus = (x.astype(np.float64) - np.float64(h) * v.reshape(x.shape)).astype(LD)
    else:
        plus, minus = x + step, x - step
    rp = cc.residual(case, axis, side, order, kind, plus, dtype)
    rm = cc.residual(case, axis, side, order, kind, minus, dtype)
    return (rp - rm) / dtype(2 * h)


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("case,order", cc.ALL, ids=lambda c: str(c))
def test_reference_against_the_central_difference_of_the_residual(case, order, kind):
    worst_ld, worst_64 = 0.0, 0.0
    for axis, side in fc.faces(case):
        P = cc.products(case, axis, side, order, kind)
        assert P.g_min > 0
        for k, v in enumerate(vectors(case, axis, side)):
            # (5) the new part is there
            assert np.isfinite(P.Kv[k]).all() and np.abs(P.new[k]).max() > 0 and P.scale[k].max() > 0
            # (4) long double, a step that moves no point across g = 0
            h = min(1e-6, 1e-3 * P.g_min / np.abs(v).max())
            fd = central_difference(case, axis, side, order, kind, v, h, LD) * LD(fc.GRAD_FACTOR)
            worst_ld = max(worst_ld, float(np.abs(fd - P.Kv_ld[k]).max() / P.scale_ld[k].max()))
            # (6) float64, h = 1e-6, where the device's quotient is taken
            if case in cc.FD_CASES and order == -1:
                assert cc.FD_STEP * np.abs(v).max() * np.sqrt(fc.product_patch(case).dim) < P.g_min, "a point may change side"
                fd = central_difference(case, axis, side, order, kind, v, cc.FD_STEP, np.float64) * fc.GRAD_FACTOR
                worst_64 = max(worst_64, float(np.abs(fd - P.Kv[k]).max() / P.scale[k].max()))
    print(f"figures consistent reference {case} order {order} {kind}: long double {worst_ld:.2e} (bar {10 * cc.LD_WORST:.2e})"
          + (f", float64 h=1e-6 {worst_64:.2e} (recorded {cc.F64_WORST:.2e})" if worst_64 else ""))
    assert worst_ld <= 10 * cc.LD_WORST
    assert worst_64 <= cc.F64_WORST
