"""Coulomb friction on the matrix-free route (csrc/kernels_face_friction_action.hpp), without a GPU:
(1) include/mimi_hip.h and mimi_amd._capi carry mimi_hip_contact_set_friction_action, the library exports it, the ABI version
    is still 12, a null handle is an error; the front end carries SetFrictionAction / HoldsFrictionRecord;
(2) the new kernels use no scratch and no LDS in contact.hip;
(3) mimi_amd.solid.resolve_route: "friction_matrix_free" needs "matrix_free_boundary", is refused with "explicit_dynamics",
    lets a body with friction through "matrix_free_boundary" (which refuses it without the flag, in today's words) and may
    stand beside "contact_consistent_tangent";
(4) the reference of tests/_friction_action_reference.py is vetted: on every face of every case of tests/_friction_cases.py,
    plane and sphere, its total K v (consistent contact + friction + the new part) against the central difference of its total
    residual (contact + friction, the committed state frozen) in long double, with the step rule of
    tests/_contact_consistent_cases.py, on the scale max_i (|K| |v|)_i with |K| entrywise;
(5) the cases are a valid input of such a quotient: at both of its end points, long double and float64, every point keeps its
    branch (none / stick / slip) and its contact flag;
(6) the inputs are not void: per case at least one face has slip points with K_new v != 0;
(7) the same difference in float64 with h = 1e-6: the bar of the device's own difference quotient.

Measured here (x86-64, 80-bit long double): (4) worst 1.07e-10 on mix3d_211 / plane (sphere 9.7e-11), nonuni3d_p3 / sphere
4.3e-11, every other face below 1e-11 (_friction_action_cases.LD_WORST; the bar is 10 x it); (7) 2.32e-10 on rep3d_p2 / sphere,
2.27e-10 on rep2d_p3 / plane, 1.2e-10 and 1.5e-10 on the other two (_friction_action_cases.F64_WORST = 2.4e-10)."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import _face_cases as fc
import _friction_action_cases as fa
from test_boundary_action_cpu import vectors

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mimi_hip_contact_set_friction_action"
HAVE_HIPCC = os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
def test_header_and_capi_carry_the_entry():
    from mimi_amd import _capi
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        text = f.read()
    assert re.search(r"^int " + ENTRY + r"\(mimi_hip_contact_t h, int on\);$", text, flags=re.M)
    before = text[:text.index("int " + ENTRY)]
    comment = before[before.rindex("/*"):]
    assert "COMMITTED" in comment and "snapshot" in comment and "no launch" in comment and "reference-FD" in comment
    assert "n_faces n_quad (8 (dim + 1) + 1) + 8" in comment
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
    assert info(None, 3) == -1


def test_python_front_end_carries_the_methods():
    from mimi_amd.integrators import MortarContact
    assert callable(MortarContact.SetFrictionAction) and callable(MortarContact.HoldsFrictionRecord)
    assert "COMMITTED" in MortarContact.SetFrictionAction.__doc__ and "ShardedContact" in MortarContact.SetFrictionAction.__doc__


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc: nothing to compile")
def test_friction_action_kernels_use_no_scratch_and_no_lds():
    from mimi_amd import isa_lint as L
    asm = L.assembly("contact.hip")
    new = {n: c for n, c in L.spill_counts(asm).items() if "contact_friction_action_kernel" in n or "contact_friction_record_kernel" in n}
    # the action for DIM 2 / 3, frozen / consistent, and the record for DIM 2 / 3
    assert len(new) == 6, sorted(new)
    assert all(c == 0 for c in new.values()), new
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, flags=re.S)
    seen = 0
    for name, body in blocks:
        if name in new:
            seen += 1
            assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", body), name
            assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\b", body), name
    assert seen == 6
    assert not any("contact_friction_" in n for n in L.spill_counts(L.assembly("pressure.hip")))


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
def test_route_rules():
    from mimi_amd import solid
    from mimi_amd.integrators import RigidPlane
    from test_nonlinear_solid import beam

    def resolve(flags, mu=None):
        nl = beam("neohook", runtime=[(f, 1) for f in flags], finish=False)
        if mu is not None:
            nl.boundary_condition.current.contact(0, RigidPlane([0.0, 0.0], [0.0, 1.0], friction=mu))
        return solid.resolve_route(nl.runtime_communication, nl.boundary_condition, [])

    solver = ("use_iterative_solver", "use_kronecker_preconditioner")
    free = solver + ("matrix_free", "matrix_free_boundary")
    for flags in (("friction_matrix_free",), solver + ("friction_matrix_free",), solver + ("matrix_free", "friction_matrix_free")):
        with pytest.raises(RuntimeError, match="friction_matrix_free needs matrix_free_boundary"):
            resolve(flags)
    with pytest.raises(RuntimeError, match="friction_matrix_free cannot be combined with explicit_dynamics"):
        resolve(("explicit_dynamics", "friction_matrix_free"))
    # a rough body: refused without the flag in today's words, accepted with it, with and without the consistent tangent
    for flags in (free, free + ("contact_consistent_tangent",)):
        with pytest.raises(RuntimeError, match=r"matrix_free_boundary cannot be combined with a contact body with friction \(mu = "
                                                 r"0\.3\): the friction tangent has no matrix-free action"):
            resolve(flags, mu=0.3)
    route = resolve(free + ("friction_matrix_free",), mu=0.3)
    assert route.friction_actions and route.boundary_actions and route.matrix_free and not route.consistent_contact
    route = resolve(free + ("friction_matrix_free", "contact_consistent_tangent"), mu=0.3)
    assert route.friction_actions and route.consistent_contact
    # a smooth body is untouched by the flag, and the flag is off by default
    assert resolve(free + ("friction_matrix_free",), mu=0.0).friction_actions
    assert not resolve(free, mu=0.0).friction_actions and not resolve(free).friction_actions
    assert not solid.Route().friction_actions
    # the assembled route takes a rough body as before
    assert not resolve((), mu=0.3).friction_actions


# ---- (4) - (7) ---------------------------------------------------------------------------------------------------------------
def central_difference(case, axis, side, order, kind, v, h, dtype, keep):
    """(r(x + h v) - r(x - h v)) / 2 h of the reference's total residual; asserts that both end points keep `keep` = (branch,
    contact flag) of every point"""
    x = fa.configuration(case)
    if dtype is np.float64:                      # the inputs a double-precision evaluation sees
        plus = (x.astype(np.float64) + np.float64(h) * v.reshape(x.shape)).astype(LD)
        minus = (x.astype(np.float64) - np.float64(h) * v.reshape(x.shape)).astype(LD)
    else:
        step = (LD(h) * v.astype(LD)).reshape(x.shape)
        plus, minus = x + step, x - step
    rp, bp, cp = fa.residual(case, axis, side, order, kind, plus, dtype)
    rm, bm, cm = fa.residual(case, axis, side, order, kind, minus, dtype)
    for b, c in ((bp, cp), (bm, cm)):
        assert np.array_equal(b, keep[0]), "a point changes its branch inside the quotient"
        assert np.array_equal(c, keep[1]), "a point changes its contact flag inside the quotient"
    return (rp - rm) / dtype(2 * h)


@pytest.mark.parametrize("kind", fa.KINDS)
@pytest.mark.parametrize("case,order", fa.CASES, ids=lambda c: str(c))
def test_reference_against_the_central_difference_of_the_total_residual(case, order, kind):
    worst_ld, worst_64, slip_new = 0.0, 0.0, False
    for axis, side in fc.faces(case):
        P = fa.products(case, axis, side, order, kind)
        assert P.g_min > 0
        # (at u1 itself the residual takes the branches of the products)
        _, b, c = fa.residual(case, axis, side, order, kind, fa.configuration(case))
        assert np.array_equal(b, P.branch) and np.array_equal(c, P.inside)
        keep = (P.branch, P.inside)
        for k, v in enumerate(vectors(case, axis, side)):
            assert np.isfinite(P.Kv[k]).all() and P.scale[k].max() > 0
            # (6) the new part is there on this face?
            slip_new = slip_new or (bool(np.any(P.branch == 2)) and np.abs(P.new[k]).max() > 0)
            # (4) long double, a step that moves no point across g = 0
            h = min(1e-6, 1e-3 * P.g_min / np.abs(v).max())
            fd = central_difference(case, axis, side, order, kind, v, h, LD, keep) * LD(fc.GRAD_FACTOR)
            worst_ld = max(worst_ld, float(np.abs(fd - P.Kv_ld[k]).max() / P.scale_ld[k].max()))
            # (7) float64, h = 1e-6, where the device's quotient is taken
            if case in fa.FD_CASES and order == -1:
                assert fa.FD_STEP * np.abs(v).max() * np.sqrt(fc.product_patch(case).dim) < P.g_min, "a point may change side"
                fd = central_difference(case, axis, side, order, kind, v, fa.FD_STEP, np.float64, keep) * fc.GRAD_FACTOR
                worst_64 = max(worst_64, float(np.abs(fd - P.Kv[k]).max() / P.scale[k].max()))
    print(f"figures friction action reference {case} order {order} {kind}: long double {worst_ld:.2e} (bar {10 * fa.LD_WORST:.2e})"
          + (f", float64 h=1e-6 {worst_64:.2e} (recorded {fa.F64_WORST:.2e})" if worst_64 else ""))
    assert slip_new, "no face of the case has slip points with K_new v != 0"
    assert worst_ld <= 10 * fa.LD_WORST
    assert worst_64 <= fa.F64_WORST
