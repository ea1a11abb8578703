"""The device status word of the domain integrator: does a kernel whose return map cannot solve its scalar equation tell the
caller -- on every kernel family, through every entry that runs a return map, under both reporting rules of
include/mimi_hip.h ("kernel-raised errors").  Cases, fields and the predicate "this point yields" (from the long-double
reference alone): tests/_status_cases.py, vetted without a GPU in tests/test_status_cases_cpu.py.  Under a softening law every
yielding point leaves ScalarSolve unbracketed, so a call must fail exactly when its field makes a point yield: quiet never,
corner_first / corner_last through ONE point (the first lane of the first workgroup, the tail of the last), many through
20 - 80 % of them.

Entries: AddDomainResidual, AddDomainResidualAndGrad (analytic, and SetTangentMode(1), which every shape serves on the general
kernels), DomainPostTimeAdvance, PointField and NodalField of cauchy_stress and von_mises_stress, Linearize.  Every assembly
asserts its kernel family.  Per entry:
  host arguments    the call itself raises RuntimeError "root not bracketed" on the three raising fields, not on quiet
  device tensors    the call returns, Synchronize() raises the same error, a second Synchronize() is clean: reported once
  afterwards        the handle works: the quiet call that follows gives the bytes of the same call on a handle that never
                    failed (for Linearize: of the ApplyTangent behind it); after a failed commit only that a quiet assembly
                    and a quiet commit do not raise (the reference leaves the state unspecified after a throw, and so do we)
No false alarms: neohook, stvk and j2linear on `many`, the hardening Voce control on every field, a handle made after a failed
one.  Element boxes of col8_p2: only the box that owns the yielding corner element raises.  Inverted geometry (one axis of the
control points mirrored): Prepare() refuses with "non-positive Jacobian" -- another bit of the same word -- and the next
handle on the device works.

Which atomicOr(p.status, ...) each family's cases pass through:
  tensor_small         rep2d_p3: tensor_small_kernel (kernels_tensor_small.hpp; residual, tangent and commit are its modes)
  tensor_p2_two_phase  col8_p2: residual tensor_residual_kernel (kernels_tensor_residual.hpp; its column kernel serves the
                       neo-Hookean law alone, which has no return map: that site cannot be reached by one), tangent and
                       commit tensor_point_kernel (kernels_tensor_wgs.hpp: the material pre-pass and its commit mode)
  tensor_p3_two_phase  col5_p3: tp3_point_kernel (tensor_p3.hip; assembly modes and the commit)
  general              mix3d_231, flat2d_p4, and every shape under SetTangentMode(1): general_material_kernel,
                       domain_general_kernel and post_time_advance_general_kernel (kernels_general.hpp)
  fields               field_tensor_kernel (the four patch shapes) and field_general_kernel (flat2d_p4, and mix3d_231, whose
                       handle is on the general path) of kernels_fields.hpp
  tangent record       apply_tensor_kernel and apply_general_kernel (kernels_apply.hpp), by the same split
Tried by hand on scratch builds with one atomicOr removed: without tensor_small_kernel's, the ten tests on rep2d_p3 fail and
the other 65 pass; without field_tensor_kernel's, the 30 tests on rep2d_p3, col8_p2 and col5_p3 (the boxes included) fail at
their first field entry and the 45 on mix3d_231, flat2d_p4 and the no-alarm cases pass.  For tp3_point_kernel the matrix of
cases argues the same: col5_p3's residual, tangent and commit entries reach the word through no other site.
The module takes 8 s."""
import numpy as np
import pytest

import _domain_cases as dc
import _status_cases as sc

pytestmark = pytest.mark.gpu

GF = dc.GRAD_FACTOR
FIELD_ENTRIES = [(kind, name) for kind in ("point", "nodal") for name in ("cauchy_stress", "von_mises_stress")]
# (entry, tangent mode); the commit comes last: it alone changes the handle's state
ENTRIES = ["residual", "residual_and_grad", "residual_and_grad_fd"] + [f"{k}:{n}" for k, n in FIELD_ENTRIES] + ["linearize", "commit"]


def make_handle(shape, material, element_box=None, patch=None):
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    a = dc.arrays(shape)
    rowptr, col, _ = dc.pattern(shape)
    pattern = CSRPattern(np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), len(col))
    if a.flat:
        G = NonlinearSolid("domain", material, pattern, tables=dict(dc.flat_tables(shape))).Prepare()
    else:
        G = NonlinearSolid("domain", material, pattern, patch=dc.product_patch(shape) if patch is None else patch,
                           quadrature_order=a.order, element_box=element_box).Prepare()
    G.dt_ = sc.DT
    assert G.path_ == (0 if a.family == "general" else 1)
    return G


def handle(shape, model, law, element_box=None):
    return make_handle(shape, sc.product_material(model, law), element_box)


def run(G, shape, entry, u, device=False):
    """one call of `entry` at the displacement u with host arrays or device tensors; returns the arrays it wrote (host copies
    are taken by the caller after a Synchronize), asserting the kernel family of an assembly"""
    a = dc.arrays(shape)
    n, nnz, dim = a.n_vdofs, len(dc.pattern(shape)[1]), a.dim
    if device:
        import torch
        dev = torch.device("cuda", 0)
        u = torch.from_numpy(np.array(u)).to(dev)
        zeros = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    else:
        zeros = lambda *s: np.zeros(s)
    if entry == "residual":
        r = zeros(n)
        try:
            G.AddDomainResidual(u, r)
        finally:
            assert G.LastKernelFamily() == a.family
        return [r]
    if entry in ("residual_and_grad", "residual_and_grad_fd"):
        fd = entry.endswith("_fd")
        r, A = zeros(n), zeros(nnz)
        G.SetTangentMode(1 if fd else 0)
        try:
            G.AddDomainResidualAndGrad(u, GF, r, A)
        finally:
            G.SetTangentMode(0)
            assert G.LastKernelFamily() == ("general" if fd else a.family)
        return [r, A]
    if entry == "commit":
        G.DomainPostTimeAdvance(u)
        return []
    if entry == "linearize":
        G.Linearize(u)
        if device:                                        # (an ApplyTangent with host arrays would read the word)
            return []
        x, y = dc.probes(shape)[0], np.zeros(n)           # the action behind the record
        G.ApplyTangent(x, y)
        return [y]
    kind, name = entry.split(":")
    ncomp = G.FieldComponents(name)
    if kind == "point":
        out = zeros(G.n_elements_, G.n_quad_, ncomp)
        G.PointField(name, u, out)
        return [out]
    s, w = zeros(a.n_nodes, ncomp), zeros(a.n_nodes)
    G.NodalField(name, u, s, w)
    return [s, w]


def as_bytes(arrays):
    return [(a if isinstance(a, np.ndarray) else a.cpu().numpy()).tobytes() for a in arrays]


def raises_in_call(G, shape, entry, u):
    with pytest.raises(RuntimeError, match=sc.MESSAGE):
        run(G, shape, entry, u)


def raises_at_synchronize(G, shape, entry, u):
    """device tensors: the call only enqueues, the word is read at Synchronize(), once"""
    run(G, shape, entry, u, device=True)
    with pytest.raises(RuntimeError, match=sc.MESSAGE):
        G.Synchronize()
    G.Synchronize()


def check_contract(shape, model, law):
    G0, G = handle(shape, model, law), handle(shape, model, law)
    quiet = sc.field(shape, "quiet")
    for entry in ENTRIES:
        base = None if entry == "commit" else as_bytes(run(G0, shape, entry, quiet))
        for name in sc.RAISING_FIELDS:
            assert sc.expected_to_raise(shape, model, law, name)
            u = sc.field(shape, name)
            for failing in (raises_in_call, raises_at_synchronize):
                failing(G, shape, entry, u)
                if entry == "commit":
                    run(G, shape, "residual", quiet)
                    run(G, shape, "commit", quiet)
                else:
                    assert as_bytes(run(G, shape, entry, quiet)) == base, (entry, name, failing.__name__)
        G.Synchronize()
    # the quiet field with device tensors leaves the word clean, and a handle made after the failures is clean
    for entry in ENTRIES:
        run(G, shape, entry, quiet, device=True)
        G.Synchronize()
    G2 = handle(shape, model, law)
    G2.Synchronize()
    assert as_bytes(run(G2, shape, "residual", quiet)) == as_bytes(run(G0, shape, "residual", quiet))


@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_a_failed_return_map_is_reported(shape, model):
    check_contract(shape, model, sc.MAIN_LAW)


@pytest.mark.parametrize("law", [l for l in sc.SOFT_LAWS if l != sc.MAIN_LAW])
@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("shape", sc.FAMILY_SHAPES)
def test_the_other_softening_laws(shape, model, law):
    check_contract(shape, model, law)


def never_raises(G, shape, fields, stateful=True):
    for entry in ENTRIES:
        if entry == "commit" and not stateful:
            continue
        for name in fields:
            u = sc.field(shape, name)
            run(G, shape, entry, u)
            run(G, shape, entry, u, device=True)
            G.Synchronize()


@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_the_hardening_control_never_raises(shape, model):
    """(the commit comes last per field list, so the fields after the first meet a committed state: still no alarm)"""
    never_raises(handle(shape, model, sc.CONTROL_LAW), shape, sc.FIELD_NAMES)


@pytest.mark.parametrize("matname", ["neohook", "stvk", "j2linear"])
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_materials_without_a_scalar_equation_never_raise(shape, matname):
    never_raises(make_handle(shape, dc.product_material(matname)), shape, ["many"], stateful=matname == "j2linear")


@pytest.mark.parametrize("model", sc.MODELS)
def test_only_the_box_that_owns_the_corner_element_raises(model):
    shape = dc.BOX_CASE
    quiet = sc.field(shape, "quiet")
    for owner, name in enumerate(("corner_first", "corner_last")):
        u = sc.field(shape, name)
        for k, box in enumerate(dc.BOXES):
            G = handle(shape, model, sc.MAIN_LAW, element_box=box)
            for entry in ("residual", "residual_and_grad", "point:von_mises_stress", "linearize", "commit"):
                if k == owner:
                    raises_in_call(G, shape, entry, u)
                    raises_at_synchronize(G, shape, entry, u)
                else:
                    run(G, shape, entry, u)
                    run(G, shape, entry, u, device=True)
                    G.Synchronize()
                run(G, shape, "residual", quiet)


@pytest.mark.parametrize("shape", ["rep2d_p3", "col8_p2", "mix3d_231"])
def test_an_inverted_geometry_is_refused_at_prepare(shape):
    import mimi_amd
    a = dc.arrays(shape)
    mirrored = np.array(a.ctrl)
    mirrored[:, 0] *= -1.0
    bad = mimi_amd.BSplinePatch(list(a.degrees), a.knots, mirrored, a.weights)
    with pytest.raises(RuntimeError, match="non-positive Jacobian"):
        make_handle(shape, sc.product_material("j2", sc.MAIN_LAW), patch=bad)
    G = handle(shape, "j2", sc.MAIN_LAW)
    G.Synchronize()
    run(G, shape, "residual_and_grad", sc.field(shape, "quiet"))
    raises_in_call(G, shape, "residual", sc.field(shape, "corner_last"))
