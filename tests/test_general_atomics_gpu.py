"""The atomics fallback of the general path (csrc/domain_dispatch.hpp, ensure_general_two_phase; the `else` branches of
csrc/kernels_general.hpp that add straight into r and A) against the long-double reference of tests/_domain_reference.py.
Cases and bars: tests/_domain_cases.py (ATOMICS_CASES, SEAM_PAIRS); the inputs are vetted in tests/test_general_atomics_cpu.py.

Two ways onto the route, both asserted after EVERY assembly (LastKernelFamily() == "general", LastGeneralRoute() == "atomics"):
  the natural trigger  long2d_p1_o3: a CSR whose longest row (1058) exceeds the row image of the gather; no variable set
  the seam             MIMI_HIP_GENERAL_NO_TWO_PHASE=1 around the create (monkeypatch), unset again before any assembly: the
                       handle keeps it.  One case per scatter site (dc.SEAM_SITES).  It sets the handle flag that a shortage of
                       memory for the element blocks sets; that trigger cannot be reached at test sizes and is covered only
                       through this flag.
test_routes_are_reported holds the assertion itself to account: handles of the same cases created without the variable report
"gather", a two-phase tensor handle "none", and a variable set after the create changes nothing.

(a) residual, tangent and state as test_domain_reference_gpu.check_assemblies: AddDomainResidual, then
    AddDomainResidualAndGrad twice in accumulate form on random r0 / A0 with grad_factor 0.37; the state first for the laws that
    have one.  The project's bars, not loosened: the atomics permute the summands of an entry, a few eps of the sum of their
    magnitudes.  No bit-equality between the two tangent calls (each is held to the reference); on long2d_p1_o3 the increment of
    every padded entry is exactly 0.0.
(b) AddDomainResidualAndGradFrom on the route (the A <- A_base copy of launch_general_dim and the staged forms of run_domain):
    A_out prefilled with NaN, A_base random, as (device, device), (host, host), (host base, device output); A_out - A_base within
    the bars, no NaN left, A_base unchanged to the bit; and A_base == A_out, the plain "+=".
(c) the reference's forward-difference tangent (SetTangentMode(1): the fifth scatter) against the oracle's restatement at the
    5e-4 of test_domain_shapes_gpu.py, residual 1e-12.
(d) element boxes on the route: mix3d_231 through two complementary boxes cut in z, each against the reference restricted to
    its parameter range, their sum against the whole, and r / A of the nodes outside a box equal to r0 / A0 to the bit.  (The
    general family accepts element boxes on this patch; nothing is refused.)
(e) what else a long row changes: AddMass / AddDiffusion refuse ("longer than the row image"); AddBodyForce, the point fields
    and ApplyTangent, which do not read the CSR, agree with the reference at their usual bars.

Mutations tried by hand on scratch builds of csrc/kernels_general.hpp / domain_dispatch.hpp (one each; 37 tests), and what failed:
  pp_tab[a * n_dof + b] -> pp_tab[b * n_dof + a] in the node-pair scatter that the vector-pipe, the 256-thread and the
  one-wave-per-element kernels share (the transposed offset clamped to the row, so that the scratch build writes inside A)
                       26 tests: test_atomics_route_against_the_reference on every case but rep3d_p3 (the matrix-instruction
                       kernel has a scatter text of its own), mix3d_322 with its three materials among them -- K v off by
                       1.6 - 1.8 of max |K v|, and on long2d_p1_o3 already the padded entries -- all eight of
                       test_from_base_on_the_atomics_route, both test_element_boxes_on_the_atomics_route,
                       test_long_row_forms_fields_and_action (its closing assembly)
  `+ j` dropped in the forward-difference scatter
                       the six test_reference_fd_tangent_on_the_atomics_route, nothing else
  the A <- A_base copy of launch_general_dim skipped
                       test_from_base_on_the_atomics_route[mix3d_231-device-device] and [long2d_p1_o3-device-device] (every
                       entry NaN); the other residences copy in run_domain and pass, as they should

Measured on the MI355X (worst per scatter site; test_report prints this table): residual relative to max |r| (and as a share
of its row bar), K v relative to max |K v|, asymmetry; the laws with a solver: state as a share of its bar
  site                       neo-Hookean                          StVK                         J2                                    J2Simo
  long row (wave / el. 2-D)  3.5e-15 (3.6e-3), 7.6e-15, 1.7e-16   2.8e-15 (2.8e-3), 9.4e-15, 1.6e-16
  wave per element 2-D       3.7e-16 (4.4e-4), 2.9e-15, 2.0e-16                                7.3e-13 (3.5e-4), 2.6e-12, state 0.009
  wave per element 3-D       1.0e-15 (1.0e-3), 2.4e-15, 1.6e-16                                1.5e-12 (2.3e-4), 5.0e-13, state 0.011
  256-thread node pairs      1.2e-15 (1.2e-3), 2.5e-15, 5.3e-16                                1.6e-11 (3.1e-3), 5.5e-9,  state 0.41
  512-thread vector pipe     9.3e-16 (9.3e-4), 2.9e-15, 6.2e-16                                3.9e-12 (3.2e-4), 6.1e-12, state 0.15   7.8e-12 (3.4e-4), 8.0e-12, state 0.086
  matrix instruction         1.2e-15 (1.3e-3), 4.8e-15, 4.1e-16   1.3e-15 (1.3e-3), 6.1e-15, 4.7e-16   2.0e-11 (8.8e-4), 9.1e-11, state 0.17
  flat tables                7.7e-16 (7.7e-4), 2.8e-15, 3.1e-16                                2.2e-12 (4.2e-4), 3.2e-12, state 0.011
  rational flat tables       2.6e-16 (3.1e-4), 2.2e-15, 3.9e-16                                1.3e-11 (1.3e-3), 5.4e-10, state 0.36
  (256-thread node pairs includes the element boxes of mix3d_231; the J2 tangent figures are the solver's root, not rounding:
  dc.J2_TANGENT_MEASURED.)  From a base array: residual <= 3.5e-3 of the row bar, K v <= 7.6e-15, asymmetry <= 5.1e-16 in
  every residence.  Forward-difference tangent: residual <= 1.6e-15, tangent <= 4.4e-5 (neo-Hookean), 9.3e-5 (J2), bar 5e-4.
  long2d_p1_o3 beside the assemblies: body force 1.5e-15, Cauchy stress 3.1e-15, von Mises 2.3e-15, det F 5.1e-16, action 3.4e-15.
The whole module takes 6 s; the slowest test, test_routes_are_reported, 1.8 s."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

import _domain_cases as dc
import _domain_reference as dr
from _domain_cases import DT, GRAD_FACTOR, f64

pytestmark = pytest.mark.gpu

WORST = {}          # (scatter site, material) -> {figure: worst}, for test_report


def note(site, matname, **fig):
    w = WORST.setdefault((site, matname), {})
    for k, v in fig.items():
        w[k] = max(w.get(k, 0.0), float(v))


def relmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max() / max(np.abs(f64(b)).max(), 1e-300))


def site_of(case):
    return "long row (wave per element 2-D)" if case == dc.LONG_CASE else dc.SEAM_SITES[case]


@contextlib.contextmanager
def environment(monkeypatch, seam):
    """the variable of the seam set to 1 (True) or to the given text, or certainly unset (False), for the statements inside"""
    with monkeypatch.context() as m:
        if seam:
            m.setenv(dc.SEAM_ENV, "1" if seam is True else seam)
        else:
            m.delenv(dc.SEAM_ENV, raising=False)
        yield


def handle(monkeypatch, case, matname, seam=None, element_box=None):
    """the product handle of a case on its atomics pattern; seam: the variable around the create only (default: set on every
    case but the long one, which needs none)"""
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    a = dc.arrays(case)
    rowptr, col, _ = dc.atomics_pattern(case)
    pattern = CSRPattern(np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), len(col))
    with environment(monkeypatch, case != dc.LONG_CASE if seam is None else seam):
        if a.flat:
            assert element_box is None
            G = NonlinearSolid("domain", dc.product_material(matname), pattern, tables=dict(dc.flat_tables(case))).Prepare()
        else:
            G = NonlinearSolid("domain", dc.product_material(matname), pattern, patch=dc.product_patch(case),
                               quadrature_order=a.order, element_box=element_box).Prepare()
    G.dt_ = DT
    assert G.LastGeneralRoute() == "none" and G.LastKernelFamily() == "none"
    return G


def on_atomics(G):
    assert G.LastKernelFamily() == "general"
    assert G.LastGeneralRoute() == "atomics"


def csr(case, values):
    rowptr, col, _ = dc.atomics_pattern(case)
    n = len(rowptr) - 1
    return sp.csr_matrix((values, col, rowptr), shape=(n, n))


def expected(ref, mask=None):
    """(residual, [K v], row bar of the residual) of the reference, restricted to the points of `mask`"""
    geo, asm = ref.geo, ref.asm
    want_r = f64(asm.r if mask is None else dr.nodal(geo, asm.pt.P, mask))
    want_Kv = [f64(k) if mask is None else f64(dr.nodal(geo, dP, mask)) for k, dP in zip(asm.Kv, asm.pt.dP)]
    return want_r, want_Kv, dc.residual_bar(ref, mask)


def tangent_figures(ref, dA, want_Kv):
    """(worst K v deviation of the increment dA over the probes, its asymmetry or None)"""
    K = csr(ref.case, dA)
    tangent = max(relmax(K @ v, GRAD_FACTOR * Kv) for v, Kv in zip(ref.vectors, want_Kv))
    symmetry = abs(K - K.T).max() / np.abs(dA).max() if ref.matname in ("neohook", "stvk") else None
    return tangent, symmetry


def check_assemblies(G, ref, label, mask=None):
    """test_domain_reference_gpu.check_assemblies on the atomics route: every call asserts family and route, each of the two
    tangent calls is held to the reference on its own, padded entries stay exactly as they were; returns the increments
    (r, A) of the last tangent call"""
    case, matname = ref.case, ref.matname
    want_r, want_Kv, bar_r = expected(ref, mask)
    padded = dc.atomics_pattern(case)[2]
    r0 = np.random.default_rng(3).standard_normal(want_r.size)
    A0 = np.random.default_rng(4).standard_normal(len(padded))
    r_g = r0.copy()
    G.AddDomainResidual(ref.u, r_g)
    on_atomics(G)
    fig = dict(residual_only=(np.abs((r_g - r0) - want_r) / bar_r).max())
    for k in range(2):
        r_g, A_g = r0.copy(), A0.copy()
        G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
        on_atomics(G)
        dr_, dA = r_g - r0, A_g - A0
        assert np.array_equal(A_g[padded], A0[padded]) and not np.any(dA[padded])
        fig["residual"] = max(fig.get("residual", 0.0), (np.abs(dr_ - want_r) / bar_r).max())
        tangent, symmetry = tangent_figures(ref, dA, want_Kv)
        fig["tangent"] = max(fig.get("tangent", 0.0), tangent)
        if symmetry is not None:
            fig["symmetry"] = max(fig.get("symmetry", 0.0), symmetry)
    print(f"{label} {matname} [{site_of(case)}]: residual-only {fig['residual_only']:.2e} and residual {fig['residual']:.2e} of the row "
          f"bar (relative {relmax(dr_, want_r):.2e}), tangent {fig['tangent']:.2e} (bar {dc.tangent_bar(matname):.2e})"
          + (f", asymmetry {fig['symmetry']:.2e}" if "symmetry" in fig else ""))
    note(site_of(case), matname, relative_residual=relmax(dr_, want_r), **fig)
    assert fig["residual_only"] <= 1.0 and fig["residual"] <= 1.0
    assert fig["tangent"] <= dc.tangent_bar(matname)
    assert fig.get("symmetry", 0.0) <= dc.SYMMETRY_BAR
    return dr_, dA


# ---- the route report itself -------------------------------------------------------------------------------------------------
def test_routes_are_reported(monkeypatch):
    """the assertion of every other test can fail: the same cases without the variable take the gather"""
    def tangent(G, ref):
        r, A = np.zeros(dc.arrays(ref.case).n_vdofs), np.zeros(len(dc.pattern(ref.case)[1]))
        G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r, A)
        return G.LastKernelFamily(), G.LastGeneralRoute()

    for case, family in (("mix3d_231", "general"), ("rep2d_p3", "tensor_small")):
        ref = dc.reference(case, "neohook")
        plain = handle(monkeypatch, case, "neohook", seam=False)
        assert tangent(plain, ref) == (family, "gather")
        seamed = handle(monkeypatch, case, "neohook")
        assert tangent(seamed, ref) == ("general", "atomics")
        # read at create and kept on the handle: setting it afterwards moves no existing handle, in either direction
        with environment(monkeypatch, True):
            assert tangent(plain, ref) == (family, "gather")
            r = np.zeros(dc.arrays(case).n_vdofs)
            plain.AddDomainResidual(ref.u, r)
            assert plain.LastGeneralRoute() == "gather"
        with environment(monkeypatch, False):
            assert tangent(seamed, ref) == ("general", "atomics")
    # a two-phase tensor family has a row gather of its own: no general route, also after the handle reported one
    ref = dc.reference("one3d_p2", "neohook")
    G = handle(monkeypatch, "one3d_p2", "neohook", seam=False)
    assert tangent(G, ref) == ("tensor_p2_two_phase", "none")
    G.SetTangentMode(1)                                     # (the reference-FD tangent runs on the general kernels)
    assert tangent(G, ref) == ("general", "gather")
    G.SetTangentMode(0)
    assert tangent(G, ref) == ("tensor_p2_two_phase", "none")
    # a value other than 1 is not the seam
    G = handle(monkeypatch, "mix3d_231", "neohook", seam="0")
    assert tangent(G, dc.reference("mix3d_231", "neohook")) == ("general", "gather")


# ---- (a) residual, tangent and committed state ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", dc.LONG_PAIRS + dc.SEAM_PAIRS, ids=lambda v: v)
def test_atomics_route_against_the_reference(case, matname, monkeypatch):
    ref = dc.reference(case, matname)
    G = handle(monkeypatch, case, matname)
    grid = dr.layout(ref.geo.sp)
    assert (G.n_elements_, G.n_quad_) == grid.shape
    if ref.mat.stateful:
        G.DomainPostTimeAdvance(ref.u0)
        note(site_of(case), matname, state=dc.compare_state(ref, G.State, grid, f"{case} {matname}"))
    check_assemblies(G, ref, case)


# ---- (b) from a base array ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["device-device", "host-host", "host base-device output", "same array"])
@pytest.mark.parametrize("case", ["mix3d_231", dc.LONG_CASE])
def test_from_base_on_the_atomics_route(case, arrangement, monkeypatch):
    import torch
    matname = "neohook"
    ref = dc.reference(case, matname)
    want_r, want_Kv, bar_r = expected(ref)
    padded = dc.atomics_pattern(case)[2]
    G = handle(monkeypatch, case, matname)
    to = lambda a, on_dev: torch.from_numpy(a.copy()).to("cuda") if on_dev else a.copy()
    back = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    r0 = np.random.default_rng(3).standard_normal(want_r.size)
    base0 = np.random.default_rng(4).standard_normal(len(padded))
    if arrangement == "same array":                 # A_base == A_out is the plain "+=", here on the host
        r, A = r0.copy(), base0.copy()
        G.AddDomainResidualAndGradFrom(np.array(ref.u), GRAD_FACTOR, r, A, A)
        base = base0
    else:
        base_dev, out_dev = {"device-device": (True, True), "host-host": (False, False), "host base-device output": (False, True)}[arrangement]
        r, A, base = to(r0, out_dev), to(np.full(len(padded), np.nan), out_dev), to(base0, base_dev)
        G.AddDomainResidualAndGradFrom(to(np.array(ref.u), out_dev), GRAD_FACTOR, r, base, A)
        G.Synchronize()
    on_atomics(G)
    r, A, base = back(r), back(A), back(base)
    assert not np.isnan(A).any()
    assert base.tobytes() == base0.tobytes()
    assert np.array_equal(A[padded], base0[padded])                       # the copy, and nothing added where nothing belongs
    residual = (np.abs((r - r0) - want_r) / bar_r).max()
    tangent, symmetry = tangent_figures(ref, A - base0, want_Kv)
    print(f"{case} from base, {arrangement}: residual {residual:.2e} of the row bar, tangent {tangent:.2e}, asymmetry {symmetry:.2e}")
    note(site_of(case), "from base", residual=residual, tangent=tangent, symmetry=symmetry)
    assert residual <= 1.0 and tangent <= dc.tangent_bar(matname) and symmetry <= dc.SYMMETRY_BAR


# ---- (c) the reference's forward-difference tangent --------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", dc.SEAM_FD_PAIRS, ids=lambda v: v)
def test_reference_fd_tangent_on_the_atomics_route(case, matname, monkeypatch):
    import _patches
    from test_domain_shapes_gpu import bspline_handle, commit_and_compare
    P, B = _patches.patches(case)
    ref = _patches.reference_fd(case, matname)
    with environment(monkeypatch, True):
        G = bspline_handle(B, ref.D, matname)
    commit_and_compare(G, ref)
    G.SetTangentMode(1)
    r0 = np.random.default_rng(3).standard_normal(P.n_vdofs)
    A0 = np.random.default_rng(4).standard_normal(ref.D.nnz)
    r_g, A_g = r0.copy(), A0.copy()
    G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
    on_atomics(G)
    e_r, e_A = relmax(r_g - r0, ref.r), relmax(A_g - A0, ref.A)
    print(f"{case} {matname} [{dc.SEAM_SITES[case]}]: FD mode residual {e_r:.2e} tangent {e_A:.2e}")
    note("forward difference", matname, residual=e_r, tangent=e_A)
    assert e_r < 1e-12
    assert e_A < 5e-4
    # and back: the analytic tangent of the same handle stays on the route
    G.SetTangentMode(0)
    r_g, A_g = r0.copy(), A0.copy()
    G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
    on_atomics(G)
    assert relmax(r_g - r0, ref.r) < 1e-12


# ---- (d) element boxes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matname", ["neohook", "j2"])
def test_element_boxes_on_the_atomics_route(matname, monkeypatch):
    case = dc.SEAM_BOX_CASE
    ref = dc.reference(case, matname)
    a, sp_ = dc.arrays(case), ref.geo.sp
    rowptr, col, _ = dc.atomics_pattern(case)
    r0 = np.random.default_rng(3).standard_normal(a.n_vdofs)
    A0 = np.random.default_rng(4).standard_normal(len(col))
    r_sum, A_sum = 0.0, 0.0
    for begin, end in dc.SEAM_BOXES:
        G = handle(monkeypatch, case, matname, element_box=(begin, end))
        grid = dr.layout(sp_, begin, end)
        assert (G.n_elements_, G.n_quad_) == grid.shape
        if ref.mat.stateful:
            G.DomainPostTimeAdvance(ref.u0)
            dc.compare_state(ref, G.State, grid, f"{case} box {begin}-{end} {matname}")
        mask = dr.in_box(sp_, begin, end)
        r, A = check_assemblies(G, ref, f"{case} box {begin}-{end}", mask=mask)     # (on the same r0 / A0 as here)
        # nodes that no point of the box sees: their rows of r and A keep r0 / A0 to the bit
        outside = np.repeat(~(np.asarray(sp_.N)[mask] != 0).any(axis=0), a.dim)
        assert 0 < outside.sum() < a.n_vdofs
        r_g, A_g = r0.copy(), A0.copy()
        G.AddDomainResidualAndGrad(ref.u, GRAD_FACTOR, r_g, A_g)
        on_atomics(G)
        entries = np.repeat(outside, np.diff(rowptr))
        assert r_g[outside].tobytes() == r0[outside].tobytes() and A_g[entries].tobytes() == A0[entries].tobytes()
        assert not np.any(r[outside]) and not np.any(A[entries])
        r_sum, A_sum = r_sum + r, A_sum + A
    want_r, want_Kv, bar_r = expected(ref)
    assert (np.abs(r_sum - want_r) / bar_r).max() <= 1.0
    assert tangent_figures(ref, A_sum, want_Kv)[0] <= dc.tangent_bar(matname)


# ---- (e) what else a long row changes ------------------------------------------------------------------------------------------
def test_long_row_forms_fields_and_action(monkeypatch):
    case, matname = dc.LONG_CASE, "neohook"
    ref = dc.reference(case, matname)
    geo, a = ref.geo, dc.arrays(case)
    G = handle(monkeypatch, case, matname)
    nnz = len(dc.atomics_pattern(case)[1])
    for form, factor in ((G.AddMass, dc.RHO), (G.AddDiffusion, dc.NU)):
        values = np.zeros(nnz)
        with pytest.raises(RuntimeError, match=r"a CSR row of 1058 entries is longer than the row image \(\d+\)"):
            form(factor, values)
        assert not values.any()
    # the routes that do not read the CSR
    f = np.zeros(a.n_vdofs)
    G.AddBodyForce(dc.B3[:a.dim], f)
    fig = dict(body=relmax(f, dr.body_force(geo, dc.B3[:a.dim])))
    grid = dr.layout(geo.sp)
    F = dr.deformation_gradient(geo, ref.u)
    J = dr.det(F)
    sigma = dr.mm(ref.asm.pt.P, dr.T(F)) / J[:, None, None]
    q = np.sqrt(dc.LD(3) / 2) * dr.frob(dr.dev(sigma))
    want = {"cauchy_stress": f64(np.swapaxes(sigma, 1, 2).reshape(len(J), -1)), "von_mises_stress": f64(q)[:, None], "det_F": f64(J)[:, None]}
    for name, w in want.items():
        got = G.PointField(name, ref.u)
        assert got.shape == grid.shape + (w.shape[1],)
        fig[name] = relmax(got, w[grid])
    G.Linearize(np.array(ref.u))
    fig["action"] = 0.0
    for v, Kv in zip(ref.vectors, ref.asm.Kv):
        y0 = np.random.default_rng(11).standard_normal(len(v))
        y = y0.copy()
        G.ApplyTangent(np.array(v), y)
        fig["action"] = max(fig["action"], relmax(y - y0, Kv))
    assert G.LastActionFamily() == "general"
    print(f"{case}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    note(site_of(case), "forms, fields, action", **fig)
    assert fig["body"] <= dc.FORMS_BAR
    assert max(fig[k] for k in want) <= 1e-11                # the bar of tests/test_fields_gpu.py
    assert fig["action"] <= dc.tangent_bar(matname)
    # and the assembly on the same handle afterwards is the atomics route as before
    check_assemblies(G, ref, f"{case} after the forms")


def test_report():
    """the worst figures of this session per scatter site and material (what the module docstring records)"""
    for (site, matname), fig in sorted(WORST.items()):
        print(f"  {site:32s} {matname:22s} " + ", ".join(f"{k} {v:.1e}" for k, v in fig.items()))
