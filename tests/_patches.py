"""Patches that are not Patch.block for the domain-integrator tests (tests/test_domain_shapes_*.py): non-uniform knots,
repeated interior knots (what subdivide followed by elevate_degrees produces), a different degree per axis -- each as the
oracle's iga.Patch and the product's BSplinePatch over the same arrays -- and the shared oracle reference of a case.

Every case names the route of csrc/domain_dispatch.hpp / tensor_dispatch.hpp it is there for (re-derive the table when
those conditions change):
  tensor_small          2-D degree 1..3 / 3-D degree 1, one degree on all axes, nq = p + 2; repeated knots allowed (the 1-D
                        tables are indexed by span, the nodes come from the connectivity)
  tensor_p2_two_phase   3-D degree 2, structured CSR, no repeated interior knot (first[e] == e)
  tensor_p3_two_phase   3-D degree 3, the same conditions
  general               everything else: repeated knots in 3-D degree 2 / 3, mixed degrees, nq != p + 2, flat tables.
                        Tangent kernel by nodes per element n and points per element: one wave per element when
                        n ceil(n / 3) <= 128, at most 64 points and the LDS of four elements fits; 512 threads when n^2 > 768
                        (matrix instruction at 3-D n = 64, vector pipe otherwise); else 256 threads."""
import functools
import types

import numpy as np

from _cases import oracle_material, synthetic_u

DT = 0.5            # time step of every assembly
GRAD_FACTOR = 0.37
COMMIT_SCALE = 0.03  # J2: synthetic_u(scale=COMMIT_SCALE, seed=7) is committed before the assemblies


def open_knots(p, inner):
    """[0] * (p + 1) + inner + [top] * (p + 1), top = max(inner) + 1 (1 for a single span)"""
    inner = [float(x) for x in inner]
    top = max(inner) + 1.0 if inner else 1.0
    return np.array([0.0] * (p + 1) + inner + [top] * (p + 1))


def uniform(m):
    """interior knots of m unit spans"""
    return [float(k) for k in range(1, m)]


def greville_patch(degrees, knots, jitter=0.04, seed=1):
    """(oracle iga.Patch, mimi_amd.BSplinePatch) over the same arrays: control points at the Greville abscissae (the identity
    map) plus jitter * N(0, 1), first parametric direction fastest"""
    import mimi_amd
    from oracle import iga
    degrees = [int(p) for p in degrees]
    knots = [np.asarray(k, dtype=np.float64) for k in knots]
    g = [iga.greville(k, p) for k, p in zip(knots, degrees)]
    grids = np.meshgrid(*g, indexing="ij")
    ctrl = np.stack([gr.ravel(order="F") for gr in grids], axis=1)
    ctrl = ctrl + jitter * np.random.default_rng(seed).standard_normal(ctrl.shape)
    return iga.Patch(degrees, knots, ctrl), mimi_amd.BSplinePatch(degrees, knots, ctrl)


# id -> (degrees, interior knots per axis, kernel family of an assembly at the default quadrature order)
CASES = {
    "rep2d_p2": ((2, 2), ([1, 2, 2, 3], [0.4, 1.1]), "tensor_small"),
    "rep2d_p3": ((3, 3), ([1, 1, 2.5], [1, 2, 2, 2]), "tensor_small"),
    "rep3d_p1": ((1, 1, 1), ([1, 2.5], [0.3], [1, 2, 3]), "tensor_small"),
    "rep3d_p2": ((2, 2, 2), ([1, 2, 2, 3], [1, 1], [0.7, 1.9]), "general"),
    "rep3d_p3": ((3, 3, 3), ([1, 1, 2], [1.3], [1, 2, 2, 2]), "general"),
    "nonuni3d_p2": ((2, 2, 2), ([0.2, 1.5, 1.7], [1, 2.9], [0.5, 1, 4]), "tensor_p2_two_phase"),
    "nonuni3d_p3": ((3, 3, 3), ([0.2, 1.5], [2.9], [0.5, 1, 4]), "tensor_p3_two_phase"),
    "mix2d_31": ((3, 1), ([1, 1, 2.5], [1, 2]), "general"),
    "mix2d_23": ((2, 3), ([1, 2], [0.5]), "general"),
    "mix3d_211": ((2, 1, 1), (uniform(2), uniform(3), uniform(2)), "general"),
    "mix3d_221": ((2, 2, 1), (uniform(2), uniform(2), uniform(3)), "general"),
    "mix3d_231": ((2, 3, 1), ([1, 2], [1], [1, 2, 3]), "general"),
    "mix3d_322": ((3, 2, 2), (uniform(2), uniform(2), uniform(2)), "general"),
    "mix3d_332": ((3, 3, 2), (uniform(2), uniform(1), uniform(2)), "general"),
}
MATERIALS = ("neohook", "j2")
# (case, material) of the residual / tangent / commit parity: every case with both, the 90-field tangent record on three
PARITY = [(c, m) for c in CASES for m in MATERIALS] + [(c, "j2simo") for c in ("rep3d_p2", "mix3d_322", "rep2d_p2")]

# (case, quadrature_order, points per element): nq = order // 2 + 1 per direction != p + 2, so every one is on the general
# kernels, uniform or not.  Orders 3 and 9: under- and over-integration, 125 points = the limit.  The last two put 12- and
# 18-node elements with 27 points on the 3-D one-wave-per-element tangent kernel (at their default 64 points the LDS of four
# elements does not fit and each element gets a workgroup).
ORDERS = [("rep2d_p2", 3, 4), ("rep2d_p2", 9, 25), ("rep3d_p2", 3, 8), ("rep3d_p2", 9, 125), ("nonuni3d_p3", 3, 8),
          ("mix3d_211", 5, 27), ("mix3d_221", 5, 27)]
# flat tables of 2-D blocks of degree 4, 5, 7: 25, 36, 64 nodes and 36, 49, 81 points per element
BLOCKS = [((2, 2), 4), ((3, 2), 5), ((2, 2), 7)]


def knots_of(case):
    degrees, inner, _ = CASES[case]
    return [open_knots(p, k) for p, k in zip(degrees, inner)]


def family_of(case):
    return CASES[case][2]


@functools.lru_cache(maxsize=None)
def patches(case):
    """(oracle patch, product patch) of a named case; shared, never modified"""
    return greville_patch(CASES[case][0], knots_of(case))


def smallest_span(P):
    return min(float(np.diff(k)[np.diff(k) > 0].min()) for k in P.knots)


def amplitudes(P, matname):
    """(scale of the committed displacement, scale of the displacement of the assemblies).  The assemblies' follow
    test_domain_gpu.py (0.05 neo-Hookean, 0.02 J2) times the smallest knot span where that is below 1, so that no element
    comes near inversion; tests/test_domain_shapes_cpu.py holds them to det F > 0 and, for J2, to a plastic share of
    10 - 90 % of the points."""
    h = min(1.0, smallest_span(P))
    return COMMIT_SCALE, (0.05 if matname == "neohook" else 0.02) * h


def inputs(P, matname):
    """(u0 of the commit, u of the assemblies)"""
    s0, s = amplitudes(P, matname)
    return synthetic_u(P, scale=s0, seed=7), synthetic_u(P, scale=s)


def assemble(P, matname, order=-1, n_threads=2, elements=None, tangent=None):
    """the oracle's integrator on P in the committed state and what it assembles from zero: residual-only r0, and r, A of
    the residual + tangent call (exact tangent unless `tangent` says otherwise) with GRAD_FACTOR and DT"""
    from oracle import ref_path as rp
    D = rp.DomainOracle(P, oracle_material(matname), quadrature_order=order, n_threads=n_threads, elements=elements)
    D.set_dt(DT)
    u0, u = inputs(P, matname)
    if D.has_states:
        D.domain_post_time_advance(u0)
    r0, r, A = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs), np.zeros(D.nnz)
    D.add_domain_residual(u, r0)
    D.add_domain_residual_and_grad(u, GRAD_FACTOR, r, A, rp.TANGENT_EXACT if tangent is None else tangent)
    for a in (u0, u, r0, r, A):
        a.setflags(write=False)
    return types.SimpleNamespace(P=P, D=D, u0=u0, u=u, r0=r0, r=r, A=A)


@functools.lru_cache(maxsize=None)
def reference(case, matname, order=-1):
    """assemble() of a named case: computed once, shared among the tests, never modified"""
    return assemble(patches(case)[0], matname, order)


@functools.lru_cache(maxsize=None)
def reference_fd(case, matname):
    """the same with the oracle's restatement of the reference's forward-difference tangent"""
    from oracle import ref_path as rp
    return assemble(patches(case)[0], matname, tangent=rp.TANGENT_FD)


@functools.lru_cache(maxsize=None)
def block_reference(n_el, p, matname):
    """assemble() of iga.Patch.block(n_el, p): the flat-table cases"""
    from oracle import iga
    return assemble(iga.Patch.block(n_el, p), matname)
