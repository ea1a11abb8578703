"""Shapes, inputs and bars of tests/test_domain_reference_{cpu,gpu}.py: the domain integrator against the long-double
reference of tests/_domain_reference.py.  Every case is plain arrays (degrees, knots, control points, weights, order); the
oracle's iga.Patch and the product's BSplinePatch are made from the same arrays.

Cases, the smallest shapes at which each route of csrc/domain_dispatch.hpp / tensor_dispatch.hpp can still go wrong (none
above 3100 points); the family is asserted after every call:
  tensor_small         rep2d_p2, rep2d_p3, rep3d_p1 of tests/_patches.py; one element of degree 1 in 2-D
  tensor_p2_two_phase  nonuni3d_p2; one element; col8_p2, a jittered Greville patch of 2 x 2 x 8 uniform spans whose columns
                       launch_tensor_wgsym cuts into two segments of four (kernels_tensor_wgsym.hpp:298: 8 % 2 == 0 and
                       8 / 2 >= 4, 8 / 4 < 4); the same patch through element boxes [0, 3) and [3, 8) that cut the columns
                       (lengths 3 and 5: not split).  Neo-Hookean takes the symmetric-half kernel, every other law the
                       nine-block kernel behind the material pre-pass, the residual-only call the column kernel.
  tensor_p3_two_phase  nonuni3d_p3; one element; col5_p3, a jittered 2 x 1 x 5 patch: a column of 5 next to those of 1 and 4
                       (the stand-in stores of element 0, the clamped prefetch of the last element, both tile parities)
  general              rep3d_p2, rep3d_p3, mix2d_31, mix3d_231, mix3d_322; orders (rep3d_p2, 3) and (mix3d_221, 5); one
                       flat-table 2-D block of degree 4
  rational             tensor-product weights on a 3-D degree-2 patch (tensor route); weights that do not factorise through
                       flat tables (general route) -- the patches of test_domain_gpu.py::test_tensor_product_nurbs_weights
                       and ::test_rational_weights_general_path
  walks                WALK_CASES, apart from the above and neo-Hookean only: the multi-unit walks of the symmetric-half degree-2
                       kernel (tests/test_wgsym_walk_gpu.py), described where they are defined
  atomics              ATOMICS_CASES and SEAM_PAIRS, apart from the above: the atomics fallback of the general path
                       (tests/test_general_atomics_gpu.py), described where they are defined
Flat tables (dofs, dN/dX, w det) are the reference's own, rounded to double; CSR patterns are the union of the element blocks
found from the reference's values.

Materials: neohook, stvk, j2 (the default law, _cases.JC_TEST) on every case; j2[PowerLaw], j2[JohnsonCookRate] (the rate
term active at DT = 0.5) and j2linear on one case per family (EXTRA).  The finite-strain laws (FINITE_PAIRS) on the four cases
of EXTRA and nurbs_tp_p2: j2log and j2simo with the default law (under which j2simo heats); j2log[PowerLaw] and
j2simo[PowerLaw] on col8_p2 and col5_p3 (a law whose tangent figure is sharp); j2log[elastic] and j2simo[elastic] --
_finite_strain_inputs.ELASTIC_LAW at ELASTIC_FACTOR of the displacements, so that no point yields and nothing carries a solver
tolerance while the lanes still diverge in the eigen-solver (j2simo still commits F_old = F and be_old = be).

Inputs: displacements as _patches.inputs (u0 = synthetic_u(scale 0.03, seed) committed first for the stateful laws, the
assemblies at u = synthetic_u(scale 0.02 h | 0.05 h, seed)), the seeds of the stateful laws chosen per case (SEEDS) by
scanning on the reference until the conditions of `conditions` hold -- they are conditions on the inputs, asserted in
tests/test_domain_reference_cpu.py, never relaxed.  The finite-strain laws find seeds at the same scales.  SECOND_PAIRS go
on to a second commit at u and an assembly at a third field u2 (the scale of u, a third seed)."""
import functools
import types

import numpy as np

import _domain_reference as dr
import _face_reference as fr
import _finite_strain_inputs as fi
import _patches
import _radial_return as rr
from _cases import synthetic_u

LD = np.longdouble
DT = _patches.DT
GRAD_FACTOR = _patches.GRAD_FACTOR
RHO, NU, B3 = 1.7, 0.3, np.array([0.4, -9.81, 2.5])     # the linear forms, as tests/test_linear_forms_gpu.py

# bars (relative max-norm unless said otherwise)
RESIDUAL_BAR, TANGENT_BAR, FORMS_BAR, SYMMETRY_BAR = 1e-12, 1e-11, 1e-13, 1e-12
TANGENT_CAP = 1e-8                                      # the cap of the measured tangent bars
MARGIN = 0.125                                          # the oracle sits this far inside the bars (tests/test_faces_cpu.py)
STATE_BAR = 2.0 * rr.SOLVER_XTOL                        # |delta - delta_exact| of a solver that stops at |d delta| < 1e-10


def _greville(knots, p):
    return np.array([knots[i + 1:i + p + 1].mean() for i in range(len(knots) - p - 1)])


def _jittered(degrees, knots, jitter, seed):
    """control points of _patches.greville_patch from the arrays alone"""
    g = [_greville(np.asarray(k, dtype=np.float64), p) for k, p in zip(knots, degrees)]
    ctrl = np.stack([gr.ravel(order="F") for gr in np.meshgrid(*g, indexing="ij")], axis=1)
    return ctrl + jitter * np.random.default_rng(seed).standard_normal(ctrl.shape)


def _uniform_case(degrees, spans, family, **kw):
    return dict(degrees=degrees, inner=tuple(_patches.uniform(m) for m in spans), family=family, **kw)


def _named(case, **kw):
    degrees, inner, family = _patches.CASES[case]
    return dict(degrees=degrees, inner=inner, family=kw.pop("family", family), **kw)


CASES = {
    "rep2d_p2": _named("rep2d_p2"), "rep2d_p3": _named("rep2d_p3"), "rep3d_p1": _named("rep3d_p1"),
    "one2d_p1": _uniform_case((1, 1), (1, 1), "tensor_small"),
    "nonuni3d_p2": _named("nonuni3d_p2"),
    "one3d_p2": _uniform_case((2, 2, 2), (1, 1, 1), "tensor_p2_two_phase"),
    "col8_p2": _uniform_case((2, 2, 2), (2, 2, 8), "tensor_p2_two_phase"),
    "nonuni3d_p3": _named("nonuni3d_p3"),
    "one3d_p3": _uniform_case((3, 3, 3), (1, 1, 1), "tensor_p3_two_phase"),
    "col5_p3": _uniform_case((3, 3, 3), (2, 1, 5), "tensor_p3_two_phase"),
    "rep3d_p2": _named("rep3d_p2"), "rep3d_p3": _named("rep3d_p3"), "mix2d_31": _named("mix2d_31"),
    "mix3d_231": _named("mix3d_231"), "mix3d_322": _named("mix3d_322"),
    "rep3d_p2_o3": _named("rep3d_p2", order=3), "mix3d_221_o5": _named("mix3d_221", order=5),
    "flat2d_p4": _uniform_case((4, 4), (2, 2), "general", flat=True),
    "nurbs_tp_p2": _uniform_case((2, 2, 2), (4, 3, 3), "tensor_p2_two_phase", weights="tensor", jitter=0.05, seed=5),
    "nurbs_flat_p2": _uniform_case((2, 2, 2), (4, 3, 3), "general", weights="general", jitter=0.05, seed=21, flat=True),
}
# The walks of the symmetric-half degree-2 kernel (tests/test_wgsym_walk_gpu.py: a workgroup that walks several units back to
# back, reached at these sizes through MIMI_HIP_WGSYM_MIN_WGS), neo-Hookean only and apart from CASES, so that the material
# matrix above does not grow.  Jittered Greville control points as everywhere:
#   walk335_p2   3 x 3 x 5, non-uniform inner knots on all three axes: nine columns with nine different pairs of x / y tables
#                (a walk that kept the previous column's tables or spans is wrong in every column); columns of 5 carry the
#                rider's second value over two steps
#   walk761_p2   7 x 6 x 1: 42 units of one element, every step a unit end
#   walk542_p2   5 x 4 x 2 with tensor-product weights (those of nurbs_tp_p2): units of two elements, the one-step carry only
# and col8_p2 above (4 columns x 2 segments: a workgroup then walks segments of one column back to back).
WALK_CASES = {
    "walk335_p2": dict(degrees=(2, 2, 2), inner=([0.7, 1.9], [0.9, 2.6], [0.6, 1.5, 2.7, 3.4]), family="tensor_p2_two_phase",
                       jitter=0.03, seed=3),
    "walk761_p2": _uniform_case((2, 2, 2), (7, 6, 1), "tensor_p2_two_phase", seed=4),
    "walk542_p2": _uniform_case((2, 2, 2), (5, 4, 2), "tensor_p2_two_phase", weights="tensor", jitter=0.05, seed=6),
}
WALK_MATERIAL = "neohook"
WALK_PAIRS = [(c, WALK_MATERIAL) for c in WALK_CASES]
# (case, element shape, seg_len, [(value of MIMI_HIP_WGSYM_MIN_WGS, cols_per_wg, units of the last workgroup)]); seg_len is the
# column length except on col8_p2, whose columns of 8 the launcher cuts into two segments of 4
WALKS = [
    ("walk335_p2", (3, 3, 5), 5, [(4, 2, 1), (3, 3, 3), (2, 4, 1)]),
    ("walk761_p2", (7, 6, 1), 1, [(21, 2, 2), (14, 3, 3), (10, 4, 2)]),
    ("walk542_p2", (5, 4, 2), 2, [(5, 4, 4), (6, 3, 2)]),
    ("col8_p2", (2, 2, 8), 4, [(2, 4, 4), (4, 2, 2)]),
]
# walk335_p2 through two complementary element boxes cut in x (the second one's box_begin[0] != 0 feeds the span arithmetic of
# the walk) with MIMI_HIP_WGSYM_MIN_WGS = 1: (box, cols_per_wg): 3 units in one workgroup; 6 units, 4 and a tail of 2
WALK_BOXES = [(([0, 0, 0], [1, 3, 5]), 3), (([1, 0, 0], [3, 3, 5]), 4)]
WALK_BOX_CASE = "walk335_p2"

# The atomics fallback of the general path (tests/test_general_atomics_{cpu,gpu}.py; csrc/domain_dispatch.hpp,
# ensure_general_two_phase), apart from CASES so that PAIRS does not grow.
#   long2d_p1_o3   the natural trigger: 22 x 22 bilinear elements at quadrature order 3 (4 points per element, 1936 points;
#                  23^2 nodes x 2 = 1058 dofs) with the CSR of `atomics_pattern`: the support pattern made a superset in which
#                  the two rows of the interior node LONG_NODE hold every column 0 .. 1057, longer than the row image of the
#                  general gather (GG_MAX_ROW = 1056, csrc/kernels_general.hpp).  No environment variable is set.
#   SEAM_PAIRS     cases of CASES (their references are the session's) whose handles are created under
#                  MIMI_HIP_GENERAL_NO_TWO_PHASE=1, one per scatter site of csrc/kernels_general.hpp:
#                    rep2d_p3, rep3d_p1   launch_tensor_small hands over -> one wave per element, 2-D 16 nodes / 3-D 8 nodes
#                    mix3d_231            256-thread node-pair kernel, 24 nodes
#                    mix3d_322            512-thread vector-pipe kernel, 36 nodes (j2simo: the material pre-pass in front of it)
#                    rep3d_p3             matrix-instruction kernel, 64 nodes
#                    flat2d_p4            flat tables, 25 nodes;  nurbs_flat_p2: rational weights through flat tables
ATOMICS_CASES = {"long2d_p1_o3": _uniform_case((1, 1), (22, 22), "general", order=3)}
LONG_CASE = "long2d_p1_o3"
LONG_NODE = (11, 11)                       # grid position of the node whose rows are full
LONG_MATERIALS = ("neohook", "stvk")       # stateless laws: no seed scan
LONG_PAIRS = [(LONG_CASE, m) for m in LONG_MATERIALS]
SEAM_SITES = {"rep2d_p3": "wave per element 2-D", "rep3d_p1": "wave per element 3-D", "mix3d_231": "256-thread node pairs",
              "mix3d_322": "512-thread vector pipe", "rep3d_p3": "matrix instruction", "flat2d_p4": "flat tables",
              "nurbs_flat_p2": "rational flat tables"}
SEAM_PAIRS = ([(c, m) for c in SEAM_SITES for m in ("neohook", "j2")] + [("mix3d_322", "j2simo"), ("rep3d_p3", "stvk")])
SEAM_FD_PAIRS = [(c, m) for c in ("rep2d_p3", "mix3d_231", "rep3d_p3") for m in ("neohook", "j2")]
SEAM_BOX_CASE = "mix3d_231"                # 3 x 2 x 4 spans, two complementary boxes cut in the third direction
SEAM_BOXES = [([0, 0, 0], [3, 2, 1]), ([0, 0, 1], [3, 2, 4])]
SEAM_ENV = "MIMI_HIP_GENERAL_NO_TWO_PHASE"

# the element boxes of col8_p2: complementary, cutting every column
BOXES = [([0, 0, 0], [2, 2, 3]), ([0, 0, 3], [2, 2, 8])]
BOX_CASE = "col8_p2"
BASE_MATERIALS = ("neohook", "stvk", "j2")
EXTRA_MATERIALS = ("j2[PowerLaw]", "j2[JohnsonCookRate]", "j2linear")
EXTRA = {"tensor_small": "rep2d_p3", "tensor_p2_two_phase": "col8_p2", "tensor_p3_two_phase": "col5_p3", "general": "mix3d_231"}
FINITE_MODELS = ("j2log", "j2simo")
FINITE_CASES = list(EXTRA.values()) + ["nurbs_tp_p2"]
FINITE_SHARP_CASES = ["col8_p2", "col5_p3"]
FINITE_PAIRS = ([(c, m) for c in FINITE_CASES for m in FINITE_MODELS]
                + [(c, f"{m}[PowerLaw]") for c in FINITE_SHARP_CASES for m in FINITE_MODELS]
                + [(c, f"{m}[elastic]") for c in FINITE_CASES for m in FINITE_MODELS])
PAIRS = ([(c, m) for c in CASES for m in BASE_MATERIALS] + [(c, m) for c in EXTRA.values() for m in EXTRA_MATERIALS]
         + FINITE_PAIRS)
# A second step on two cases (SECOND_PAIRS): commit at u0 and assemble at u as everywhere, then commit at u, compare the state
# again, and assemble at a third field u2 (a third seed, the scale of u) from that state.  After one step from the identity
# j2log's Fp_inv = exp(-d N_p) is symmetric; only a second, non-coaxial step makes it non-symmetric (`conditions` asserts it).
SECOND_CASES = ["rep2d_p3", "col5_p3"]
SECOND_PAIRS = [(c, m) for c in SECOND_CASES for m in FINITE_MODELS]
# the displacements of the [elastic] variants: this share of the others' (the largest trial margin of the ten pairs is then
# below -0.3 sigma_y; `conditions` asserts that no point yields)
ELASTIC_FACTOR = 0.1
# the linear forms: one case per family and both rational cases
FORMS_CASES = ["rep2d_p2", "nonuni3d_p2", "col5_p3", "mix3d_231", "nurbs_tp_p2", "nurbs_flat_p2"]

# (case, material) -> (seed of u0, seed of u): what the scan `scan_seeds` finds first (the seed of u0 from 7 upwards until the
# commit satisfies `conditions`, then the seed of u from 20241008 upwards); pairs not listed use _patches' own (7, 20241008)
SEEDS = {
    ("one2d_p1", "j2"): (7, 20241009),   # plastic 0.44 / 0.11
    ("nonuni3d_p2", "j2"): (13, 20241008),   # plastic 0.86 / 0.15
    ("col8_p2", "j2"): (8, 20241009),   # plastic 0.70 / 0.17
    ("nonuni3d_p3", "j2"): (34, 20241008),   # plastic 0.69 / 0.14
    ("col5_p3", "j2"): (10, 20241008),   # plastic 0.77 / 0.33
    ("rep3d_p2", "j2"): (21, 20241008),   # plastic 0.75 / 0.12
    ("rep3d_p3", "j2"): (14, 20241008),   # plastic 0.66 / 0.22
    ("mix2d_31", "j2"): (7, 20241009),   # plastic 0.44 / 0.12
    ("mix3d_231", "j2"): (9, 20241012),   # plastic 0.75 / 0.26
    ("mix3d_322", "j2"): (15, 20241010),   # plastic 0.75 / 0.28
    ("rep3d_p2_o3", "j2"): (7, 20241009),   # plastic 0.78 / 0.07
    ("nurbs_tp_p2", "j2"): (12, 20241008),   # plastic 0.64 / 0.23
    ("nurbs_flat_p2", "j2"): (12, 20241008),   # plastic 0.65 / 0.22
    ("col8_p2", "j2[JohnsonCookRate]"): (8, 20241009),   # plastic 0.70 / 0.17
    ("col5_p3", "j2[JohnsonCookRate]"): (10, 20241008),   # plastic 0.77 / 0.33
    ("mix3d_231", "j2[JohnsonCookRate]"): (9, 20241012),   # plastic 0.75 / 0.25
    # the finite-strain laws, at the displacement scales of j2; with a third seed, of u2, on SECOND_PAIRS (plastic share of the
    # second assembly; j2log: share of the points with a non-symmetric Fp_inv after the second commit).  The [PowerLaw] and
    # [elastic] variants (no point plastic, trial margins below -0.3 sigma_y) pass with _patches' own seeds.
    ("rep2d_p3", "j2log"): (7, 20241008, 20241009),   # plastic 0.53 / 0.30 / 0.19, skew 0.12
    ("rep2d_p3", "j2simo"): (7, 20241008, 20241009),   # plastic 0.53 / 0.29 / 0.19
    ("col8_p2", "j2log"): (8, 20241009),   # plastic 0.70 / 0.17  (20241008: the tangent at the solver's root, `conditions`)
    ("col8_p2", "j2simo"): (18, 20241010),   # plastic 0.69 / 0.19
    ("col5_p3", "j2log"): (10, 20241008, 20241009),   # plastic 0.77 / 0.33 / 0.20, skew 0.24
    ("col5_p3", "j2simo"): (7, 20241008, 20241009),   # plastic 0.67 / 0.32 / 0.22
    ("mix3d_231", "j2log"): (23, 20241009),   # plastic 0.74 / 0.25
    ("mix3d_231", "j2simo"): (47, 20241009),   # plastic 0.70 / 0.26
    ("nurbs_tp_p2", "j2log"): (53, 20241011),   # plastic 0.70 / 0.15
    ("nurbs_tp_p2", "j2simo"): (34, 20241009),   # plastic 0.71 / 0.21
}

# Tangent of the plastic branch: not derivable (tests/test_closed_form_gpu.py, PLASTIC_TANGENT_BAR: a tangent taken at the
# solver's own root differs from one at the exact root by |dA / d delta| x 1e-10), so MEASURED the project's way -- on the CPU,
# on the oracle, against the reference's K v (three probe vectors), relative to max |K v|, never on the kernels; printed by
# tests/test_domain_reference_cpu.py::test_j2_tangent_table.  Worst over the cases, per law (the Johnson-Cook figures come from
# the points that have just yielded, where H' ~ eqps^(n - 1) is steep: col8_p2 3.1e-9, mix3d_231 1.4e-9, nurbs_tp_p2 1.2e-9,
# every other case <= 5.4e-10; PowerLaw <= 8.0e-13 everywhere).  The bar of a law is 10 x its figure, capped at 1e-8, on top
# of the rounding bar 1e-11.
J2_TANGENT_MEASURED = {"j2": 3.1e-09, "j2[PowerLaw]": 8.0e-13, "j2[JohnsonCookRate]": 3.1e-09}
J2_TANGENT_BAR = {k: min(TANGENT_CAP, 10 * v) for k, v in J2_TANGENT_MEASURED.items()}


def model_of(matname):
    """'j2log[PowerLaw]' -> 'j2log'"""
    return matname.split("[")[0]


# The same measurement for the finite-strain laws (tests/test_domain_reference_cpu.py::test_finite_tangent_table prints it):
# worst over the cases, the second step of SECOND_PAIRS included, per (model, law); the [elastic] variants have no plastic point
# and get nothing on top of 1e-11.  As for j2 the Johnson-Cook figures come from the points that have just yielded (j2log:
# col8_p2 7.3e-9, nurbs_tp_p2 2.9e-9, mix3d_231 1.7e-9, rep2d_p3 1.9e-11 and 3.3e-10 in its second step, col5_p3 <= 4.6e-13;
# j2simo: mix3d_231 4.4e-10, col8_p2 3.4e-10, nurbs_tp_p2 3.3e-10, col5_p3 1.1e-10, rep2d_p3 <= 2.3e-12); PowerLaw <= 1.0e-12.
# Not _finite_strain_inputs.FINITE_STRAIN_TANGENT_BAR: that one was measured on three named inputs far beyond yield.
FINITE_TANGENT_MEASURED = {"j2log": 7.3e-09, "j2log[PowerLaw]": 1.0e-12, "j2simo": 4.4e-10, "j2simo[PowerLaw]": 6.4e-13}
FINITE_TANGENT_BAR = {k: min(TANGENT_CAP, 10 * v) for k, v in FINITE_TANGENT_MEASURED.items()}


def is_j2(matname):
    """the small-strain J2 law with a hardening law"""
    return model_of(matname) == "j2"


def is_finite(matname):
    return model_of(matname) in FINITE_MODELS


def has_solver(matname):
    return is_j2(matname) or is_finite(matname)


def is_elastic(matname):
    return matname.endswith("[elastic]")


def law_of(matname):
    """'j2[PowerLaw]' -> 'PowerLaw'; 'j2log[elastic]' -> _finite_strain_inputs.ELASTIC_LAW; 'j2' -> None (the default law)"""
    if "[" not in matname:
        return None
    law = matname[matname.index("[") + 1:-1]
    return fi.ELASTIC_LAW if law == "elastic" else law


def reference_material(matname):
    return dr.material(model_of(matname), law_of(matname))


def oracle_material(matname):
    from _cases import oracle_material as om
    return om(model_of(matname), law_of(matname)) if law_of(matname) else om(matname)


def product_material(matname):
    from _cases import product_material as pm
    return pm(model_of(matname), law_of(matname)) if law_of(matname) else pm(matname)


@functools.lru_cache(maxsize=None)
def arrays(case):
    """the plain arrays of a case; shared, never modified"""
    c = next(d[case] for d in (CASES, WALK_CASES, ATOMICS_CASES) if case in d)
    degrees = tuple(c["degrees"])
    knots = [_patches.open_knots(p, k) for p, k in zip(degrees, c["inner"])]
    ctrl = _jittered(degrees, knots, c.get("jitter", 0.04), c.get("seed", 1))
    n_ctrl = [len(k) - p - 1 for k, p in zip(knots, degrees)]
    weights = None
    if c.get("weights") == "tensor":            # test_domain_gpu.py::test_tensor_product_nurbs_weights
        rng = np.random.default_rng(5)
        w1d = [1.0 + 0.4 * rng.uniform(-1, 1, n) for n in n_ctrl]
        w = w1d[0]
        for d in range(1, len(degrees)):
            w = np.multiply.outer(w1d[d], w)
        weights = 0.7 * w.ravel()
    elif c.get("weights") == "general":         # ::test_rational_weights_general_path
        weights = 1.0 + 0.3 * np.random.default_rng(21).uniform(-1, 1, int(np.prod(n_ctrl)))
    for a in knots + [ctrl] + ([weights] if weights is not None else []):
        a.setflags(write=False)
    spans = [np.diff(np.unique(k)) for k in knots]
    return types.SimpleNamespace(case=case, degrees=degrees, knots=knots, ctrl=ctrl, weights=weights, order=c.get("order", -1),
                                 family=c["family"], flat=c.get("flat", False), dim=len(degrees), n_ctrl=n_ctrl,
                                 n_nodes=int(np.prod(n_ctrl)), n_vdofs=int(np.prod(n_ctrl)) * len(degrees),
                                 smallest_span=min(float(s.min()) for s in spans))


def oracle_patch(case):
    from oracle import iga
    a = arrays(case)
    return iga.Patch(list(a.degrees), a.knots, a.ctrl, a.weights)


def product_patch(case):
    import mimi_amd
    a = arrays(case)
    return mimi_amd.BSplinePatch(list(a.degrees), a.knots, a.ctrl, a.weights)


def inputs(case, matname, seeds=None):
    """(u0 of the commit, u of the assemblies), as _patches.inputs: scale 0.03 / (0.05 neo-Hookean and StVK, 0.02 the J2
    laws, the finite-strain ones included) x the smallest knot span where that is below 1; both x ELASTIC_FACTOR for the
    [elastic] variants"""
    a = arrays(case)
    shim = types.SimpleNamespace(n_vdofs=a.n_vdofs, dim=a.dim, boundary_nodes=lambda axis, side: fr.face_node_ids(a.n_ctrl, axis, side))
    s0, s = (seeds or SEEDS.get((case, matname), (7, 20241008)))[:2]
    h = min(1.0, a.smallest_span)
    scale = (0.05 if matname in ("neohook", "stvk") else 0.02) * h
    factor = ELASTIC_FACTOR if is_elastic(matname) else 1.0
    return synthetic_u(shim, scale=factor * _patches.COMMIT_SCALE, seed=s0), synthetic_u(shim, scale=factor * scale, seed=s)


def second_input(case, matname, seeds=None):
    """u2 of the second step: the scale of u, the third seed"""
    a = arrays(case)
    shim = types.SimpleNamespace(n_vdofs=a.n_vdofs, dim=a.dim, boundary_nodes=lambda axis, side: fr.face_node_ids(a.n_ctrl, axis, side))
    return synthetic_u(shim, scale=0.02 * min(1.0, a.smallest_span), seed=(seeds or SEEDS[case, matname])[2])


def probes(case):
    """the three vectors a tangent is applied to: random, smooth, supported on a single (interior, where there is one) node"""
    a = arrays(case)
    random = np.random.default_rng(5).standard_normal(a.n_vdofs)
    smooth = np.stack([np.sin(0.7 * a.ctrl[:, (i + 1) % a.dim] + 0.3 * i) + 0.2 * a.ctrl[:, i] for i in range(a.dim)], axis=1).ravel()
    single = np.zeros((a.n_nodes, a.dim))
    mid = [n // 2 for n in a.n_ctrl]
    node = 0
    for d in reversed(range(a.dim)):
        node = node * a.n_ctrl[d] + mid[d]
    single[node] = [1.0, -0.5, 0.25][:a.dim]
    return [random, smooth, single.ravel()]


@functools.lru_cache(maxsize=None)
def geometry(case):
    a = arrays(case)
    sp = dr.space(a.degrees, a.knots, a.weights, a.order)
    return dr.geometry(sp, a.ctrl)


@functools.lru_cache(maxsize=None)
def pattern(case):
    """(rowptr, col, conn) of the union of the element blocks, from the reference's values"""
    out = dr.support_pattern(geometry(case).sp)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def atomics_pattern(case):
    """(rowptr, col, padded) of the CSR a handle of the atomics tests is created with.  LONG_CASE: `pattern` with the dim rows
    of the node at grid position LONG_NODE replaced by the full row 0 .. n_vdofs - 1 (columns ascending, every node's dim
    columns adjacent), padded[k] true where entry k is not an entry of `pattern`.  Every other case: `pattern`, nothing padded"""
    rowptr, col, _ = pattern(case)
    if case != LONG_CASE:
        return rowptr, col, np.zeros(len(col), dtype=bool)
    a = arrays(case)
    node = LONG_NODE[0] + a.n_ctrl[0] * LONG_NODE[1]
    full = np.arange(a.n_vdofs, dtype=np.int32)
    rows, pad = [], []
    for v in range(a.n_vdofs):
        own = col[rowptr[v]:rowptr[v + 1]]
        rows.append(full if v // a.dim == node else own)
        pad.append(~np.isin(rows[-1], own))
    out = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32),
           np.concatenate(pad))
    for x in out:
        x.setflags(write=False)
    return out


def compute(case, matname, seeds=None):
    """the reference of (case, material): commit at u0 (stateful laws), then residual and K v at u from the committed state"""
    geo = geometry(case)
    mat = reference_material(matname)
    u0, u = inputs(case, matname, seeds)
    out = types.SimpleNamespace(case=case, matname=matname, geo=geo, mat=mat, u0=u0, u=u, vectors=probes(case), commit=None, state=None, blocks={})
    if mat.stateful:
        virgin = dr.virgin_state(mat, geo.sp.n_points, geo.sp.dim)
        out.commit = dr.point_law(mat, dr.deformation_gradient(geo, u0), virgin, DT)
        out.state = out.commit.new
        out.state_before = dict(commit=virgin, assembly=out.state)
    out.asm = dr.assemble(geo, mat, u, out.state, DT, out.vectors)
    out.second = None
    if (case, matname) in SECOND_PAIRS and len(seeds or SEEDS[case, matname]) == 3:
        # the commit at u is the point law of the assembly at u: its `new` is the state the second assembly starts from
        u2 = second_input(case, matname, seeds)
        out.second = types.SimpleNamespace(u=u2, commit=out.asm.pt, state=out.asm.pt.new,
                                           asm=dr.assemble(geo, mat, u2, out.asm.pt.new, DT, out.vectors))
        out.state_before["second"] = out.asm.pt.new
        u2.setflags(write=False)
    for v in (u0, u):
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case, matname):
    """compute() with the seeds of SEEDS: computed once, shared among the tests, never modified"""
    return compute(case, matname)


def conditions(ref):
    """the conditions on the inputs of a reference, as a list of the ones that FAIL (empty: all hold), and the figures:
      det(dX/dxi) > 0 (asserted by dr.geometry) and det F > 0.25 at every point, for u0 and u;
      10 - 90 % of the points plastic at the commit, at least 5 % plastic and 5 % elastic in the assembly;
      no point where the law is discontinuous or kinked (tests/_radial_return.py): no virgin point under a Johnson-Cook law
      with yield margin in (-1e-6 sigma_y, 0.1] (the 1e-13 switch jumps by ~0.03 there and the equation may have no root),
      no point with |margin| < 1e-6 sigma_y otherwise, and for the rate laws no plastic point with
      |delta / dt - eps0_dot| < 1e-6 eps0_dot;
      on the pairs with a second step the same for u2 and the second assembly, and after the second commit at least 5 % of
      the points of j2log with max |Fp_inv - Fp_inv^T| above 1e4 x the state bar of Fp_inv there;
      for the [elastic] variants instead of the plastic shares: no point plastic, at the commit or in the assembly;
      and one more, found while pinning the oracle: no plastic point at which the reference's own ScalarSolve stops more than
      SOLVER_XTOL from the root (`reference_solver`, its iteration followed in long double).  The 2 x SOLVER_XTOL bars assume
      that the stop |d delta| < 1e-10 bounds the error; on the steep start of a Johnson-Cook curve it need not: at rep3d_p2
      with the seeds (19, 20241020) a virgin point at margin 0.27 has delta = 2.66e-10, the bisection from the upper bound
      reaches 8.5e-10, a Newton step from there lands at 7.8e-12, the next one is 4.7e-11 long and the solver stops at
      5.5e-11 -- and so does the oracle, which follows it line by line;
      and a second one, found while pinning the node blocks of J2Log: the tangent taken where the reference's solver stops
      is within TANGENT_CAP = 1e-8 of the tangent at the root, in K v over the probes and in the node blocks (`root_shift`,
      on the reference alone), for every assembly.  The tangent bars are capped at 1e-8 and assume it; at a point that has
      only just yielded (delta ~ 1e-11, below the solver's own tolerance) H' ~ eqps^(n - 1) is so steep that it need not
      hold: at col8_p2 with the seeds (8, 20241008) of j2log the node blocks of the oracle, which follows the solver line by
      line, are 1.13e-8 from the reference's, and `root_shift` gives the same 1.13e-8 from the reference alone."""
    geo, mat = ref.geo, ref.mat
    bad, fig = [], {}
    fig["min_det"] = float(geo.det.min())
    for name, u in (("u0", ref.u0), ("u", ref.u)) + ((("u2", ref.second.u),) if ref.second else ()):
        if name == "u0" and not mat.stateful:
            continue
        dF = float(dr.det(dr.deformation_gradient(geo, u)).min())
        fig[f"min_detF_{name}"] = dF
        if not dF > 0.25:
            bad.append(f"det F {dF} at {name}")
    if not mat.stateful:
        return bad, fig
    sigma_y = mat.hardening.sigma_y if mat.solver else float(mat.sigma_y)
    johnson_cook = mat.solver and mat.hardening.johnson_cook
    s0, s1 = float(ref.commit.plastic.mean()), float(ref.asm.pt.plastic.mean())
    fig["plastic_commit"], fig["plastic_assembly"] = s0, s1
    if is_elastic(ref.matname):
        if s0 or s1:
            bad.append(f"plastic shares {s0}, {s1} of an elastic variant")
    else:
        if not 0.1 < s0 < 0.9:
            bad.append(f"plastic share {s0} at the commit")
        if not (s1 >= 0.05 and 1 - s1 >= 0.05):
            bad.append(f"plastic share {s1} in the assembly")
    fig["min_abs_margin"] = np.inf
    steps = [("commit", ref.commit, np.zeros(len(geo.det))), ("assembly", ref.asm.pt, ref.state.eqps)]
    if ref.second:
        s2 = float(ref.second.asm.pt.plastic.mean())
        fig["plastic_second"] = s2
        if not (s2 >= 0.05 and 1 - s2 >= 0.05):
            bad.append(f"plastic share {s2} in the second assembly")
        steps.append(("second", ref.second.asm.pt, ref.second.state.eqps))
        if ref.matname == "j2log":
            Fp = f64(ref.second.state.Fp_inv)
            skew = np.abs(Fp - np.swapaxes(Fp, 1, 2)).max(axis=(1, 2))
            fig["skew_share"] = float((skew > 1e4 * state_bars(ref, 2)["plastic_strain"]).mean())
            if not fig["skew_share"] >= 0.05:
                bad.append(f"only {fig['skew_share']} of the points have a non-symmetric Fp_inv after the second commit")
    for name, pt, eqps_before in steps:
        margin = np.asarray(pt.margin, dtype=np.float64)
        virgin = np.asarray(eqps_before == 0)
        fig["min_abs_margin"] = min(fig["min_abs_margin"], float(np.abs(margin).min()))
        if johnson_cook and np.any(virgin & (margin > -1e-6 * sigma_y) & (margin <= 0.1)):
            bad.append(f"a virgin point in the Johnson-Cook window at the {name}")
        if np.any(np.abs(margin[~virgin if johnson_cook else slice(None)]) < 1e-6 * sigma_y):
            bad.append(f"a point on the yield surface at the {name}")
        if mat.solver:
            off = np.abs(reference_solver(mat.hardening, pt, eqps_before, ref.state_before[name]) - pt.delta)[np.asarray(pt.plastic)]
            fig["solver_stop"] = max(fig.get("solver_stop", 0.0), float(off.max(initial=0)))
            if np.any(off > rr.SOLVER_XTOL):
                bad.append(f"the reference's solver stops {float(off.max()):.2e} from the root at the {name}")
        if mat.solver and not is_elastic(ref.matname) and name != "commit":
            shift = root_shift(ref, 2 if name == "second" else 1)
            fig["root_shift"] = max(fig.get("root_shift", 0.0), *shift)
            if max(shift) > TANGENT_CAP:
                bad.append(f"the tangent at the solver's root is {shift[0]:.2e} (K v), {shift[1]:.2e} (node blocks) from the exact one at the {name}")
        if mat.solver and mat.hardening.has_rate:
            r0 = float(mat.hardening.a["eps0_dot"])
            rate = np.asarray(pt.delta, dtype=np.float64)[np.asarray(pt.plastic)] / DT
            fig["min_rate_gap"] = min(fig.get("min_rate_gap", np.inf), float(np.abs(rate - r0).min() / r0))
            if np.any(np.abs(rate - r0) < 1e-6 * r0):
                bad.append(f"a plastic point at the reference rate at the {name}")
    return bad, fig


def blocks_of(ref, step=1):
    """the node blocks D[A, i, j] = sum_q w det d_J N_A (dP_iJ / dF_jL) d_L N_A of the stiffness term in long double, dP / dF
    at every point from the unit directions e_j (x) e_L, at the inputs and the state of `ref`; computed once per ref"""
    if step not in ref.blocks:
        geo = ref.geo
        u, state = (ref.u, ref.state) if step == 1 else (ref.second.u, ref.second.state)
        pt = dr.point_law(ref.mat, dr.deformation_gradient(geo, u), state, DT, _unit_directions(len(geo.wdet), geo.sp.dim))
        ref.blocks[step] = _node_blocks(geo, pt.dP)
        ref.blocks[step].setflags(write=False)
    return ref.blocks[step]


def reference_blocks(case, matname, step=1):
    return blocks_of(reference(case, matname), step)


def _unit_directions(n, dim):
    units = []
    for j in range(dim):
        for L in range(dim):
            E = np.zeros((n, dim, dim), dtype=LD)
            E[:, j, L] = 1
            units.append(E)
    return units


def _node_blocks(geo, dPs):
    n, dim = len(geo.wdet), geo.sp.dim
    C = np.stack(dPs, axis=-1).reshape(n, dim, dim, dim, dim)                   # [q, i, J, j, L]
    half = np.einsum("qAJ,qiJjL->qAijL", geo.dNdX, C)
    return np.einsum("q,qAijL,qAL->Aij", geo.wdet, half, geo.dNdX)


def root_shift(ref, step=1):
    """what the reference's own solver does to the tangent of an assembly, on the reference alone: dP / dF taken at the
    increment where ScalarSolve stops (`reference_solver`) against dP / dF at the bisected root, as (K v over the three
    probes relative to max |K v|, node blocks relative to the largest entry).  The measured tangent figures
    (J2_TANGENT_MEASURED, FINITE_TANGENT_MEASURED) are these to three digits: col8_p2 j2 3.09e-9, col8_p2 j2log 7.27e-9"""
    geo, mat = ref.geo, ref.mat
    asm = steps_of(ref, step)[0]
    u, state = (ref.u, ref.state) if step == 1 else (ref.second.u, ref.second.state)
    idx = np.nonzero(np.asarray(asm.pt.plastic))[0]
    stopped = reference_solver(mat.hardening, asm.pt, state.eqps, state)[idx]
    dFs = [dr.gradient(geo, v)[idx] for v in ref.vectors] + _unit_directions(len(idx), geo.sp.dim)
    F, st = dr.deformation_gradient(geo, u)[idx], dr.take(state, idx)
    exact, off = dr.point_law(mat, F, st, DT, dFs), dr.point_law(mat, F, st, DT, dFs, delta=stopped)
    diff = []
    for a, b in zip(off.dP, exact.dP):
        d = np.zeros((len(geo.wdet),) + a.shape[1:], dtype=LD)
        d[idx] = a - b
        diff.append(d)
    n = len(ref.vectors)
    Kv = max(float(np.abs(dr.nodal(geo, d)).max() / np.abs(k).max()) for d, k in zip(diff[:n], asm.Kv))
    return Kv, float(np.abs(_node_blocks(geo, diff[n:])).max() / np.abs(blocks_of(ref, step)).max())


def reference_solver(h, pt, eqps, state):
    """what the reference's ScalarSolve (solvers/newton.hpp:53-169: Newton from 0, bisection where a step leaves the bracket
    or does not halve the residual, stop at |dx| < 1e-10 or |R| < sigma_y 1e-10; its derivative holds the rate factor fixed,
    material_hardening.hpp:69-71) returns for the scalar equation of every point of pt, followed in long double -- only to
    see where it stops (`conditions`), never as an answer.  The equation is q - slope0 x - H(eqps + x) rate thermo with
    slope0 = 3 G (j2, j2log) or G tr be and q = s_eff (j2simo): the same scalar_solve serves the three models"""
    G3 = pt.slope0
    q, dt = pt.q, LD(DT)
    thermo = h.thermo(state.temperature)
    xtol, rtol = LD(rr.SOLVER_XTOL), LD(h.sigma_y) * LD(1e-10)

    def R(x):
        fac = h.rate(x / dt) * thermo
        return q - G3 * x - h.H(eqps + x) * fac, -G3 - h.dH(eqps + x) * fac

    lower, upper = np.zeros_like(q), np.where(pt.plastic, (q - h.H(eqps) * thermo) / G3, LD(0))
    fl, fh = R(lower)[0], R(upper)[0]
    x = np.where(np.abs(fl) < xtol, lower, upper)
    done = ~np.asarray(pt.plastic) | (np.abs(fl) < xtol) | (np.abs(fh) < xtol)
    xl, xh = np.where(fl > 0, upper, lower), np.where(fl > 0, lower, upper)
    x = np.where(done, x, LD(0))
    dx = dx_old = np.abs(upper - lower)
    f, df = R(x)
    for _ in range(100):
        bisect = ((x - xh) * df - f > 0) | ((x - xl) * df - f < 0) | (np.abs(2 * f) > np.abs(dx_old * df))
        step = np.where(bisect, (xh - xl) / 2, f / df)
        x = np.where(done, x, np.where(bisect, xl + step, x - step))
        dx_old, dx = dx, step
        f, df = R(x)
        xl, xh = np.where(~done & (f < 0), x, xl), np.where(~done & ~(f < 0), x, xh)
        done = done | (np.abs(dx) < xtol) | (np.abs(f) < rtol)
        if done.all():
            break
    assert done.all(), "the reference's solver does not converge"
    return np.where(pt.plastic, x, LD(0))


def _finite_trial_deviator(mat, F, st, G):
    """the trial deviator of j2log (2 G dev E_e) or j2simo (G dev be: s_eff = sqrt(3/2) |s|) in doubles, numpy's eigh"""
    dim = F.shape[-1]
    if mat.name == "j2log":
        Fe = F @ np.asarray(st.Fp_inv, dtype=np.float64)
        lam, Q = np.linalg.eigh(np.swapaxes(Fe, 1, 2) @ Fe)
        A, factor = np.einsum("nia,na,nja->nij", Q, 0.5 * np.log(lam), Q), 2 * G
    else:
        f = F @ np.linalg.inv(np.asarray(st.F_old, dtype=np.float64))
        f = f * np.cbrt(np.linalg.det(f))[:, None, None]
        A, factor = f @ np.asarray(st.be_old, dtype=np.float64) @ np.swapaxes(f, 1, 2), G
    return factor * (A - np.trace(A, axis1=1, axis2=2)[:, None, None] / dim * np.eye(dim))


def _trial_margins(geo64, mat, u, state):
    """(yield margin of the trial state, det F, virgin) at every point, in doubles: the quick look of the scan"""
    dNdX, dim = geo64
    F = np.eye(dim) + np.einsum("Ai,qAJ->qiJ", u.reshape(-1, dim), dNdX)
    n = len(F)
    st = dr.virgin_state(mat, n, dim) if state is None else state
    eps = 0.5 * (F + np.swapaxes(F, 1, 2)) - np.eye(dim) - (0.0 if mat.name in FINITE_MODELS else np.asarray(st.plastic_strain, dtype=np.float64))
    G = float(dr.constants()[3])
    s = 2 * G * (eps - np.trace(eps, axis1=1, axis2=2)[:, None, None] / dim * np.eye(dim))
    if mat.name in FINITE_MODELS:
        s = _finite_trial_deviator(mat, F, st, G)
    if mat.solver:
        h = mat.hardening
        q = np.sqrt(1.5) * np.sqrt((s * s).sum(axis=(1, 2)))
        margin = q - np.asarray(h.H(st.eqps) * h.thermo(st.temperature), dtype=np.float64)
    else:
        eta = s - np.asarray(st.beta, dtype=np.float64)
        margin = np.sqrt(1.5) * np.sqrt((eta * eta).sum(axis=(1, 2))) - np.asarray(mat.sigma_y + mat.h_iso * st.eqps, dtype=np.float64)
    return margin, np.linalg.det(F), np.asarray(st.eqps == 0)


def _quick(geo64, mat, u, state, share):
    """the conditions that need no return map, on the trial state in doubles (the scan's sieve; `conditions` decides)"""
    margin, detF, virgin = _trial_margins(geo64, mat, u, state)
    sigma_y = mat.hardening.sigma_y if mat.solver else float(mat.sigma_y)
    s = float((margin > 0).mean())
    if detF.min() <= 0.25 or not share[0] < s < share[1]:
        return False
    if mat.solver and mat.hardening.johnson_cook:
        if np.any(virgin & (margin > -1e-6 * sigma_y) & (margin <= 0.1)):
            return False
        return not np.any(np.abs(margin[~virgin]) < 1e-6 * sigma_y)
    return not np.any(np.abs(margin) < 1e-6 * sigma_y)


def scan_seeds(case, matname, tries=20000):
    """the seeds of SEEDS: the first seed 7 + k of u0 at which the commit satisfies the conditions, then the first seed
    20241008 + k of u at which the whole of `conditions` holds; on SECOND_PAIRS then the first seed of u2 above that of u at
    which the conditions of the second step hold as well"""
    geo, mat = geometry(case), reference_material(matname)
    geo64 = (np.asarray(geo.dNdX, dtype=np.float64), geo.sp.dim)
    shares = ((-1.0, 1e-12), (-1.0, 1e-12)) if is_elastic(matname) else ((0.1, 0.9), (0.05, 0.95))
    for k0 in range(tries):
        u0 = inputs(case, matname, (7 + k0, 0))[0]
        if not _quick(geo64, mat, u0, None, shares[0]):
            continue
        try:
            virgin = dr.virgin_state(mat, geo.sp.n_points, geo.sp.dim)
            pt = dr.point_law(mat, dr.deformation_gradient(geo, u0), virgin, DT)
        except AssertionError:          # (the reference's own bracket check: a root that does not exist)
            continue
        state = pt.new
        if mat.solver and np.any(np.abs(reference_solver(mat.hardening, pt, virgin.eqps, virgin) - pt.delta) > rr.SOLVER_XTOL):
            continue
        for k in range(200):
            u = inputs(case, matname, (7 + k0, 20241008 + k))[1]
            if not _quick(geo64, mat, u, state, shares[1]):
                continue
            try:
                bad, _ = conditions(compute(case, matname, (7 + k0, 20241008 + k)))
            except AssertionError:
                continue
            if not bad and (case, matname) in SECOND_PAIRS:
                return _scan_third_seed(case, matname, 7 + k0, 20241008 + k)
            if not bad:
                return 7 + k0, 20241008 + k
    raise RuntimeError(f"no seed of {tries} satisfies the conditions for {case} {matname}")


def _scan_third_seed(case, matname, s0, s):
    for k in range(1, 200):
        try:
            bad, _ = conditions(compute(case, matname, (s0, s, s + k)))
        except AssertionError:
            continue
        if not bad:
            return s0, s, s + k
    raise RuntimeError(f"no third seed satisfies the conditions for {case} {matname}")


# ---- bars of the J2 laws ---------------------------------------------------------------------------------------------------
def carry(matname, pt, earlier):
    """the factor with which the error that the earlier commit `earlier` left in the state reaches the trial stress at the
    points `pt`, relative to pt's own one-step bar (tests/_finite_strain_return.py, `Result.carry` and `sequence_bar`):
    1 for the small-strain law, cond(C_e) of pt for j2log, |f_bar|_2^2 tr(be then) / tr(be now), at least 1, for j2simo"""
    if is_j2(matname):
        return np.ones(len(pt.q))
    if model_of(matname) == "j2log":
        return f64(pt.cond)
    return np.maximum(1.0, f64(pt.fbar2 * earlier.tr_be / pt.tr_be))


def steps_of(ref, step):
    """(the assembly, the commits before it) of step 1 (commit at u0, assembly at u) or 2 (commit at u, assembly at u2)"""
    return (ref.asm, [ref.commit]) if step == 1 else (ref.second.asm, [ref.commit, ref.second.commit])


def stress_bar_points(ref, step=1):
    """the stress bar per point of an assembly: the one-step bar 2 x 1e-10 x |dP / d delta| (j2, j2log:
    2 G sqrt(3/2) |det F F^-T|_F; j2simo: G 2/3 tr(be) sqrt(3/2) |F^-T|_F) once where the point is plastic in the assembly,
    and `carry` times for every earlier commit at which it was plastic -- sequence_bar, point by point"""
    asm, earlier = steps_of(ref, step)
    pt = asm.pt
    one = rr.stress_bar(f64(pt.JFinvT_norm)) if is_j2(ref.matname) else STATE_BAR * f64(pt.stress_scale)
    count = f64(pt.plastic) + sum(f64(e.plastic) * carry(ref.matname, pt, e) for e in earlier)
    return one * count


def residual_bar(ref, mask=None, step=1):
    """per row (A, i): 1e-12 max |r|, and for the laws with a solver the derived sum_q w det sum_J |dN_A/dX_J| stress_bar(q)
    (tests/_radial_return.py, tests/_finite_strain_return.py) over the plastic points.  A point that was plastic at the commit
    carries the solver's 1e-10 in its committed state into the trial stress of the assembly (j2: 2 G sqrt(3/2) 1e-10, the same
    bound; the finite-strain laws: that times `carry`), a point that is plastic in the assembly adds its own: one stress_bar
    for either, two for both, as test_closed_form_gpu.py's two-step test.  The [elastic] variants have no plastic point and so
    nothing beyond the rounding bar."""
    asm = steps_of(ref, step)[0]
    r = np.asarray(asm.r if mask is None else dr.nodal(ref.geo, asm.pt.P, mask), dtype=np.float64)
    bar = np.full(r.size, RESIDUAL_BAR * np.abs(r).max())
    if has_solver(ref.matname):
        geo = ref.geo
        per_point = stress_bar_points(ref, step)
        if mask is not None:
            per_point = per_point * mask
        row = np.einsum("q,qA->A", np.asarray(geo.wdet, dtype=np.float64) * per_point, np.abs(np.asarray(geo.dNdX, dtype=np.float64)).sum(axis=2))
        bar = bar + np.repeat(row, geo.sp.dim)
    return bar


def tangent_bar(matname):
    return TANGENT_BAR + J2_TANGENT_BAR.get(matname, 0.0) + FINITE_TANGENT_BAR.get(matname, 0.0)


def state_bars(ref, step=1):
    """absolute bars of the state committed at step 1 (at u0, from the virgin state) or 2 (at u): eqps, first matrix
    (`plastic_strain`: the plastic strain, Fp_inv or be_old), temperature, second matrix (`state2`: back stress or F_old).
    J2, from |delta - delta_exact| <= 2 x SOLVER_XTOL = B: eqps B, plastic strain sqrt(3/2) B (|N_p|_F = sqrt(3/2)),
    temperature chi q / (rho c) B.  J2Linear's return is closed-form: rounding only, 1e-12 of the largest entry.
    j2log: eqps B; Fp_inv <- Fp_inv_old exp(-d N_p) moves by Fp_inv_old N_p per unit of d: sqrt(3/2) |Fp_inv_old|_F B; the
    temperature is never touched (the bar of j2simo, for a value that does not move).
    j2simo: eqps B; be <- be - 2/3 d tr(be) N_p: 2/3 tr(be) sqrt(3/2) B; T += chi s_eff d / (rho c): chi s_eff / (rho c) B;
    F_old = F is rounding only: 1e-12 of the largest entry, as J2Linear.
    The [elastic] variants: no point yields, nothing carries the solver's tolerance: 1e-12 of the largest entry throughout
    (eqps is exactly 0 on both sides).
    Step 2 starts from a state that is itself off by the bars of step 1 at the points that were plastic then (B1 = B there,
    0 elsewhere); c = `carry`:
      the trial stress is off by c x the one-step stress bar, which moves the root of the scalar equation by at most c B1
      (j2log: |dq| <= sqrt(3/2) 2 G |dE_e|_F <= 3 G c B1 against a slope >= 3 G; j2simo: |d s_eff| <= G tr(be) c B1 against
      a slope >= G tr be), and eqps_old is off by B1:                                   eqps   B + (1 + c) B1
      the matrix inherits the old error through the step (c x its own bar: for j2log |exp(-d N_p)|_2 <= e^d is within the
      factor 2 of B), moves along N_p by the shifted root (c B1) and turns with N_p, whose error is |ds| / |s| times
      3 G d / q <= 1 (j2log) or G tr(be) d / s_eff <= 1 (j2simo), i.e. again at most c x the bar:
                                                                                        matrix (1 + (1 + 2 c) [plastic at 1]) x its bar
      the temperature adds chi / (rho c) (s_eff (B + c B1) + d |d s_eff|) <= chi s_eff / (rho c) (B + 2 c B1) to its old
      error chi s_eff_1 / (rho c) B1:                                                   (1 + (1 + 2 c) [..]) x the larger bar"""
    commit = ref.commit if step == 1 else ref.second.commit
    new = commit.new
    big = lambda a: 1e-12 * float(np.abs(a).max())
    if ref.matname == "j2linear":
        return dict(eqps=big(new.eqps), plastic_strain=big(new.plastic_strain), state2=big(new.beta))
    if is_elastic(ref.matname):
        bars = dict(eqps=max(big(new.eqps), np.finfo(np.float64).tiny), temperature=big(new.temperature),
                    plastic_strain=big(first_matrix(ref.matname, new)))
        if model_of(ref.matname) == "j2simo":
            bars["state2"] = big(new.F_old)
        return bars
    th = ref.mat.hardening.thermal
    heat = float(th["heat_fraction"] / th["specific_heat"]) * f64(commit.q)
    if is_j2(ref.matname):
        return dict(eqps=STATE_BAR, plastic_strain=np.sqrt(1.5) * STATE_BAR, temperature=heat * STATE_BAR)
    before = ref.state_before["commit" if step == 1 else "assembly"]
    if model_of(ref.matname) == "j2log":
        matrix = np.sqrt(1.5) * f64(dr.frob(before.Fp_inv))
    else:
        matrix = 2.0 / 3.0 * np.sqrt(1.5) * f64(commit.tr_be)
    bars = dict(eqps=np.full(len(heat), STATE_BAR), plastic_strain=matrix * STATE_BAR, temperature=heat * STATE_BAR)
    if step == 2:
        first = ref.commit
        was = f64(first.plastic)
        c = carry(ref.matname, commit, first)
        heat1 = float(th["heat_fraction"] / th["specific_heat"]) * f64(first.q)
        bars = dict(eqps=STATE_BAR * (1 + (1 + c) * was), plastic_strain=bars["plastic_strain"] * (1 + (1 + 2 * c) * was),
                    temperature=np.maximum(heat, heat1) * STATE_BAR * (1 + (1 + 2 * c) * was))
    if model_of(ref.matname) == "j2simo":
        bars["state2"] = big(new.F_old)
    return bars


def first_matrix(matname, state):
    """the first state matrix, as mimi_hip_domain_get_state names it: the plastic strain, Fp_inv (j2log) or be_old (j2simo)"""
    return getattr(state, {"j2log": "Fp_inv", "j2simo": "be_old"}.get(model_of(matname), "plastic_strain"))


def f64(a):
    return np.asarray(a, dtype=np.float64)


def compare_state(ref, get, grid, label="", step=1):
    """the committed state of `get(name)` ([e, q] / [e, q, i + J dim]) against the reference's at grid[e, q] (step 1: after the
    commit at u0; 2: after the one at u): sorted values first (a misread layout then shows as a layout error, not a value
    error), then point by point.  Returns the worst error / bar"""
    new, bars = (ref.commit if step == 1 else ref.second.commit).new, state_bars(ref, step)
    n = len(new.eqps)
    flat = lambda M: f64(np.swapaxes(M, 1, 2).reshape(n, -1))
    want = dict(eqps=f64(new.eqps), plastic_strain=flat(first_matrix(ref.matname, new)))
    names = dict(eqps="accumulated_plastic_strain", plastic_strain="plastic_strain", temperature="temperature", state2="state2")
    if ref.matname == "j2linear":
        want["state2"] = flat(new.beta)
    else:
        want["temperature"] = f64(new.temperature)
    if model_of(ref.matname) == "j2simo":
        want["state2"] = flat(new.F_old)
    worst = 0.0
    for key, w in want.items():
        got = np.asarray(get(names[key]))
        w = w[grid]
        assert got.shape == w.shape, (key, got.shape, w.shape)
        bar = bars[key][grid] if np.ndim(bars[key]) else bars[key]
        flat_bar = np.max(bar)
        assert np.all(np.abs(np.sort(got.ravel()) - np.sort(w.ravel())) <= flat_bar), f"{label} {key}: the VALUES differ"
        err = np.abs(got - w) / (bar[..., None] if np.ndim(bar) and got.ndim == 3 else bar)
        assert err.max() <= 1.0, f"{label} {key}: the values agree as a set but not point by point -- the LAYOUT differs ({err.max():.2e} of the bar)"
        worst = max(worst, float(err.max()))
    return worst


@functools.lru_cache(maxsize=None)
def flat_tables(case):
    """the tables of mimi_hip_domain_create from the reference's values rounded to double: dofs[e, a] (ascending node ids),
    dN_dX[e, q, J, a], weight_det[e, q], N[e, q, a], in the (element, point) layout"""
    geo = geometry(case)
    sp_, conn = geo.sp, pattern(case)[2]
    grid = dr.layout(sp_)
    pts = grid[:, :, None]
    return dict(dim=sp_.dim, n_nodes=sp_.n_nodes, dofs=np.ascontiguousarray(conn),
                dN_dX=np.ascontiguousarray(np.transpose(f64(geo.dNdX[pts, conn[:, None, :], :]), (0, 1, 3, 2))),
                weight_det=np.ascontiguousarray(f64(geo.wdet[grid])), N=np.ascontiguousarray(f64(sp_.N[pts, conn[:, None, :]])))
