"""Cases and predicate of tests/test_status_cases_cpu.py, test_status_gpu.py and test_status_solid_gpu.py: the device status
word of the domain integrator (csrc/domain_create.hpp: check_status) -- does a kernel whose return map cannot solve its scalar
equation tell anyone.

The failure, with public classes and finite inputs: a SOFTENING hardening law.  scalar_solve (csrc/materials.hpp) brackets the
root of R(d) = q - slope d - H(eqps + d) rate thermo in [0, upper], upper = (q - H(eqps) thermo) / slope, and under a law whose
H decreases R(upper) = thermo (H(eqps) - H(eqps + upper)) > 0: every yielding point is unbracketed (bit 1, "root not bracketed
by input bounds"), every other point is untouched.  So "the call raises" is exactly "some point yields", and the predicate
"this point yields" -- trial q above H(eqps) thermo -- is taken from the long-double reference alone
(_domain_reference.trial_state, the trial state point_law itself starts from), never from the device or the oracle.

Laws (LAWS, in the format of _cases.HARDENING_LAWS; every one has sigma_y = 70 and no thermal factor, so on the virgin state
the yield stress is 70 under all four and a field's predicate does not depend on the law):
  VoceSoft         Voce, sigma_sat 20 < sigma_y 70            PowerLawSoft   PowerLaw, n = -4
  JohnsonCookSoft  JohnsonCook, B = -30                       VoceHard       _cases' own Voce (sigma_sat 150): the negative control

Shapes (tests/_domain_cases.py), one per kernel family plus flat tables, the smallest that keep a tail: rep2d_p3 (tensor_small,
four elements per workgroup), col8_p2 (tensor_p2_two_phase, 32 elements), col5_p3 (tensor_p3_two_phase, 10 elements, 125
points on two waves), mix3d_231 (general), flat2d_p4 (general, flat tables).

Fields, all on the virgin state with dt = _domain_cases.DT, the same for the three models j2, j2simo, j2log:
  quiet         synthetic_u at QUIET_SCALE: no point yields
  corner_first  only the first corner control point (node 0) moves, by FIELDS[shape]["corner_first"] = (amplitude, seed of the
                direction): its basis function lives on element 0 alone, so every yielding point lies there -- the first lane of
                the first workgroup
  corner_last   the same for the last corner control point and the last element -- the tail of the last workgroup
  many          a sheared block on a clamped one, with synthetic_u on top: the first `planes` node planes along the last axis
                stay at zero, every node A above them moves by gamma (Z_A - z0) d + synthetic_u(noise, seed)_A, Z_A the
                node's own last coordinate, z0 the mean one of the last clamped plane, d a unit vector across the axis
                (from the seed); FIELDS[shape]["many"] = (gamma, noise, seed, planes).  Splines reproduce the affine part, so
                the points fed by free nodes alone see the simple shear gamma (ratio sqrt(3) G gamma / 70 ~ 3, det F = 1)
                plus the noise, the points fed by clamped nodes alone have q = 0 exactly, and only the few point layers
                between the two can come near the yield stress: 20 - 80 % of the points yield.  A plain synthetic_u cannot
                meet the band condition below on these shapes: its trial q is spread continuously through the yield stress,
                and at the largest scale that det F > 0.5 allows (0.1 of a knot span) the median count of points within
                10 % of it is 15 of the 2048 of col8_p2, the best of 200 seeds 4 (1 with all but two node planes
                clamped).
Conditions on the inputs (`conditions`; asserted in tests/test_status_cases_cpu.py, never relaxed): every point of every field
has q / (H(0) thermo) outside [0.9, 1.1] (BAND: fp64 and long double cannot disagree about who yields -- the two differ by
1e-16 relative); quiet has no yielding point; each corner field has at least one and all of them in its element; many has
20 - 80 %; det F > 0.5 everywhere.  `scan` is how FIELDS was found.

Bit 2 ("failed to converge in allotted iterations") is reached by no test, and no finite input that reaches it was found.  The
argument: scalar_solve enters its loop only with a bracket, R(0) > 0 >= R(upper) (else bit 1), keeps a bracket [xl, xh] with
R(xl) > 0 > R(xh) throughout, and takes a bisection step whenever the Newton step would leave the bracket or fails to halve
the residual (solvers/newton.hpp:53-169).  It stops at |dx| < 1e-10.  The bracket is no wider than upper = margin / slope
<= q / (3 G) ~ q / 2400 (G tr be for j2simo, of the same size), so 100 bisections alone shrink it to q 2^-100 / 2400, below
1e-10 for every q < 1e23; and between bisections a Newton step that is accepted at least halves |R|, so it cannot hold the
loop either: the stop |R| < sigma_y 1e-10 is reached after at most log2(q / 7e-9) < 80 halvings for q < 1e15.  A trial q that
large needs strains beyond 1e11, where det F > 0 fails long before; what is left is a non-finite R (NaN compares false with
everything, so no stop ever fires), and feeding NaNs is not a test of the solver."""
import functools
import types

import numpy as np

import _domain_cases as dc
import _domain_reference as dr
import _face_reference as fr
from _cases import HARDENING_LAWS, POISSON, THERMAL, YOUNG, _law, synthetic_u

LD = np.longdouble
DT = dc.DT
LAWS = {
    "VoceSoft": _law("Voce", "VoceHardening", dict(sigma_y=70, sigma_sat=20, strain_constant=0.05)),
    "PowerLawSoft": _law("PowerLaw", "PowerLawHardening", dict(sigma_y=70, n=-4, eps0=0.01)),
    "JohnsonCookSoft": _law("JohnsonCook", "JohnsonCookHardening", dict(A=70, B=-30, n=0.5)),
    "VoceHard": HARDENING_LAWS["Voce"],
}
SOFT_LAWS = ("VoceSoft", "PowerLawSoft", "JohnsonCookSoft")
MAIN_LAW, CONTROL_LAW = "VoceSoft", "VoceHard"
MODELS = ("j2", "j2simo", "j2log")
SHAPES = ("rep2d_p3", "col8_p2", "col5_p3", "mix3d_231", "flat2d_p4")
# one shape per kernel family for the two other softening laws
FAMILY_SHAPES = tuple(dc.EXTRA.values())
FIELD_NAMES = ("quiet", "corner_first", "corner_last", "many")
RAISING_FIELDS = FIELD_NAMES[1:]
BAND = (0.9, 1.1)
SHARE = (0.2, 0.8)
MIN_DET_F = 0.5
QUIET_SCALE = 1e-4
MESSAGE = "root not bracketed"
# the facade's problem (tests/test_status_solid_gpu.py): sq_p2 of tests/_explicit_cases.py under a body force along x, one
# implicit step from rest; sized on the CPU with the oracle's own stepper (tests/test_status_cases_cpu.py)
SOLID_CASE, SOLID_BODY_FORCE, SOLID_STEP = "sq_p2", 20.0, 0.5

# shape -> field -> parameters, what `scan(shape)` finds first (the figures: yielding points / points, the ratios q / yield
# stress nearest to the band from below and from above, over the three models)
FIELDS = {
    # every corner field makes exactly one point yield
    "rep2d_p3": dict(corner_first=(0.01735, 0),   # 1 / 225, 0.750 | 1.337
                     corner_last=(0.01828, 0),   # 1 / 225, 0.739 | 1.359
                     many=(0.15, 0.01, 1, 4)),   # 105 / 225, 0.892 | 1.266
    "col8_p2": dict(corner_first=(0.02335, 0),   # 1 / 2048, 0.786 | 1.238
                    corner_last=(0.0245, 0),   # 1 / 2048, 0.797 | 1.271
                    many=(0.2, 0.01, 0, 5)),   # 1216 / 2048, 0.310 | 1.156
    "col5_p3": dict(corner_first=(0.01541, 0),   # 1 / 1250, 0.746 | 1.292
                    corner_last=(0.01705, 0),   # 1 / 1250, 0.765 | 1.322
                    many=(0.15, 0.01, 4, 4)),   # 800 / 1250, 0.899 | 1.239
    # (degree 1 along the last axis: the corner function decays slowly and the two largest ratios are only 1.25 apart)
    "mix3d_231": dict(corner_first=(0.01726, 4),   # 1 / 3000, 0.895 | 1.117
                      corner_last=(0.01893, 3),   # 1 / 3000, 0.899 | 1.105
                      many=(0.15, 0.01, 0, 2)),   # 2250 / 3000, 0.000 | 1.980
    "flat2d_p4": dict(corner_first=(0.01162, 0),   # 1 / 144, 0.730 | 1.378
                      corner_last=(0.01692, 0),   # 1 / 144, 0.834 | 1.199
                      many=(0.15, 0.01, 0, 3)),   # 108 / 144, 0.654 | 1.141
}


def material(model, law):
    """the long-double reference's material (only its trial state is ever used: under a softening law there is no root)"""
    return dr.material(model, law, table=LAWS)


def oracle_material(model, law):
    from oracle import ref_path as rp
    return rp.make_material(model, YOUNG, POISSON, density=1.0, hardening=LAWS[law][0], **THERMAL)


def product_material(model, law):
    import mimi_amd
    m = {"j2": mimi_amd.J2, "j2simo": mimi_amd.J2Simo, "j2log": mimi_amd.J2Log}[model]()
    m.density = 1.0
    m.set_young_poisson(YOUNG, POISSON)
    for k, v in THERMAL.items():
        setattr(m, k, v)
    h = getattr(mimi_amd, LAWS[law][1])()
    for k, v in LAWS[law][2].items():
        setattr(h, k, v)
    m.hardening = h
    return m


def _shim(a, clamp_axis):
    return types.SimpleNamespace(n_vdofs=a.n_vdofs, dim=a.dim, boundary_nodes=lambda axis, side: fr.face_node_ids(a.n_ctrl, axis, side))


def corner_node(shape, which):
    return 0 if which == "corner_first" else dc.arrays(shape).n_nodes - 1


def make_field(shape, name, params=None):
    """the displacement of a field from its parameters (module docstring)"""
    a = dc.arrays(shape)
    h = min(1.0, a.smallest_span)
    if name == "quiet":
        return synthetic_u(_shim(a, 0), scale=QUIET_SCALE * h, seed=7)
    params = FIELDS[shape][name] if params is None else params
    if name in ("corner_first", "corner_last"):
        amplitude, seed = params
        d = np.random.default_rng(seed).standard_normal(a.dim)
        u = np.zeros((a.n_nodes, a.dim))
        u[corner_node(shape, name)] = amplitude * d / np.linalg.norm(d)
        return u.ravel()
    gamma, noise, seed, planes = params
    axis = a.dim - 1
    plane = np.unravel_index(np.arange(a.n_nodes), a.n_ctrl, order="F")[axis]
    Z = a.ctrl[:, axis]
    d = np.zeros(a.dim)
    d[:axis] = np.random.default_rng(seed).standard_normal(axis)
    ramp = gamma * (Z - Z[plane == planes - 1].mean())
    u = np.outer(ramp, d / np.linalg.norm(d)) + synthetic_u(_shim(a, axis), scale=noise, seed=seed, clamp_axis=axis).reshape(a.n_nodes, a.dim)
    u[plane < planes] = 0.0
    return u.ravel()


@functools.lru_cache(maxsize=None)
def field(shape, name):
    """shared, never modified"""
    u = make_field(shape, name)
    u.setflags(write=False)
    return u


def trial(shape, model, u):
    """(ratio q / (H(0) thermo) [q] in long double, det F [q]) of the trial state on the virgin state: the reference's own"""
    geo = dc.geometry(shape)
    mat = material(model, MAIN_LAW)
    F = dr.deformation_gradient(geo, u)
    t = dr.trial_state(mat, F, dr.virgin_state(mat, geo.sp.n_points, geo.sp.dim))
    return t.q / t.limit, dr.det(F)


@functools.lru_cache(maxsize=None)
def predicate(shape, model, name):
    """which points yield under `field(shape, name)`: yields [q] (grid index), ratio [q], det_F [q], element [q] (the element of
    every point in the (element, point) layout); from the long-double reference alone.  Every law of LAWS has the same virgin
    yield stress (asserted), so there is no law argument"""
    geo = dc.geometry(shape)
    for law in LAWS:
        h = material(model, law).hardening
        assert float(h.H(np.zeros(1, dtype=LD))[0]) == 70.0 and float(h.thermo(np.full(1, LD(THERMAL["initial_temperature"])))[0]) == 1.0
    ratio, detF = trial(shape, model, field(shape, name))
    grid = dr.layout(geo.sp)
    element = np.empty(geo.sp.n_points, dtype=np.int64)
    element[grid] = np.arange(grid.shape[0])[:, None]
    out = types.SimpleNamespace(yields=np.asarray(ratio > 1), ratio=np.asarray(ratio, dtype=np.float64),
                                det_F=np.asarray(detF, dtype=np.float64), element=element, n_elements=grid.shape[0])
    for v in (out.yields, out.ratio, out.det_F, out.element):
        v.setflags(write=False)
    return out


def expected_to_raise(shape, model, law, name):
    return law != CONTROL_LAW and bool(predicate(shape, model, name).yields.any())


def _check(name, ratio, detF, element, n_elements):
    bad = []
    yields = ratio > 1
    if np.any((ratio >= BAND[0]) & (ratio <= BAND[1])):
        bad.append(f"{int(((ratio >= BAND[0]) & (ratio <= BAND[1])).sum())} points within the band {BAND} of the yield stress")
    if not detF.min() > MIN_DET_F:
        bad.append(f"det F {float(detF.min())}")
    share = float(yields.mean())
    if name == "quiet" and yields.any():
        bad.append(f"{int(yields.sum())} points yield under the quiet field")
    if name in ("corner_first", "corner_last"):
        owner = 0 if name == "corner_first" else n_elements - 1
        if not yields.any():
            bad.append("no point yields")
        if np.any(element[yields] != owner):
            bad.append(f"points of the elements {sorted(set(element[yields]) - {owner})} yield, not only of element {owner}")
    if name == "many" and not SHARE[0] <= share <= SHARE[1]:
        bad.append(f"{share:.3f} of the points yield")
    return bad


def conditions(shape, model, name):
    """the conditions on the inputs (module docstring) as the list of those that FAIL, and the figures"""
    p = predicate(shape, model, name)
    below, above = p.ratio[p.ratio < BAND[0]], p.ratio[p.ratio > BAND[1]]
    fig = dict(yielding=int(p.yields.sum()), points=len(p.yields), below=float(below.max(initial=0.0)),
               above=float(above.min(initial=np.inf)), min_det_F=float(p.det_F.min()))
    return _check(name, p.ratio, p.det_F, p.element, p.n_elements), fig


# ---- how FIELDS was found -------------------------------------------------------------------------------------------------
def _quick_ratio(shape, u):
    """the trial ratio of the small-strain law in doubles: the scan's sieve (`conditions`, on the reference, decides)"""
    geo = dc.geometry(shape)
    dim = geo.sp.dim
    dNdX = _dNdX64(shape)
    F = np.eye(dim) + np.einsum("Ai,qAJ->qiJ", u.reshape(-1, dim), dNdX)
    eps = 0.5 * (F + np.swapaxes(F, 1, 2)) - np.eye(dim)
    G = float(dr.constants()[3])
    s = 2 * G * (eps - np.trace(eps, axis1=1, axis2=2)[:, None, None] / dim * np.eye(dim))
    return np.sqrt(1.5) * np.sqrt((s * s).sum(axis=(1, 2))) / 70.0, np.linalg.det(F)


@functools.lru_cache(maxsize=None)
def _dNdX64(shape):
    return np.asarray(dc.geometry(shape).dNdX, dtype=np.float64)


def _holds(shape, name, params):
    """the conditions for the three models at once, the sieve first"""
    geo = dc.geometry(shape)
    grid = dr.layout(geo.sp)
    element = np.empty(geo.sp.n_points, dtype=np.int64)
    element[grid] = np.arange(grid.shape[0])[:, None]
    u = make_field(shape, name, params)
    ratio, detF = _quick_ratio(shape, u)
    if _check(name, ratio, detF, element, grid.shape[0]):
        return False
    for model in MODELS:
        ratio, detF = trial(shape, model, u)
        if _check(name, np.asarray(ratio, dtype=np.float64), np.asarray(detF, dtype=np.float64), element, grid.shape[0]):
            return False
    return True


def scan(shape, seeds=4000):
    """FIELDS[shape].  A corner field: the trial q of the small-strain law is linear in the amplitude, so the sorted ratios at a
    unit amplitude show where the band fits -- the first direction seed, then the fewest yielding points k, at which the k-th
    and (k + 1)-th largest ratios are a factor 1.4 apart (where there is none, 1.23: the band itself takes 1.1 / 0.9 = 1.222),
    the amplitude at their geometric mean, and the conditions hold for the three models.  `many`: the clamp nearest to half of the node planes, gamma of (0.15, 0.2, 0.12), the noise
    at 0.01 x the smallest knot span, then the first seed"""
    a = dc.arrays(shape)
    h = min(1.0, a.smallest_span)
    out = {}
    for name in ("corner_first", "corner_last"):
        def candidates():
            for gap in (1.4, 1.23):
                for seed in range(50):
                    unit = np.sort(_quick_ratio(shape, make_field(shape, name, (1e-3 * h, seed)))[0])[::-1]
                    for k in range(1, 13):
                        if unit[k - 1] >= gap * unit[k]:
                            yield float(f"{1e-3 * h / np.sqrt(unit[k - 1] * unit[k]):.4g}"), seed
        out[name] = next(p for p in candidates() if _holds(shape, name, p))
    n_last = a.n_ctrl[a.dim - 1]
    by_half = sorted(range(1, n_last), key=lambda k: (abs(2 * k - n_last), k))
    out["many"] = next((g, float(f"{0.01 * h:.4g}"), seed, planes) for planes in by_half for g in (0.15, 0.2, 0.12)
                       for seed in range(seeds) if _holds(shape, "many", (g, float(f"{0.01 * h:.4g}"), seed, planes)))
    return out
