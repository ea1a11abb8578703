"""The named inputs of tests/test_finite_strain_cpu.py and tests/test_finite_strain_gpu.py: deformation gradients the
random `I + scale randn` of the other tests never produces, and the closed-form answers to them (tests/_finite_strain_return.py),
computed once per (model, law, dim) and shared.

Elastic spectra (virgin state): F = R U, U = Q diag(lam) Q^T with coincident or nearly coincident principal stretches -- the
paths of the eigen-solver's `apq == 0` skip, of the `x == 0` branch of the logarithm's divided difference and of J2Simo's
|s| ~ 0 normal: identity, a rotation alone, volumetric, uniaxial, equibiaxial, and two families of nearly equal stretches
with gaps from 1e-15 to 1e-3.  Every spectrum comes axis-aligned without rotation (F^T F exactly diagonal), axis-aligned under
the rotation R (off-diagonals of rounding size) and with general principal axes Q under R.
Plastic sequences: three steps far beyond yield whose principal axes differ from step to step, so that J2Log's Fp_inv loses
its symmetry and stops commuting with the next increment; the first step is uniaxial (repeated eigenvalue in the trial
deviator and in the exponential's argument).
All rotations are fixed (Rodrigues' formula on written-out axes and angles); the one random matrix is seeded."""
import functools

import numpy as np

import _finite_strain_return as fs

DT = 0.5                       # as in test_closed_form_gpu.py: the rate term of the rate laws is active
STRETCH = 0.015                # `a`: q <= 0.5 sigma_y for every spectrum (asserted from the 50-digit q)
GAPS = (1e-15, 1e-12, 1e-9, 1e-6, 1e-3)
ELASTIC_LAW = "JohnsonCookTempRate"            # sigma_y = 70; the law does not matter below yield
PLASTIC_LAWS = ["PowerLaw", "Voce", "JohnsonCook", "JohnsonCookRate", "JohnsonCookTempRate", "JohnsonCookConstTemp"]
# the temperature-dependent law with an active rate term at homologous temperature 0.5 (thermal factor 0.61): CPU only
HOT_THERMAL = dict(initial_temperature=760.0)
# Tangent of the plastic branch: it cannot be derived (test_closed_form_gpu.py, at PLASTIC_TANGENT_BAR), so it is MEASURED the
# same way -- on the CPU, on the oracle, never on the code under test: the oracle's tangent contracted with direction(dim)
# against fs.directional_derivative for exactly the F of plastic_inputs, relative to max|dP|, worst of the three steps
# (test_finite_strain_cpu.test_tangent_bar_is_what_the_oracle_measures prints the table step by step):
#              PowerLaw  Voce     JohnsonCook  ...Rate   ...TempRate  ...ConstTemp  hot
#   J2Log  2-D  5.5e-13  1.8e-12  1.8e-12      1.3e-11   1.8e-12      2.4e-11       1.6e-12
#   J2Log  3-D  1.1e-12  2.7e-12  1.1e-12      6.6e-12   1.1e-12      1.7e-11       3.1e-12
#   J2Simo 2-D  2.7e-13  3.4e-13  2.6e-13      2.6e-12   2.6e-13      1.1e-12       9.4e-13
#   J2Simo 3-D  5.1e-13  1.0e-12  6.3e-13      1.9e-11   7.1e-13      1.2e-11       1.0e-11
# The bar is 10 x the worst of those (the cap of 1e-8 is not reached).  The host-compiled device code and the GPU tests use
# the same constant; on the GPU it comes on top of the rounding bar of the moment sum.
FINITE_STRAIN_TANGENT_BAR = 10 * 2.4e-11


def rotation(dim, axis, angle):
    """Rodrigues; in 2-D the axis is ignored"""
    if dim == 2:
        c, s = np.cos(angle), np.sin(angle)
        return np.array([[c, -s], [s, c]])
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def spin(dim):
    """R: a rotation of about 1 rad"""
    return rotation(dim, (1.0, -2.0, 1.5), 1.0)


def axes(dim, k=0):
    """Q: principal axes that are not the coordinate axes; k = 0, 1, 2 give three different ones"""
    return rotation(dim, [(2.0, 1.0, 3.0), (-1.0, 3.0, 1.0), (1.0, 1.0, -2.0)][k], [0.7, 1.9, -1.2][k])


def direction(dim):
    """the fixed dF every tangent is contracted with"""
    return np.random.default_rng(20250117 + dim).standard_normal((dim, dim))


def spectra(dim):
    """[(name, principal stretches)]"""
    a = STRETCH
    if dim == 3:
        out = [("volumetric", (1.07, 1.07, 1.07)), ("uniaxial", (1 + a, 1.0, 1.0)), ("equibiaxial", (1 + a, 1 + a, 1.0))]
        out += [(f"near_uniaxial[{g:g}]", (1 + a, 1 + g, 1.0)) for g in GAPS]
        out += [(f"near_equibiaxial[{g:g}]", (1 + a, (1 + a) * (1 + g), 1.0)) for g in GAPS]
    else:
        out = [("volumetric", (1.07, 1.07)), ("uniaxial", (1 + a, 1.0))]
        out += [(f"near_identity[{g:g}]", (1 + g, 1.0)) for g in GAPS]
        out += [(f"near_volumetric[{g:g}]", (1 + a, (1 + a) * (1 + g))) for g in GAPS]
    return out


def elastic_inputs(dim):
    """[(name, F)]: the identity, R alone, and every spectrum three times (see the module docstring)"""
    R, Q = spin(dim), axes(dim)
    out = [("identity", np.eye(dim)), ("rotation", R)]
    for name, lam in spectra(dim):
        U = np.diag(lam)
        out += [(name + "/aligned", U), (name + "/aligned,rotated", R @ U), (name + "/general,rotated", R @ (Q @ U @ Q.T))]
    return out


def plastic_inputs(dim):
    """[F1, F2, F3]"""
    rng = np.random.default_rng(20250117)
    lam = [(1.12, 1.0, 1.0), (1.15, 1.0, 0.9), (1.15, 1.0, 0.9)]
    Fs = []
    for k in range(3):
        Q = axes(dim, k)
        Fs.append(Q @ np.diag(lam[k][:dim] if dim == 3 else (lam[k][0], lam[k][2])) @ Q.T)
    Fs[2] = Fs[2] @ (np.eye(dim) + 0.1 * rng.standard_normal((dim, dim)))
    return Fs


def law_of(name):
    return fs.Law("hot", **HOT_THERMAL) if name == "hot" else fs.Law(name)


class Case:
    """one input with its closed-form answer: name, F, state before (m1, m2, eqps, T), ref (the Result), dP (the 50-digit
    directional derivative along direction(dim)), bar (the derived stress bar: 0 for an elastic point)"""


@functools.lru_cache(maxsize=None)
def elastic_cases(model, dim):
    law = law_of(ELASTIC_LAW)
    dF = direction(dim)
    m1, m2 = fs.initial_state(model, dim)
    T0 = float(law.thermal["initial_temperature"])
    cases = []
    for name, F in elastic_inputs(dim):
        c = Case()
        c.name, c.F, c.m1, c.m2, c.eqps, c.T = name, F, m1, m2, 0.0, T0
        c.ref = fs.finite_strain_return(model, law, F, DT)
        assert not c.ref.plastic and c.ref.q <= 0.5 * law.sigma_y, (name, c.ref.q)
        c.dP = fs.directional_derivative(model, law, F, dF, DT)
        c.bar = 0.0
        cases.append(c)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def plastic_cases(model, law_name, dim):
    """the three steps, each from the state the closed form committed at the one before; that every step yields, with a margin
    of at least 0.1 sigma_y, is asserted here, on the inputs -- no point is skipped or filtered"""
    law = law_of(law_name)
    dF = direction(dim)
    m1, m2 = fs.initial_state(model, dim)
    eqps, T = 0.0, float(law.thermal["initial_temperature"])
    cases = []
    for k, F in enumerate(plastic_inputs(dim)):
        c = Case()
        c.name, c.F, c.m1, c.m2, c.eqps, c.T = f"step {k + 1}", F, m1, m2, eqps, T
        c.ref = fs.finite_strain_return(model, law, F, DT, m1, m2, eqps, T)
        assert c.ref.plastic and c.ref.margin >= 0.1 * law.sigma_y, (law_name, k, c.ref.margin)
        c.dP = fs.directional_derivative(model, law, F, dF, DT, m1, m2, eqps, T)
        cases.append(c)
        c.bar = fs.sequence_bar(model, [x.ref for x in cases])
        m1, m2, eqps, T = c.ref.m1, c.ref.m2, c.ref.eqps, c.ref.temperature
    if model == "j2log":
        assert np.abs(m1 - m1.T).max() > 1e-3                  # Fp_inv has lost its symmetry by step 3
        assert T == float(law.thermal["initial_temperature"])
    elif law.temperature_dependent():
        assert T > float(law.thermal["initial_temperature"]) + 1e-4
    return tuple(cases)

