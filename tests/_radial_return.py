"""The small-strain J2 radial return in extended precision, written from the reference's source and from nothing else
(no oracle, no kernel): J2::PlasticStress (materials/materials.hpp:311-391), the hardening laws
(materials/material_hardening.hpp:79-346), P = J sigma F^-T (materials/materials.cpp:60-71).

    eps = sym(F) - I - eps_p,  p = K tr(eps),  s = 2 G dev_dim(eps),  q = sqrt(3/2) |s|
    R(d) = q - 3 G d - H(eqps + d) rate(d / dt) thermo(T)
    yields when R(0) > 0:  d = the root of R in [0, (q - H(eqps) thermo) / 3G]  (R decreases monotonically: one root),
    s <- s (1 - 3 G d / q),  sigma = s + p I,  P = J sigma F^-T
    committed state: eqps + d,  eps_p + d N_p with N_p = 3/2 s / q,  T + chi q d / (rho c)  (temperature-dependent law only)

The root is found by PLAIN BISECTION with mpmath at 50 digits, to 1e-45: no Newton, no tolerance of the reference's solver.
The Johnson-Cook laws jump by B (1e-13)^n ~ 0.03 at |eqps + d| = 1e-13 (material_hardening.hpp:138): a virgin point with
0 < q - A thermo < 0.03 has no root at all, so callers keep |q - H(eqps) thermo| >= 0.1 sigma_y (`margin`, asserted by them).

Derived bound for any double-precision implementation that follows the reference's solver (which stops at |dx| < 1e-10 or
|R| < sigma_y 1e-10): |d - d_exact| <= 1e-10, hence |sigma - sigma_exact|_F <= 2 G sqrt(3/2) 1e-10 (s moves along N_p,
|N_p|_F = sqrt(3/2)) and |P - P_exact|_max <= 2 G sqrt(3/2) 1e-10 |J F^-T|_F: `stress_bar`, with a factor 2 for rounding."""
import mpmath as mp
import numpy as np

from _cases import HARDENING_LAWS, POISSON, YOUNG, thermal_of

DPS = 50
SOLVER_XTOL = 1e-10


def _elastic():
    # MaterialBase::SetYoungPoisson (materials.cpp:7-14), in the doubles the codes under test hold
    K = YOUNG / (3.0 * (1.0 - (2.0 * POISSON)))
    G = YOUNG / (2.0 * (1.0 + POISSON))
    return mp.mpf(K), mp.mpf(G)


class Law:
    def __init__(self, law, **thermal):
        oracle, _, attrs = HARDENING_LAWS[law]
        self.kind = oracle["kind"]
        self.a = {k: mp.mpf(float(v)) for k, v in attrs.items()}
        self.a.setdefault("C", mp.mpf(0))
        self.thermal = {k: mp.mpf(float(v)) for k, v in thermal_of(law, **thermal).items()}
        self.sigma_y = float(attrs["sigma_y"] if "sigma_y" in attrs else attrs["A"])

    def hardening(self, e):
        a = self.a
        if self.kind == "PowerLaw":
            return a["sigma_y"] * (1 + e / a["eps0"]) ** (1 / a["n"])
        if self.kind == "Voce":
            return a["sigma_sat"] - (a["sigma_sat"] - a["sigma_y"]) * mp.exp(-e / a["strain_constant"])
        if abs(e) < mp.mpf("1e-13"):
            return a["A"]
        return a["A"] + a["B"] * e ** a["n"]

    def rate(self, r):
        if self.kind in ("JohnsonCookRate", "JohnsonCookTempRate", "JohnsonCookConstTemp") and r > self.a["eps0_dot"]:
            return 1 + self.a["C"] * mp.log(r / self.a["eps0_dot"])
        return mp.mpf(1)

    def _homologous(self, T):
        Tr, Tm = self.a["reference_temperature"], self.thermal["melting_temperature"]
        return 1 - ((T - Tr) / (Tm - Tr)) ** self.a["m"]

    def thermo(self, T):
        if self.kind == "JohnsonCookTempRate":
            if T < self.a["reference_temperature"]:
                return mp.mpf(1)
            if T > self.thermal["melting_temperature"]:
                return mp.mpf(0)
            return self._homologous(T)
        if self.kind == "JohnsonCookConstTemp":          # SetTemperature(initial), the state's temperature is ignored
            return self._homologous(self.thermal["initial_temperature"])
        return mp.mpf(1)

    def temperature_dependent(self):
        return self.kind == "JohnsonCookTempRate"


class Result:
    pass


def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def radial_return(law, F, dt, plastic_strain=None, eqps=0.0, temperature=None, dF=None, h=None):
    """law: a Law.  F, plastic_strain: [i, J] arrays of doubles (taken exactly); dF, h: evaluate at F + h dF with h an mpf
    (for difference quotients in extended precision).  Returns a Result with doubles rounded from the 50-digit values:
    P, sigma, delta, margin (= q - H(eqps) thermo), plastic, and the committed state eqps / plastic_strain / temperature;
    P_mp is the unrounded stress."""
    with mp.workdps(DPS):
        K, G = _elastic()
        dim = np.asarray(F).shape[0]
        Fm = _mat(F)
        if dF is not None:
            Fm = Fm + h * _mat(dF)
        eye = mp.eye(dim)
        ep = _mat(np.zeros((dim, dim)) if plastic_strain is None else plastic_strain)
        T = law.thermal["initial_temperature"] if temperature is None else mp.mpf(float(temperature))
        e0 = mp.mpf(float(eqps))
        eps = (Fm + Fm.T) / 2 - eye - ep
        tr = sum(eps[i, i] for i in range(dim))
        p = K * tr
        s = 2 * G * (eps - tr / dim * eye)
        q = mp.sqrt(mp.mpf(3) / 2) * mp.sqrt(sum(s[i, j] ** 2 for i in range(dim) for j in range(dim)))
        thermo = law.thermo(T)

        def R(d):
            return q - 3 * G * d - law.hardening(e0 + d) * law.rate(d / mp.mpf(float(dt))) * thermo

        out = Result()
        margin = q - law.hardening(e0) * thermo
        out.margin, out.q = float(margin), float(q)
        out.plastic = margin > 0
        delta = mp.mpf(0)
        if out.plastic:
            lo, hi = mp.mpf(0), margin / (3 * G)
            assert R(lo) > 0 and R(hi) <= mp.mpf("1e-40")      # (thermo = 0: R(hi) is 0 to the working precision)
            while hi - lo > mp.mpf("1e-45"):
                mid = (lo + hi) / 2
                if R(mid) > 0:
                    lo = mid
                else:
                    hi = mid
            delta = (lo + hi) / 2
        Np = s * (mp.mpf(3) / 2 / q) if q > 0 else s
        s_new = s * (1 - 3 * G * delta / q) if out.plastic else s
        sigma = s_new + p * eye
        J = mp.det(Fm)
        P = J * sigma * mp.inverse(Fm).T
        out.P_mp = P
        out.P, out.sigma, out.delta = _np(P), _np(sigma), float(delta)
        out.JFinvT_norm = float(mp.sqrt(sum(v ** 2 for v in (J * mp.inverse(Fm).T))))
        out.eqps = float(e0 + delta)
        out.plastic_strain = _np(ep + delta * Np)
        Tn = T
        if out.plastic and law.temperature_dependent():
            Tn = T + law.thermal["heat_fraction"] * q * delta / (mp.mpf(1) * law.thermal["specific_heat"])   # density 1
        out.temperature = float(Tn)
        return out


def directional_derivative(law, F, dF, dt, plastic_strain=None, eqps=0.0, temperature=None):
    """d/dh P(F + h dF) at h = 0: central difference of the 50-digit stress with its bisected root, h = 1e-15 (truncation
    ~ 1e-30 |P'''|, root error 1e-45 / h): exact to double precision wherever P is smooth in F (away from the yield surface,
    the reference rate and the 1e-13 switch of the Johnson-Cook laws)."""
    with mp.workdps(DPS):
        h = mp.mpf("1e-15")
        a = radial_return(law, F, dt, plastic_strain, eqps, temperature, dF=dF, h=h).P_mp
        b = radial_return(law, F, dt, plastic_strain, eqps, temperature, dF=dF, h=-h).P_mp
        return _np((a - b) / (2 * h))


def stress_bar(JFinvT_norm):
    """2 x 2G sqrt(3/2) 1e-10 |J F^-T|_F, see the module docstring"""
    G = YOUNG / (2.0 * (1.0 + POISSON))
    return 2.0 * 2.0 * G * np.sqrt(1.5) * SOLVER_XTOL * JFinvT_norm


def von_mises(F, plastic_strain=None):
    """q of the elastic predictor, in doubles (for choosing inputs)"""
    F = np.asarray(F, dtype=np.float64)
    dim = F.shape[0]
    G = YOUNG / (2.0 * (1.0 + POISSON))
    eps = 0.5 * (F + F.T) - np.eye(dim) - (0 if plastic_strain is None else plastic_strain)
    s = 2.0 * G * (eps - np.trace(eps) / dim * np.eye(dim))
    return np.sqrt(1.5) * np.linalg.norm(s)
