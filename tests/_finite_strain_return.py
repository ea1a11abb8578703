"""The two finite-strain J2 models in extended precision, written from the reference's source and from nothing else (no
oracle import, no product import): J2Log::PlasticStress (materials/materials.hpp:636-735) with LogarithmicStrain
(materials/material_utils.hpp:91-114) under MaterialBase::EvaluatePK1 (materials/materials.cpp:60-71), and
J2Simo::PlasticStress (materials/materials.hpp:455-564); Dev / Norm / AlmostZero (material_utils.hpp:14-57, 116-127); the
initial states (materials/materials.cpp:184-203 be_old = F_old = I, :221-241 Fp_inv = I); the hardening laws of tests/_radial_return.py.

J2Log    F_e = F Fp_inv,  E_e = 1/2 log(F_e^T F_e),  p = K tr E_e,  s = 2 G dev_dim(E_e),  q = sqrt(3/2) |s|
         R(d) = q - 3 G d - H(eqps + d) rate(d / dt) thermo(T);  yields when R(0) > 0, d = the root in [0, (q - H(eqps) thermo) / 3G]
         N_p = 3/2 s / q,  s <- s - 2 G d N_p;   commit: Fp_inv <- Fp_inv exp(-d N_p), eqps += d  (the temperature is never touched)
         P = det F (s + p / det F I) F^-T: PlasticStress leaves M = s + p / det F I in alternative_stress_ and its own
         F_e^-T M F_e^T F^-T in stress_; the base class then takes alternative_stress_ as the Cauchy stress and overwrites stress_.
J2Simo   f_bar = (F_old F^-1)^-1,  f_bar <- f_bar cbrt(det f_bar)  (multiplied, as written at materials.hpp:486)
         be = f_bar be_old f_bar^T,  s = G dev_dim(be),  N_p = sqrt(3/2) s / |s|  (sqrt(1/2) I when |s| < DBL_EPSILON),  s_eff = N_p : s
         R(d) = s_eff - G d tr(be) - H(eqps + d) thermo(T) rate(d / dt);  d = the root in [0, (s_eff - H(eqps) thermo) / (G tr be)]
         be <- be - 2/3 d tr(be) N_p,  s = G dev_dim(be);   commit: eqps += d, T += chi s_eff d / (rho c) (temperature-dependent
         law only); then, yielding or not, F_old = F, be_old = be
         P = (s + K/2 (det F^2 - 1) I) F^-T

Symmetric matrix functions go through mpmath's eigsy at 50 digits; the root is found by PLAIN BISECTION to 1e-45 on the
reference's own bracket (R decreases monotonically): no Newton, no tolerance of the reference's solver.  Callers keep the
yield margin away from 0 (the Johnson-Cook jump at 1e-13, see _radial_return.py) and assert it.

Derived bounds for a double-precision implementation that follows the reference's solver, which stops at |dx| < 1e-10 (or
|R| < sigma_y 1e-10), i.e. |d - d_exact| <= 1e-10 (`stress_bar`, with the factor 2 for rounding of _radial_return.py):
  J2Log   s moves along N_p (|N_p|_F = sqrt(3/2)) by 2 G 1e-10:  |P - P_exact|_max <= 2 G sqrt(3/2) 1e-10 |det F F^-T|_F, the J2 bar.
  J2Simo  be moves by 2/3 tr(be) N_p 1e-10, s = G dev(be) by G 2/3 tr(be) sqrt(3/2) 1e-10, and P = tau F^-T:
          |P - P_exact|_max <= G 2/3 tr(be) sqrt(3/2) 1e-10 |F^-T|_F.
Step k of a sequence, each step from the state the implementation itself committed: every earlier step left a state that is
off by its own 1e-10, and that reaches the trial stress of step k through the finite-strain kinematics with a factor
(`Result.carry`, computed here at 50 digits) where the small-strain model has 1:
  J2Log   Fp_inv (1 + X), |X|_F <= sqrt(3/2) 1e-10, gives F_e (1 + X), dC_e = X^T C_e + C_e X, |dC_e|_F <= 2 lam_max |X|_F, and
          the derivative of 1/2 log at C_e is bounded by 1 / (2 lam_min) (its divided differences are):  |dE_e|_F <= cond(C_e) |X|_F.
          carry = cond(C_e) = lam_max / lam_min of the trial C_e of step k  (1 for coaxial steps, as in the small-strain model).
  J2Simo  be_old + D, |D|_F <= 2/3 tr(be) sqrt(3/2) 1e-10, gives be + f_bar D f_bar^T:  carry = |f_bar|_2^2 tr(be of the step
          that left D) / tr(be of step k), at least 1;  F_old is committed exactly.
The radial return does not expand a perturbation of the trial stress (the component along N_p shrinks by H' / (3G + H'), the
rest by q_new / q), and the shift of eqps by 1e-10 moves the final stress by H' 1e-10 << 2 G 1e-10.  So the bar of step k is
`sequence_bar` = stress_bar(step k) x (1 + sum of carry over the earlier steps) -- k times the one-step bar where carry is 1,
which is how test_closed_form_gpu.test_j2_beyond_yield_two_steps reasons."""
import mpmath as mp
import numpy as np

from _cases import POISSON, YOUNG
from _radial_return import DPS, SOLVER_XTOL, Law, Result, _elastic, _mat, _np  # noqa: F401  (Law: for the callers)

MODELS = ("j2log", "j2simo")
DBL_EPSILON = 2.220446049250313e-16             # std::numeric_limits<double>::epsilon() of AlmostZero (material_utils.hpp:14-17)


def initial_state(model, dim):
    """(first state matrix, second state matrix): J2Log Fp_inv = I (and nothing); J2Simo be_old = I, F_old = I"""
    return np.eye(dim), (np.eye(dim) if model == "j2simo" else np.zeros((dim, dim)))


def _sym_fun(A, f):
    """Q diag(f(lam)) Q^T of the symmetric A (mfem::DenseMatrix::CalcEigenvalues + MultADAt in the reference)"""
    lam, Q = mp.eigsy((A + A.T) / 2)
    n = A.rows
    return Q * mp.diag([f(lam[i]) for i in range(n)]) * Q.T, [lam[i] for i in range(n)]


def _dev(A, dim, factor):
    tr = sum(A[i, i] for i in range(dim))
    return (A - tr / dim * mp.eye(dim)) * factor


def _norm(A):
    return mp.sqrt(sum(v ** 2 for v in A))


def _bisect(R, hi):
    lo = mp.mpf(0)
    assert R(lo) > 0 and R(hi) <= mp.mpf("1e-40")          # (thermo = 0: R(hi) is 0 to the working precision)
    while hi - lo > mp.mpf("1e-45"):
        mid = (lo + hi) / 2
        if R(mid) > 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def finite_strain_return(model, law, F, dt, m1=None, m2=None, eqps=0.0, temperature=None, dF=None, h=None):
    """model: 'j2log' | 'j2simo'.  law: a Law.  F, m1, m2: [i, J] arrays of doubles, taken exactly (m1: Fp_inv | be_old, m2:
    F_old of J2Simo; None: the initial state); dF, h: evaluate at F + h dF with h an mpf.  Returns a Result with doubles
    rounded from the 50-digit values: P, delta, q (the trial q | s_eff), margin (= R(0): q net of the hardening at eqps),
    plastic, the committed state m1 / m2 / eqps / temperature, stress_bar and carry (module docstring); P_mp is unrounded."""
    with mp.workdps(DPS):
        K, G = _elastic()
        dim = np.asarray(F).shape[0]
        Fm = _mat(F)
        if dF is not None:
            Fm = Fm + h * _mat(dF)
        eye = mp.eye(dim)
        i1, i2 = initial_state(model, dim)
        M1 = _mat(i1 if m1 is None else m1)
        M2 = _mat(i2 if m2 is None else m2)
        T = law.thermal["initial_temperature"] if temperature is None else mp.mpf(float(temperature))
        e0 = mp.mpf(float(eqps))
        thermo = law.thermo(T)
        J = mp.det(Fm)
        FinvT = mp.inverse(Fm).T
        out = Result()
        tenth = mp.mpf(SOLVER_XTOL)
        if model == "j2log":
            F_e = Fm * M1
            E_e, lam = _sym_fun(F_e.T * F_e, lambda x: mp.log(x) / 2)
            p = K * sum(E_e[i, i] for i in range(dim))
            s = _dev(E_e, dim, 2 * G)
            q = mp.sqrt(mp.mpf(3) / 2) * _norm(s)
            slope = 3 * G
            carry = max(lam) / min(lam)
        else:
            f_bar = mp.inverse(M2 * mp.inverse(Fm))
            f_bar = f_bar * mp.cbrt(mp.det(f_bar))
            be = f_bar * M1 * f_bar.T
            s = _dev(be, dim, G)
            s_norm = _norm(s)
            if abs(s_norm) < mp.mpf(DBL_EPSILON):
                N_p = mp.sqrt(mp.mpf(1) / 2) * eye
            else:
                N_p = s * (mp.sqrt(mp.mpf(3) / 2) / s_norm)
            q = sum(N_p[i, j] * s[i, j] for i in range(dim) for j in range(dim))          # s_effective
            be_trace = sum(be[i, i] for i in range(dim))
            slope = G * be_trace
            _, lam = _sym_fun(f_bar.T * f_bar, lambda x: x)
            carry = max(lam)                                 # |f_bar|_2^2; the callers weigh it with the traces
            out.be_trace = float(be_trace)

        def R(d):
            return q - slope * d - law.hardening(e0 + d) * law.rate(d / mp.mpf(float(dt))) * thermo

        margin = q - law.hardening(e0) * thermo
        out.margin, out.q = float(margin), float(q)
        out.plastic = margin > 0
        delta = _bisect(R, margin / slope) if out.plastic else mp.mpf(0)
        Tn = T
        if model == "j2log":
            new1, new2 = M1, M2
            if out.plastic:
                N_p = s * (mp.mpf(3) / 2 / q)
                s = s - 2 * G * delta * N_p
                ex, _ = _sym_fun(-delta * N_p, mp.exp)
                new1 = M1 * ex
            P = J * (s + p / J * eye) * FinvT
            bar = 2 * G * mp.sqrt(mp.mpf(3) / 2) * tenth * _norm(J * FinvT)
        else:
            if out.plastic:
                be = be - mp.mpf(2) / 3 * delta * be_trace * N_p
                s = _dev(be, dim, G)
                if law.temperature_dependent():
                    Tn = T + law.thermal["heat_fraction"] * q * delta / (mp.mpf(1) * law.thermal["specific_heat"])   # density 1
            P = (s + K * (J * J - 1) / 2 * eye) * FinvT
            new1, new2 = be, Fm
            bar = G * mp.mpf(2) / 3 * be_trace * mp.sqrt(mp.mpf(3) / 2) * tenth * _norm(FinvT)
        out.P_mp = P
        out.P, out.delta = _np(P), float(delta)
        out.m1, out.m2 = _np(new1), _np(new2)
        out.eqps, out.temperature = float(e0 + delta), float(Tn)
        out.stress_bar = 2.0 * float(bar)
        out.carry = float(carry)
        return out


def directional_derivative(model, law, F, dF, dt, m1=None, m2=None, eqps=0.0, temperature=None):
    """d/dh P(F + h dF) at h = 0: central difference of the 50-digit stress with its bisected root, h = 1e-15 (truncation
    ~ 1e-30 |P'''|, root error 1e-45 / h): exact to double precision wherever P is smooth in F -- P is (matrix logarithm and
    all) also where principal stretches coincide; not at the yield surface, the reference rate and the 1e-13 switch of the
    Johnson-Cook laws."""
    with mp.workdps(DPS):
        h = mp.mpf("1e-15")
        a = finite_strain_return(model, law, F, dt, m1, m2, eqps, temperature, dF=dF, h=h).P_mp
        b = finite_strain_return(model, law, F, dt, m1, m2, eqps, temperature, dF=dF, h=-h).P_mp
        return _np((a - b) / (2 * h))


def sequence_bar(model, steps):
    """The derived stress bar of the last of `steps` (Results of successive steps, each from the state the one before
    committed): its own stress_bar x (1 + the earlier steps' errors carried into it), see the module docstring"""
    last = steps[-1]
    if model == "j2log":
        carried = last.carry * (len(steps) - 1)
    else:
        carried = sum(max(1.0, last.carry * s.be_trace / last.be_trace) for s in steps[:-1])
    return last.stress_bar * (1.0 + carried)


def shear_modulus():
    return YOUNG / (2.0 * (1.0 + POISSON))
