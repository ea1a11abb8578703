"""J2Simo and J2Log against their 50-digit return maps (tests/_finite_strain_return.py: written from the reference's source
alone, bisection, mpmath's eigsy), without a GPU: the oracle (oracle/ref_path.c through point_pk1 and DomainOracle) AND the
device routines compiled for the host (tests/host_materials.hip), dim 2 and 3, on the named inputs of
tests/_finite_strain_inputs.py -- coincident and nearly coincident principal stretches, and three plastic steps with turning
principal axes.  Until this file both sides were compared with each other only (and with the reference's 2-D golden series):
a reading of the reference that both share -- the order of Fp_inv exp(.), the multiplied cbrt of f_bar, the stress the base
class overwrites -- could not show.

Bars.  Elastic points: P to 1e-12 of max(|P|, G) (absolute on the shear-modulus scale where P = 0), the tangent contracted with
a fixed direction to 1e-10 of max|dP| (the bar of test_materials_host_cpu.py for the dual-number tangents).  Plastic steps:
P within the bar derived in _finite_strain_return.py from the reference solver's stop, grown along the sequence as derived
there; committed eqps / state matrices rtol 1e-9 + 1e-13, temperature 1e-12 (the state bars of the parity tests); the
contracted tangent within FINITE_STRAIN_TANGENT_BAR, measured on the oracle (see its comment).

Measured worst values (the oracle and the host-compiled device code agree to the digits shown unless two are given):
  elastic  J2Log   P 2.8e-15 of max(|P|, G), tangent oracle 1.7e-12 (its difference quotient) / device code 2.2e-15
           J2Simo  P 7.1e-16,                tangent oracle 4.8e-13 / device code 8.4e-16
  plastic  J2Log   P 7.7e-3 of its bar, tangent 2.4e-11, eqps 1.8e-10, Fp_inv 2.7e-12 (relative), T bit-equal
           J2Simo  P 2.8e-3 of its bar, tangent 1.9e-11, eqps 5.9e-11, be 3.1e-12, T 1.8e-15 (relative)
  (the largest values belong to the laws with a rate term, where Newton stops on |dx| < 1e-10 one step earlier)
Nothing here skips or filters a point: margins are assertions on the chosen inputs (in _finite_strain_inputs.py)."""
import ctypes as C

import numpy as np
import pytest

import _finite_strain_inputs as fi
import _finite_strain_return as fs
from _cases import oracle_material, product_material
from test_hardening_laws_cpu import host_point
from test_materials_host_cpu import host_lib, ptr  # noqa: F401  (host_lib: the module-scoped fixture)

MODELS = list(fs.MODELS)
LAWS = fi.PLASTIC_LAWS + ["hot"]


def materials(model, law):
    thermal = fi.HOT_THERMAL if law == "hot" else {}
    return oracle_material(model, law, **thermal), product_material(model, law, **thermal)._c_struct()


def contract(A, dF):
    return np.einsum("iJjL,jL->iJ", A, dF)


def both_sides(host_lib, mo, mp_, dim, c):
    """[(side, P, dP)] at the case's F from the case's state"""
    from oracle import ref_path as rp
    dF = fi.direction(dim)
    Po, Ao = rp.point_pk1(mo, c.F, dt=fi.DT, plastic_strain=c.m1, eqps=c.eqps, temperature=c.T, state2=c.m2)
    Pg, Ag = host_point(host_lib, mp_, dim, fi.DT, c.F, c.m1, c.m2, c.eqps, c.T)
    return [("oracle", Po, contract(Ao, dF)), ("device code", Pg, contract(Ag, dF))]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("model", MODELS)
def test_elastic_spectra_vs_extended_precision(host_lib, model, dim):
    mo, mp_ = materials(model, fi.ELASTIC_LAW)
    G = fs.shear_modulus()
    worst = {}
    for c in fi.elastic_cases(model, dim):
        for side, P, dP in both_sides(host_lib, mo, mp_, dim, c):
            assert np.all(np.isfinite(P)) and np.all(np.isfinite(dP)), (side, c.name)
            err_P = np.abs(P - c.ref.P).max() / max(np.abs(c.ref.P).max(), G)
            err_K = np.abs(dP - c.dP).max() / np.abs(c.dP).max()
            w = worst.setdefault(side, [0.0, 0.0])
            w[0], w[1] = max(w[0], err_P), max(w[1], err_K)
            assert err_P <= 1e-12, (side, c.name, err_P)
            assert err_K <= 1e-10, (side, c.name, err_K)
    print(f"{model} dim {dim}: " + "; ".join(f"{s}: P {w[0]:.2e} (bar 1e-12), tangent {w[1]:.2e} (bar 1e-10)" for s, w in worst.items()))


def state_close(a, b):
    return np.allclose(a, b, rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("law", LAWS)
def test_plastic_sequence_vs_extended_precision(host_lib, law, model, dim):
    """The oracle starts every step from the closed form's committed state (point_pk1 exposes no commit: see
    test_oracle_commits_vs_extended_precision); the host-compiled device code is fed forward with its own."""
    mo, mp_ = materials(model, law)
    cases = fi.plastic_cases(model, law, dim)
    own = None                                        # the device code's own committed (m1, m2, eqps, T)
    worst = dict(P=0.0, K=0.0, eqps=0.0, m1=0.0, T=0.0)
    for k, c in enumerate(cases):
        sides = both_sides(host_lib, mo, mp_, dim, c)
        if own is not None:                           # the device code again, from its own state
            Pg, Ag = host_point(host_lib, mp_, dim, fi.DT, c.F, *own)
            sides.append(("device code, own state", Pg, contract(Ag, fi.direction(dim))))
        for side, P, dP in sides:
            err_P = np.abs(P - c.ref.P).max()
            err_K = np.abs(dP - c.dP).max() / np.abs(c.dP).max()
            worst["P"], worst["K"] = max(worst["P"], err_P / c.bar), max(worst["K"], err_K)
            assert err_P <= c.bar, (side, k, err_P, c.bar)
            assert err_K <= fi.FINITE_STRAIN_TANGENT_BAR, (side, k, err_K)
        m1, m2, eqps, T = own if own is not None else (c.m1, c.m2, c.eqps, c.T)
        a1, a2 = np.ascontiguousarray(m1.T).ravel().copy(), np.ascontiguousarray(m2.T).ravel().copy()
        e, Tc = C.c_double(eqps), C.c_double(T)
        Fc = np.ascontiguousarray(c.F.T).ravel()
        assert host_lib.host_accumulate(C.byref(mp_), dim, C.c_double(fi.DT), ptr(Fc), ptr(a1), ptr(a2), C.byref(e), C.byref(Tc)) == 0
        own = (a1.reshape(dim, dim).T.copy(), a2.reshape(dim, dim).T.copy(), e.value, Tc.value)
        worst["eqps"] = max(worst["eqps"], abs(own[2] - c.ref.eqps) / c.ref.eqps)
        worst["m1"] = max(worst["m1"], np.abs(own[0] - c.ref.m1).max() / np.abs(c.ref.m1).max())
        worst["T"] = max(worst["T"], abs(own[3] - c.ref.temperature) / c.ref.temperature)
        assert state_close(own[2], c.ref.eqps), (k, own[2], c.ref.eqps)
        assert state_close(own[0], c.ref.m1), (k, np.abs(own[0] - c.ref.m1).max())
        if model == "j2simo":
            assert np.array_equal(own[1], c.F)                                  # F_old = F, exactly
        assert np.isclose(own[3], c.ref.temperature, rtol=1e-12, atol=1e-12), (k, own[3], c.ref.temperature)
        if model == "j2log" or law not in ("hot", "JohnsonCookTempRate"):
            assert own[3] == c.T                      # J2Log never touches the temperature; nor does a law that does not depend on it
        else:
            assert own[3] > c.T
    print(f"{model} {law} dim {dim}: P {worst['P']:.2e} of its bar, tangent {worst['K']:.2e} (bar {fi.FINITE_STRAIN_TANGENT_BAR:.1e}), "
          f"eqps {worst['eqps']:.2e}, first state matrix {worst['m1']:.2e}, T {worst['T']:.2e} (relative)")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("law", LAWS)
def test_oracle_commits_vs_extended_precision(law, model, dim):
    """DomainOracle's own commits: DomainPostTimeAdvance at the homogeneous fields of F1, F2, F3 in turn, every quadrature
    point's state against the closed form at the state bars"""
    from oracle import iga, ref_path as rp
    P = iga.Patch.block((2, 2) if dim == 2 else (2, 1, 2), 2, [1.0 + 0.5 * d for d in range(dim)])
    thermal = fi.HOT_THERMAL if law == "hot" else {}
    D = rp.DomainOracle(P, oracle_material(model, law, **thermal))
    D.set_dt(fi.DT)
    T0 = D.temperature.copy()
    for c in fi.plastic_cases(model, law, dim):
        D.domain_post_time_advance((P.ctrl @ (c.F - np.eye(dim)).T).ravel())
        assert state_close(D.eqps, c.ref.eqps)
        assert state_close(D.plastic_strain, c.ref.m1.T.ravel())              # [e, q, i + J dim]
        if model == "j2simo":
            assert state_close(D.state2, c.ref.m2.T.ravel())
        assert np.allclose(D.temperature, c.ref.temperature, rtol=1e-12, atol=1e-12)
    if model == "j2simo" and law in ("hot", "JohnsonCookTempRate"):
        assert D.temperature.min() > T0.max() + 1e-4
    else:
        assert np.array_equal(D.temperature, T0)


def test_tangent_bar_is_what_the_oracle_measures():
    """FINITE_STRAIN_TANGENT_BAR: 10 x the oracle's worst distance from the 50-digit directional derivative over the plastic
    sequences (every law of the GPU tests and `hot`, both models, dim 2 and 3, all three steps), capped at 1e-8 -- measured again here, so
    that the table next to the constant stays true"""
    from oracle import ref_path as rp
    worst = 0.0
    for model in MODELS:
        for dim in (2, 3):
            dF = fi.direction(dim)
            for law in LAWS:
                mo, _ = materials(model, law)
                steps = []
                for c in fi.plastic_cases(model, law, dim):
                    _, Ao = rp.point_pk1(mo, c.F, dt=fi.DT, plastic_strain=c.m1, eqps=c.eqps, temperature=c.T, state2=c.m2)
                    steps.append(np.abs(contract(Ao, dF) - c.dP).max() / np.abs(c.dP).max())
                print(f"{model} dim {dim} {law}: " + " ".join(f"{v:.1e}" for v in steps))
                worst = max(worst, max(steps))
    print(f"oracle tangent against the 50-digit derivative, worst: {worst:.2e}")
    assert 2.0 * worst <= fi.FINITE_STRAIN_TANGENT_BAR <= 1e-8
