"""Every hardening law the library ships (include/mimi_hip.h mimi_hip_hardening_kind), without a GPU.

(a) The device constitutive routines compiled for the host (tests/host_materials.hip, which calls the library's own
    make_material_dev) against the oracle, point by point, for each law x {J2, J2Simo, J2Log} x dim {2, 3}: the loop and the
    bars of test_materials_host_cpu.test_device_materials_on_host_vs_oracle (stress 1e-12; tangent 1e-11 for J2's closed
    form, 1e-10 for the dual-number tangents), and the committed state against DomainOracle's over two successive commits
    (1e-9 eqps / state matrices, 1e-12 temperature: the bars of test_domain_gpu.test_residual_and_tangent_parity).
(b) The oracle AND the host-compiled device code against the extended-precision radial return of tests/_radial_return.py
    (J2; all six laws and the "hot" parameter set; dim 2 and 3), with the bar derived there.  Only the Johnson-Cook law of
    the reference's own tests (kind 4, C = 0) has golden series of the reference behind the oracle; for the other laws this
    is what pins the oracle.
(c) The Python -> C struct mapping of every hardening class, and the reference's errors for impossible temperatures.

Nothing here skips or filters a point: yield margins and plastic shares are assertions on the chosen inputs."""
import ctypes as C

import numpy as np
import pytest

import _radial_return as rr
from _cases import HARDENING_LAWS, oracle_material, product_material, sigma_y_of, synthetic_u, thermal_of
from test_materials_host_cpu import host_lib, ptr, random_state  # noqa: F401  (host_lib: the module-scoped fixture)

LAWS = list(HARDENING_LAWS)
RATE_LAWS = ("JohnsonCookRate", "hot", "JohnsonCookConstTemp")
# temperatures handed to the temperature-dependent law: below the reference temperature (factor 1), at it (0^m), homologous
# 0.5, beyond melting (factor 0, every point yields, the root is the upper end of the bracket)
HOT_TEMPERATURES = [10.0, 20.0, 760.0, 1600.0]


def temperature_for(law, rng, trial):
    if law != "hot":
        return float(thermal_of(law)["initial_temperature"])
    return HOT_TEMPERATURES[trial % 5] if trial % 5 < 4 else float(rng.uniform(20.0, 1500.0))


def host_point(lib, mp_, dim, dt, F, m1, m2, eqps, T):
    Fc = np.ascontiguousarray(F.T).ravel()
    P, A = np.zeros(dim * dim), np.zeros(dim ** 4)
    a1, a2 = np.ascontiguousarray(m1.T).ravel().copy(), np.ascontiguousarray(m2.T).ravel().copy()
    st = lib.host_point(C.byref(mp_), dim, C.c_double(dt), ptr(Fc), ptr(a1), ptr(a2), C.c_double(eqps), C.c_double(T),
                        ptr(P), ptr(A))
    assert st == 0
    return P.reshape(dim, dim).T, A.reshape(dim, dim, dim, dim)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["j2", "j2simo", "j2log"])
@pytest.mark.parametrize("law", LAWS)
def test_every_law_on_host_vs_oracle(host_lib, law, name, dim):
    from oracle import ref_path as rp
    mo = oracle_material(name, law)
    mp_ = product_material(name, law)._c_struct()
    rng = np.random.default_rng(7 + dim)
    tol_A = 1e-11 if name == "j2" else 1e-10
    dt = 0.05                                   # (rates of 0.02 ... 2 against eps0_dot = 0.004: the rate term is active)
    n_plastic = n_rate = 0
    for trial in range(120):
        scale = 10 ** rng.uniform(-2.5, -0.9)
        F = np.eye(dim) + scale * rng.standard_normal((dim, dim))
        m1, m2, eqps = random_state(name, dim, rng, fresh=trial % 2 == 0)
        T = temperature_for(law, rng, trial)
        Po, Ao = rp.point_pk1(mo, F, dt=dt, plastic_strain=m1, eqps=eqps, temperature=T, state2=m2)
        Pg, Ag = host_point(host_lib, mp_, dim, dt, F, m1, m2, eqps, T)
        assert np.abs(Pg - Po).max() <= 1e-12 * max(np.abs(Po).max(), 1.0), (trial, scale)
        assert np.abs(Ag - Ao).max() <= tol_A * np.abs(Ao).max(), (trial, scale, np.abs(Ag - Ao).max() / np.abs(Ao).max())
        Fc = np.ascontiguousarray(F.T).ravel()
        a1, a2 = np.ascontiguousarray(m1.T).ravel().copy(), np.ascontiguousarray(m2.T).ravel().copy()
        e, Tc = C.c_double(eqps), C.c_double(T)
        assert host_lib.host_accumulate(C.byref(mp_), dim, C.c_double(dt), ptr(Fc), ptr(a1), ptr(a2), C.byref(e), C.byref(Tc)) == 0
        n_plastic += e.value > eqps
        n_rate += (e.value - eqps) / dt > 0.004
        if law != "hot" and law != "JohnsonCookTempRate":
            assert Tc.value == T                # IsTemperatureDependent() == false: the commit leaves the temperature alone
    assert n_plastic > 20                       # the plastic branch was exercised
    if law in RATE_LAWS:
        assert n_rate > 20                      # ... beyond the reference rate


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["j2", "j2simo", "j2log"])
@pytest.mark.parametrize("law", LAWS)
def test_every_law_commit_on_host_vs_domain_oracle(host_lib, law, name, dim):
    """DomainPostTimeAdvance twice (the second from the state the first left): the oracle's committed arrays against
    host_accumulate at every quadrature point, F rebuilt from the oracle's own gradient tables."""
    from oracle import iga, ref_path as rp
    P = iga.Patch.block((2, 2) if dim == 2 else (2, 1, 2), 2)
    thermal = dict(initial_temperature=760.0, specific_heat=0.05) if law == "hot" else {}
    D = rp.DomainOracle(P, oracle_material(name, law, **thermal))
    mp_ = product_material(name, law, **thermal)._c_struct()
    dt = 0.05
    D.set_dt(dt)
    dN, conn = D.tables["dN_dX"], D.conn                                    # [e, q, a, J], [e, a]
    n_plastic = 0
    for step, (scale, seed) in enumerate([(0.03, 7), (0.05, 8)]):
        u = synthetic_u(P, scale=scale, seed=seed).reshape(-1, dim)
        before = [a.copy() for a in (D.plastic_strain, D.state2, D.eqps, D.temperature)]
        D.domain_post_time_advance(u.ravel())
        F = np.eye(dim)[None, None] + np.einsum("eai,eqaj->eqij", u[conn], dN)
        for e in range(F.shape[0]):
            for q in range(F.shape[1]):
                Fc = np.ascontiguousarray(F[e, q].T).ravel()
                a1, a2 = before[0][e, q].copy(), before[1][e, q].copy()
                eq, T = C.c_double(before[2][e, q]), C.c_double(before[3][e, q])
                assert host_lib.host_accumulate(C.byref(mp_), dim, C.c_double(dt), ptr(Fc), ptr(a1), ptr(a2), C.byref(eq),
                                                C.byref(T)) == 0
                assert np.isclose(eq.value, D.eqps[e, q], rtol=1e-9, atol=1e-13)
                assert np.allclose(a1, D.plastic_strain[e, q], rtol=1e-9, atol=1e-13)
                if name == "j2simo":
                    assert np.allclose(a2, D.state2[e, q], rtol=1e-9, atol=1e-13)
                assert np.isclose(T.value, D.temperature[e, q], rtol=1e-12, atol=1e-12)
                n_plastic += eq.value > before[2][e, q]
    assert n_plastic > 20
    T0 = thermal_of(law, **thermal)["initial_temperature"]
    if law in ("hot", "JohnsonCookTempRate") and name != "j2log":
        assert D.temperature.max() > T0 and D.temperature.min() >= T0
    else:
        # IsTemperatureDependent() == false; and J2Log::PlasticStress never touches the temperature (materials.hpp:592-713)
        assert np.all(D.temperature == T0)


def chosen_points(law, dim, n=36):
    """(F, plastic strain, eqps, T) with |q - H(eqps) thermo| >= 0.1 sigma_y: a draw inside the band is pushed outward
    (F - I scaled by 1.3 until it has left it) -- the inputs are chosen, no point is dropped"""
    rng = np.random.default_rng(100 + dim)
    L = rr.Law(law)
    pts = []
    for trial in range(n):
        scale = 10 ** rng.uniform(-2.0, -1.0)
        H = scale * rng.standard_normal((dim, dim))
        ep, _, eqps = random_state("j2", dim, rng, fresh=trial % 2 == 0)
        T = temperature_for(law, rng, trial)
        for _ in range(40):
            m = rr.radial_return(L, np.eye(dim) + H, 0.05, ep, eqps, T).margin
            if abs(m) >= 0.1 * L.sigma_y:
                break
            H *= 1.3
        pts.append((np.eye(dim) + H, ep, eqps, T))
    return L, pts


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("law", LAWS)
def test_j2_return_map_vs_extended_precision(host_lib, law, dim):
    """Oracle and host-compiled device code against the bisected 50-digit radial return (J2).  Bar (derived, not
    measured): 2 x 2G sqrt(3/2) 1e-10 |J F^-T|_F = 5.6e-7 for F ~ I, i.e. the reference solver's own |dx| < 1e-10 stop.
    Measured worst error / bar over the 36 chosen points, dim 2 / dim 3 (oracle and device code agree to the digits shown):
    PowerLaw 4.7e-5 / 4.0e-5, Voce 2.0e-3 / 1.4e-3, JohnsonCook 3.7e-3 / 1.1e-3, JohnsonCookRate 7.5e-2 / 3.7e-2,
    JohnsonCookTempRate 3.7e-3 / 1.1e-3, hot 5.4e-2 / 4.8e-2, JohnsonCookConstTemp 1.0e-1 / 4.1e-2 -- i.e. at most a tenth of
    the bar (5.6e-8 absolute), reached where the rate term makes Newton stop on |dx| < 1e-10 one step earlier."""
    from oracle import ref_path as rp
    L, pts = chosen_points(law, dim)
    mo = oracle_material("j2", law)
    mp_ = product_material("j2", law)._c_struct()
    dt = 0.05
    zero = np.zeros((dim, dim))
    worst = [0.0, 0.0]
    n_plastic = 0
    for F, ep, eqps, T in pts:
        ref = rr.radial_return(L, F, dt, ep, eqps, T)
        assert abs(ref.margin) >= 0.1 * L.sigma_y
        n_plastic += ref.plastic
        bar = rr.stress_bar(ref.JFinvT_norm)
        Po, _ = rp.point_pk1(mo, F, dt=dt, plastic_strain=ep, eqps=eqps, temperature=T, state2=zero)
        Pg, _ = host_point(host_lib, mp_, dim, dt, F, ep, zero, eqps, T)
        for k, Pk in enumerate((Po, Pg)):
            worst[k] = max(worst[k], np.abs(Pk - ref.P).max() / bar)
        assert np.abs(Po - ref.P).max() <= bar, ("oracle", np.abs(Po - ref.P).max(), bar)
        assert np.abs(Pg - ref.P).max() <= bar, ("device code", np.abs(Pg - ref.P).max(), bar)
        # the committed state: eqps + delta, eps_p + delta N_p, T + chi q delta / (rho c) (1e-9: the state bar)
        Fc = np.ascontiguousarray(F.T).ravel()
        a1, a2 = np.ascontiguousarray(ep.T).ravel().copy(), np.zeros(dim * dim)
        e, Tc = C.c_double(eqps), C.c_double(T)
        assert host_lib.host_accumulate(C.byref(mp_), dim, C.c_double(dt), ptr(Fc), ptr(a1), ptr(a2), C.byref(e), C.byref(Tc)) == 0
        # (the same derivation: |d - d_exact| <= 1e-10, |N_p| = sqrt(3/2), dT = chi q d / (rho c); factor 2 for rounding)
        assert abs(e.value - ref.eqps) <= 2e-10
        assert np.abs(a1.reshape(dim, dim).T - ref.plastic_strain).max() <= 2 * np.sqrt(1.5) * 1e-10
        assert abs(Tc.value - ref.temperature) <= 2 * 0.9 * ref.q * 1e-10 / thermal_of(law)["specific_heat"] + 1e-12 * abs(ref.temperature)
    print(f"{law} dim {dim}: worst error / bar: oracle {worst[0]:.2e}, device code {worst[1]:.2e}; {n_plastic} of {len(pts)} plastic")
    assert 3 * n_plastic >= len(pts)


KIND = dict(PowerLaw=0, Voce=1, JohnsonCook=2, JohnsonCookRate=3, JohnsonCookTempRate=4, hot=4, JohnsonCookConstTemp=5)
HARDENING_FIELDS = ("sigma_y", "n", "eps0", "sigma_sat", "strain_constant", "A", "B", "C", "eps0_dot", "reference_temperature", "m")


@pytest.mark.parametrize("name", ["j2", "j2simo", "j2log"])
@pytest.mark.parametrize("law", LAWS)
def test_c_struct_of_every_hardening_class(law, name):
    """J2._c_struct(): the kind of include/mimi_hip.h and exactly the fields the law has -- in particular the Johnson-Cook
    classes, whose sigma_y is a METHOD (py_hardening.cpp), leave m.sigma_y at 0, and PowerLaw's n does not leak into A/B"""
    mat = product_material(name, law)
    m = mat._c_struct()
    attrs = HARDENING_LAWS[law][2]
    assert m.hardening == KIND[law] == mat.hardening._kind
    assert m.kind == dict(j2=1, j2simo=4, j2log=5)[name]
    for f in HARDENING_FIELDS:
        assert getattr(m, f) == float(attrs.get(f, 0.0)), f          # (the table sets every field of a law but kind 4's C = 0)
    if KIND[law] >= 2:
        assert m.sigma_y == 0.0 and callable(mat.hardening.sigma_y) and mat.hardening.sigma_y() == attrs["A"]
    th = thermal_of(law)
    assert (m.heat_fraction, m.specific_heat, m.initial_temperature, m.melting_temperature) == (
        th["heat_fraction"], th["specific_heat"], th["initial_temperature"], th["melting_temperature"])
    assert mat.hardening.is_rate_dependent() == (KIND[law] >= 3)


def make_dev(lib, mat):
    m = mat._c_struct()
    sy, ctc, msg = C.c_double(-1.0), C.c_double(-1.0), C.create_string_buffer(256)
    st = lib.host_make_material(C.byref(m), C.byref(sy), C.byref(ctc), msg, 256)
    return st, sy.value, ctc.value, msg.value.decode()


@pytest.mark.parametrize("name", ["j2", "j2simo", "j2log"])
def test_library_material_setup_of_every_law(host_lib, name):
    """make_material_dev (csrc/common.hpp), the function the library calls: HardeningBase::SigmaY() per law -- it sets the
    yield test and the tolerance of the return-map solve -- and the constant-temperature factor against its formula
    (material_hardening.hpp:308-321) in extended precision"""
    import mpmath
    for law in LAWS:
        st, sy, ctc, msg = make_dev(host_lib, product_material(name, law))
        assert st == 0, msg
        assert sy == sigma_y_of(law) == 70.0
        if law == "JohnsonCookConstTemp":
            with mpmath.workdps(40):
                exact = 1 - (mpmath.mpf(180) / 1480) ** mpmath.mpf(1.3558)
            assert abs(ctc - float(exact)) <= 4e-16 and 0.94 < ctc < 0.945
        else:
            assert ctc == 1.0
    # sigma_y_ref comes from the law's own field: a Voce law with another yield stress, and A set to something else
    mat = product_material(name, "Voce")
    mat.hardening.sigma_y, mat.hardening.A = 55.0, 999.0
    assert make_dev(host_lib, mat)[1] == 55.0
    mat = product_material(name, "JohnsonCook")
    mat.hardening.A = 55.0
    assert make_dev(host_lib, mat)[1] == 55.0


@pytest.mark.parametrize("name", ["j2", "j2simo", "j2log"])
def test_impossible_temperatures_raise_with_the_references_messages(host_lib, name):
    """material_hardening.hpp:238-249 (Validate) and 308-321 (SetTemperature)"""
    for law in ("hot", "JohnsonCookConstTemp"):
        st, _, _, msg = make_dev(host_lib, product_material(name, law, melting_temperature=10.0))
        assert st == 1 and "reference temperature" in msg and "can't be bigger than melting temperature" in msg
    for T0 in (1500.0, 1600.0):      # at melting: contribution 0; beyond: negative
        st, _, _, msg = make_dev(host_lib, product_material(name, "JohnsonCookConstTemp", initial_temperature=T0))
        assert st == 1 and "Invalid temperature contribution" in msg
    st, _, ctc, _ = make_dev(host_lib, product_material(name, "JohnsonCookConstTemp", initial_temperature=1499.0))
    assert st == 0 and 0.0 < ctc < 2e-3
    # the temperature-dependent law takes any initial temperature (its factor is evaluated per point)
    assert make_dev(host_lib, product_material(name, "hot", initial_temperature=1600.0))[0] == 0
    m = product_material(name, "Voce")
    m.hardening = None
    with pytest.raises(RuntimeError, match="hardening missing"):
        m._c_struct()
