"""Shared problem definitions for the tests (inputs follow the reference's own tests:
tests/test_nonlinear_solid.py:6-81 in j042/mimi; synthetic blocks follow SURVEY 8d)."""
import numpy as np

JC_TEST = dict(kind="JohnsonCookTempRate", A=70, B=140, n=0.2835, m=1.3558, eps0_dot=0.004,
               reference_temperature=20)


# Every hardening law the library ships (include/mimi_hip.h mimi_hip_hardening_kind; material_hardening.hpp:79-346):
# name -> (hardening dict of oracle.ref_path.make_material, product class name, attributes set on the product object).
# Only "JohnsonCookTempRate" (= JC_TEST, the reference's own test parameters) has golden series of the reference behind the
# oracle; the others are pinned by tests/test_hardening_laws_cpu.py against an extended-precision radial return.
_JC = dict(A=70, B=140, n=0.2835)
_JC_RATE = dict(_JC, C=0.04, eps0_dot=0.004)
_JC_TEMP = dict(_JC_RATE, reference_temperature=20, m=1.3558)


def _law(kind, cls, attrs):
    return dict(attrs, kind=kind), cls, dict(attrs)


HARDENING_LAWS = {
    "PowerLaw": _law("PowerLaw", "PowerLawHardening", dict(sigma_y=70, n=4, eps0=0.01)),
    "Voce": _law("Voce", "VoceHardening", dict(sigma_y=70, sigma_sat=150, strain_constant=0.05)),
    "JohnsonCook": _law("JohnsonCook", "JohnsonCookHardening", _JC),
    "JohnsonCookRate": _law("JohnsonCookRate", "JohnsonCookRateDependentHardening", _JC_RATE),
    "JohnsonCookTempRate": (JC_TEST, "JohnsonCookTemperatureAndRateDependentHardening",
                            {k: v for k, v in JC_TEST.items() if k != "kind"}),
    # the temperature-dependent law with an active rate term, for the tests that move the temperature over its whole range
    "hot": _law("JohnsonCookTempRate", "JohnsonCookTemperatureAndRateDependentHardening", _JC_TEMP),
    "JohnsonCookConstTemp": _law("JohnsonCookConstTemp", "JohnsonCookConstantTemperatureHardening", _JC_TEMP),
}
# the laws no test built before tests/test_hardening_laws_*.py
UNTESTED_LAWS = ["PowerLaw", "Voce", "JohnsonCook", "JohnsonCookRate", "JohnsonCookConstTemp"]
THERMAL = dict(heat_fraction=0.9, specific_heat=450, initial_temperature=20, melting_temperature=1500)
# thermal settings that belong to a law: the constant-temperature law's factor is 1 - ((200 - 20) / 1480)^m = 0.9425
LAW_THERMAL = {"JohnsonCookConstTemp": dict(initial_temperature=200)}
YOUNG, POISSON = 2100, 0.3


def thermal_of(law, **thermal):
    return {**THERMAL, **LAW_THERMAL.get(law, {}), **thermal}


def sigma_y_of(law):
    """HardeningBase::SigmaY()"""
    attrs = HARDENING_LAWS[law][2]
    return attrs["sigma_y"] if "sigma_y" in attrs else attrs["A"]


def oracle_material(name, law=None, **thermal):
    from oracle import ref_path as rp
    if name == "neohook":
        return rp.make_material("neohookean", 2100, 0.3, density=1.0)
    if name == "stvk":
        return rp.make_material("stvk", 2100, 0.3, density=1.0)
    if name == "j2linear":
        return rp.make_material("j2linear", 2100, 0.3, density=1.0, isotropic_hardening=40.0, kinematic_hardening=25.0,
                                sigma_y=70.0)
    kind = {"j2": "j2", "j2simo": "j2simo", "j2log": "j2log"}[name]
    if law is not None or thermal:
        law = law or "JohnsonCookTempRate"
        return rp.make_material(kind, 2100, 0.3, density=1.0, hardening=HARDENING_LAWS[law][0], **thermal_of(law, **thermal))
    return rp.make_material(kind, 2100, 0.3, density=1.0, hardening=JC_TEST, heat_fraction=0.9,
                            specific_heat=450, initial_temperature=20, melting_temperature=1500)


def product_material(name, law=None, **thermal):
    import mimi_amd
    if name == "neohook":
        m = mimi_amd.CompressibleOgdenNeoHookean()
        m.density = 1.0
        m.set_young_poisson(2100, 0.3)
        return m
    if name == "stvk":
        m = mimi_amd.StVenantKirchhoff()
        m.density = 1.0
        m.set_young_poisson(2100, 0.3)
        return m
    if name == "j2linear":
        m = mimi_amd.J2Linear()
        m.density = 1.0
        m.set_young_poisson(2100, 0.3)
        m.isotropic_hardening, m.kinematic_hardening, m.sigma_y = 40.0, 25.0, 70.0
        return m
    m = {"j2": mimi_amd.J2, "j2simo": mimi_amd.J2Simo, "j2log": mimi_amd.J2Log}[name]()
    m.density = 1.0
    m.set_young_poisson(2100, 0.3)
    if law is not None or thermal:
        law = law or "JohnsonCookTempRate"
        for k, v in thermal_of(law, **thermal).items():
            setattr(m, k, v)
        h = getattr(mimi_amd, HARDENING_LAWS[law][1])()
        for k, v in HARDENING_LAWS[law][2].items():
            setattr(h, k, v)
        m.hardening = h
        return m
    m.heat_fraction, m.specific_heat = 0.9, 450
    m.initial_temperature, m.melting_temperature = 20, 1500
    h = mimi_amd.JohnsonCookTemperatureAndRateDependentHardening()
    for k, v in JC_TEST.items():
        if k != "kind":
            setattr(h, k, v)
    m.hardening = h
    return m


def synthetic_u(patch, scale=0.05, seed=20241008, clamp_axis=0):
    """u = scale*h*N(0,1), Dirichlet face x=0 zeroed (h = 1 for unit cells)."""
    rng = np.random.default_rng(seed)
    u = scale * rng.standard_normal(patch.n_vdofs)
    nodes = patch.boundary_nodes(clamp_axis, 0)
    u.reshape(-1, patch.dim)[nodes] = 0.0
    return u


def balken_oracle(matname, tangent_mode=0, n_threads=1):
    """2-D 5x1 beam, p=3, 2x2 elements (balken.mesh + elevate_degrees(2) + subdivide(1))."""
    from oracle import iga, ref_path as rp, harness as hz
    P = iga.Patch.block((2, 2), 3, [5.0, 1.0])
    D = rp.DomainOracle(P, oracle_material(matname), n_threads=n_threads)
    force, dt = (-5.0, 0.05) if matname == "neohook" else (-3.0, 0.5)
    mass = hz.assemble_mass(P, D.tables, 1.0, D.rowptr, D.col)
    rhs = hz.assemble_body_force(P, D.tables, [0.0, force])
    nodes = P.boundary_nodes(0, 0)
    dirichlet = np.sort(np.concatenate([nodes * 2, nodes * 2 + 1]))
    op = hz.Operator(D, D.rowptr, D.col, mass, rhs, dirichlet)
    op.tangent_mode = tangent_mode
    ode = hz.GeneralizedAlpha2(op, 0.5, dict(rel_tol=1e-12, abs_tol=1e-8, max_iter=10, iterative_mode=False))
    return P, D, op, ode, dt
