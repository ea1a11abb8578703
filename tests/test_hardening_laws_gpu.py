"""Every hardening law on every kernel family, through the C ABI, against the oracle -- modelled on
test_domain_gpu.test_rate_dependent_johnson_cook_parity, with its bars and those of test_residual_and_tangent_parity: committed
eqps / state matrices 1e-9, temperature 1e-12, residual 1e-12, tangent 1e-11 against the oracle's exact tangent.

Before this file every test built the temperature- and rate-dependent Johnson-Cook law at T = T_ref; the power law, Voce, the
plain and the rate-only Johnson-Cook laws and the constant-temperature one ran on no kernel, and thermal softening never
mattered (factor 1 to eight digits).  For those five laws the oracle has no golden series of the reference behind it: what
pins the oracle is tests/test_hardening_laws_cpu.py (extended-precision radial return), what is checked here is that the
same arithmetic survives compilation for the device in each kernel family -- small tensor, degree-2 two-phase, degree-3 with
parked tensors and scalar-register Horner coefficients, general -- in the assembly, residual-only and commit kernels."""
import numpy as np
import pytest

from _cases import HARDENING_LAWS, UNTESTED_LAWS, oracle_material, product_material, synthetic_u, thermal_of

pytestmark = pytest.mark.gpu

# (elements, degree, creator, kernel family the assembly must run on)
SHAPES = [((3, 4), 2, "bspline", "tensor_small"), ((3, 2, 2), 2, "bspline", "tensor_p2_two_phase"),
          ((2, 3, 2), 3, "bspline", "tensor_p3_two_phase"), ((3, 2, 2), 2, "tables", "general")]
SHAPE_IDS = [f"{'x'.join(map(str, s[0]))}p{s[1]}-{s[2]}" for s in SHAPES]
MODELS = ["j2", "j2simo", "j2log"]
RATE_LAWS = ("JohnsonCookRate", "hot", "JohnsonCookConstTemp")


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make_pair(n_el, p, creator, matname, law, **thermal):
    """(patch, oracle integrator, product integrator) with the same law on both sides"""
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    from oracle import iga, ref_path as rp
    P = iga.Patch.block(n_el, p)
    D = rp.DomainOracle(P, oracle_material(matname, law, **thermal), n_threads=2)
    pattern = CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)
    mat = product_material(matname, law, **thermal)
    if creator == "tables":
        tables = dict(dim=P.dim, n_nodes=P.n_nodes, dofs=D.conn, dN_dX=D.dN_dX, weight_det=D.weight * D.det)
        G = NonlinearSolid("domain", mat, pattern, tables=tables).Prepare()
    else:
        G = NonlinearSolid("domain", mat, pattern, patch=mimi_amd.BSplinePatch.block(n_el, p)).Prepare()
    return P, D, G


def compare_state(D, G, matname):
    assert np.allclose(G.State("accumulated_plastic_strain"), D.eqps, rtol=1e-9, atol=1e-13)
    assert np.allclose(G.State("plastic_strain"), D.plastic_strain, rtol=1e-9, atol=1e-13)
    if matname == "j2simo":
        assert np.allclose(G.State("state2"), D.state2, rtol=1e-9, atol=1e-13)
    assert np.allclose(G.State("temperature"), D.temperature, rtol=1e-12, atol=1e-12)


def compare_assembly(P, D, G, u, family):
    """AddDomainResidual and AddDomainResidualAndGrad on both sides; returns the oracle's residual"""
    from oracle import ref_path as rp
    r_o, r_g = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs)
    D.add_domain_residual(u, r_o)
    G.AddDomainResidual(u, r_g)
    assert G.LastKernelFamily() == family
    assert relmax(r_g, r_o) < 1e-12
    r_o, r_g, A_o, A_g = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs), np.zeros(D.nnz), np.zeros(D.nnz)
    D.add_domain_residual_and_grad(u, 0.37, r_o, A_o, rp.TANGENT_EXACT)
    G.AddDomainResidualAndGrad(u, 0.37, r_g, A_g)
    assert G.LastKernelFamily() == family
    assert relmax(r_g, r_o) < 1e-12
    assert relmax(A_g, A_o) < 1e-11
    return r_o


@pytest.mark.parametrize("matname", MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("law", UNTESTED_LAWS)
def test_law_parity_on_every_kernel_family(law, shape, matname):
    n_el, p, creator, family = shape
    P, D, G = make_pair(n_el, p, creator, matname, law)
    dt = 0.05                      # (with eps0_dot = 0.004 the rate term of the rate laws is active; the others ignore it)
    D.set_dt(dt)
    G.dt_ = dt
    T0 = thermal_of(law)["initial_temperature"]
    assert np.all(G.State("temperature") == T0)
    u0 = synthetic_u(P, scale=0.03, seed=7)
    D.domain_post_time_advance(u0)
    G.DomainPostTimeAdvance(u0)
    assert D.eqps.max() > 1e-4
    if law in RATE_LAWS:
        assert D.eqps.max() / dt > 10 * HARDENING_LAWS[law][2]["eps0_dot"]
    compare_state(D, G, matname)
    # none of these laws is temperature-dependent (IsTemperatureDependent() == false): the commit leaves T alone, exactly
    assert np.all(G.State("temperature") == T0) and np.all(D.temperature == T0)
    r_o = compare_assembly(P, D, G, synthetic_u(P, scale=0.02), family)
    if law == "JohnsonCookConstTemp":
        # the constant factor 1 - ((200 - 20) / 1480)^m = 0.9425 is really applied: the same law at T_initial = T_ref differs
        cold = dict(initial_temperature=HARDENING_LAWS[law][2]["reference_temperature"])
        P2, D2, G2 = make_pair(n_el, p, creator, matname, law, **cold)
        D2.set_dt(dt)
        G2.dt_ = dt
        D2.domain_post_time_advance(u0)
        G2.DomainPostTimeAdvance(u0)
        r_c, r_gc = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs)
        D2.add_domain_residual(synthetic_u(P, scale=0.02), r_c)
        G2.AddDomainResidual(synthetic_u(P, scale=0.02), r_gc)
        assert relmax(r_gc, r_c) < 1e-12
        assert relmax(r_c, r_o) > 1e-4 and relmax(r_gc, r_o) > 1e-4


@pytest.mark.parametrize("matname", MODELS)
def test_constant_temperature_at_or_beyond_melting_is_refused(matname):
    """material_hardening.hpp:308-321: SetTemperature throws when 1 - ((T - T_ref) / (T_melt - T_ref))^m <= 0"""
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    patch = mimi_amd.BSplinePatch.block((2, 2), 2)
    pat = CSRPattern.of_bspline_patch(patch)
    for T0 in (1500.0, 1600.0):
        with pytest.raises(RuntimeError, match="Invalid temperature contribution"):
            NonlinearSolid("domain", product_material(matname, "JohnsonCookConstTemp", initial_temperature=T0), pat,
                           patch=patch).Prepare()
    with pytest.raises(RuntimeError, match="can't be bigger than melting temperature"):
        NonlinearSolid("domain", product_material(matname, "hot", melting_temperature=10.0), pat, patch=patch).Prepare()


HOT_SHAPES = [SHAPES[1], SHAPES[2]]
# below the reference temperature (factor 1); at it (base == 0, the special-cased power); homologous temperature 0.5
# (pow_positive at a value that matters: factor 0.61); beyond melting (factor 0: every point yields, the root of the return
# map is the upper end of its bracket)
INITIAL_TEMPERATURES = [10.0, 20.0, 760.0, 1600.0]


@pytest.mark.parametrize("matname", MODELS)
@pytest.mark.parametrize("shape", HOT_SHAPES, ids=SHAPE_IDS[1:3])
@pytest.mark.parametrize("T0", INITIAL_TEMPERATURES)
def test_thermal_softening_over_its_whole_range(T0, shape, matname):
    """The temperature-dependent law (kind 4, rate term active) at an initial temperature where its factor is 1, 1 - 0^m,
    0.61 and 0; specific heat 450 as in the reference's tests, so the commit moves T by ~ 1e-3 K"""
    n_el, p, creator, family = shape
    P, D, G = make_pair(n_el, p, creator, matname, "hot", initial_temperature=T0)
    dt = 0.05
    D.set_dt(dt)
    G.dt_ = dt
    u0 = synthetic_u(P, scale=0.03, seed=7)
    D.domain_post_time_advance(u0)
    G.DomainPostTimeAdvance(u0)
    assert D.eqps.max() > 1e-4
    if T0 > 1500.0:
        assert D.eqps.min() > 0.0                          # melted: every point yields
    compare_state(D, G, matname)
    if matname == "j2log":
        assert np.all(G.State("temperature") == T0)        # J2Log::PlasticStress never updates T (materials.hpp:592-713)
    else:
        assert G.State("temperature").max() > T0
    compare_assembly(P, D, G, synthetic_u(P, scale=0.02), family)


# specific heat of the heating sequence, picked with the oracle on the CPU: with 0.06 the hottest point of the three
# successive commits below goes 760 -> 1003 -> 1791 -> 3273 K (J2, (3,2,2) p2; 1237 -> 2320 -> 5411 on (2,3,2) p3; J2Simo
# within 10 % of that) while the coolest never yields and stays at 760 K
HEATING_SPECIFIC_HEAT = 0.06


@pytest.mark.parametrize("matname", ["j2", "j2simo"])
@pytest.mark.parametrize("shape", HOT_SHAPES, ids=SHAPE_IDS[1:3])
def test_heating_sequence_through_melting(shape, matname):
    """Three commits that heat the hottest points from homologous 0.5 past melting while others stay cold: the factor runs
    over (0.61 ... 0] and the T > T_melt branch inside one mesh; state and assembly after each commit.  (J2Log has no
    heating: see test_thermal_softening_over_its_whole_range.)"""
    n_el, p, creator, family = shape
    P, D, G = make_pair(n_el, p, creator, matname, "hot", initial_temperature=760.0, specific_heat=HEATING_SPECIFIC_HEAT)
    dt = 0.05
    D.set_dt(dt)
    G.dt_ = dt
    for k in range(3):
        u0 = synthetic_u(P, scale=0.03, seed=7 + k)
        D.domain_post_time_advance(u0)
        G.DomainPostTimeAdvance(u0)
        if k == 0:
            assert 900.0 < D.temperature.max() < 1500.0
        compare_state(D, G, matname)
        compare_assembly(P, D, G, synthetic_u(P, scale=0.02, seed=20 + k), family)
    assert D.temperature.min() < 1500.0 < D.temperature.max()
    Tg = G.State("temperature")
    assert Tg.min() < 1500.0 < Tg.max()
