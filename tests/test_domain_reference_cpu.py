"""The long-double reference of the domain integrator (tests/_domain_reference.py) checked against independent answers, the
inputs of tests/test_domain_reference_gpu.py vetted on the reference alone, and the oracle (oracle/ref_path.c, oracle/harness.py)
pinned to the reference on every case of tests/_domain_cases.py -- 3-D, degree 2, StVK, J2Linear, the viscosity and the mass
form for the first time against something its author did not write twice.  No GPU.

  1. neo-Hookean and StVK: P and dP : dF against the first and second central differences of the ENERGIES
     W = mu/2 (tr C - dim) - mu ln J + lambda/2 (J - 1)^2 and W = lambda/2 tr(E)^2 + mu E:E in mpmath at 50 digits (no stress
     formula of the repository is in them), 20 deformation gradients per law and dimension, bar 1e-15 relative.
  2. J2: P, the committed state and dP : dF against tests/_radial_return.py (50-digit bisection, 50-digit central difference)
     at 16 points per (case, law) drawn from the actual inhomogeneous inputs, 8 at the commit and 8 in the assembly from the
     committed state, elastic and plastic both present; bar 1e-13 relative.  J2Linear against test_closed_form_gpu.py::pk1
     from the virgin state and against a 50-digit restatement of box 7.5 at points with a back stress.
  2b. J2Log and J2Simo: the long-double Jacobi eigen-solver on its own (identity, coincident pairs and triples, pairs 1e-9 and
     1e-17 apart, rotated axes, 2 x 2 and 3 x 3: |A Q - Q lam|, |Q^T Q - I|, exp(log A) = A within 1e-17 of the largest entry),
     and P, the committed state, dP : dF and delta against tests/_finite_strain_return.py (50-digit eigsy, bisection and central
     difference) at 24 points per (case, material, step) of the actual inhomogeneous inputs -- the smallest |margin|, the
     largest carry, the smallest and largest eigenvalue gap, elastic points, plastic points that were virgin and that were
     not, a seeded fill -- both sides given the same doubles; bars 1e-15 (P, state), 1e-14 (dP) of the largest entry at the
     sample, 1e-17 absolute (delta).
  3. the conditions of _domain_cases.conditions on every (case, material), and the plastic shares written next to the seeds.
  4. the oracle against the reference: residual and K v (random, smooth, single-node v) of the hyperelastic laws and J2Linear
     within MARGIN (1/8) of the project's bars 1e-12 / 1e-11; J2 residual row by row within MARGIN of the derived bar
     (_domain_cases.residual_bar), committed state within the derived 2 x SOLVER_XTOL bars, state through the (element, point)
     layout; the three linear forms within MARGIN of 1e-13; the J2 tangent measured into _domain_cases.J2_TANGENT_MEASURED.
     J2Log and J2Simo the same way (the [elastic] variants at the plain MARGIN x 1e-12 / 1e-11), their second step on
     _domain_cases.SECOND_PAIRS, the element boxes, and the tangent measured into FINITE_TANGENT_MEASURED.

Measured (x86-64, worst over the cases; -s prints every case):
  reference     against the energies P 6.6e-19, dP 2.5e-18; J2 against the 50-digit map P, dP <= 1e-20 (equal doubles almost
                everywhere), eqps 2.1e-16, plastic strain 1.7e-16; J2Linear 6.0e-16 against pk1 (a double-precision closed
                form), <= 1e-18 against the 50-digit box 7.5
  oracle        neo-Hookean residual 2.2e-15, K v 8.9e-15; StVK 2.9e-15, 1.8e-13 (its tangent is the least accurate, still 1/7
                of MARGIN x 1e-11); J2Linear 1.1e-15, 2.1e-15, state 4.9e-3 of its bar; J2 residual 2.6e-11 relative = 1.2e-2 of
                the derived row bar, state 0.41 of its bar (eqps 8.2e-11, where the reference's own solver stops), tangent
                3.1e-9 (Johnson-Cook laws) and 8.0e-13 (PowerLaw): _domain_cases.J2_TANGENT_MEASURED
  linear forms  body force 6.9e-16, mass 1.3e-15, viscosity 4.0e-15 (bar MARGIN x 1e-13)
  finite strain eigen-solver: residual 4.9e-19, orthogonality 6.0e-19, exp(log A) 1.2e-18; against the 50-digit maps P <= 2.0e-16,
                dP <= 8.4e-17, state <= 2.2e-16 (one ulp of the doubles the 50-digit side returns), delta <= 8.7e-19; oracle:
                residual <= 1.9e-2 of the row bar, state <= 0.39 of its bar (second commit <= 0.08), the [elastic] variants
                residual <= 4.2e-14 and K v <= 2.5e-13, tangent 7.3e-9 (j2log), 4.4e-10 (j2simo), <= 1.0e-12 (PowerLaw)
The finite-strain additions take about 50 s of the module's 105 s (35 s of them the 50-digit samples)."""
import functools

import mpmath as mp
import numpy as np
import pytest
import scipy.sparse as sp

import _domain_cases as dc
import _domain_reference as dr
import _radial_return as rr
from _domain_cases import MARGIN

LD = np.longdouble


def f64(a):
    return np.asarray(a, dtype=np.float64)


def relmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max() / max(np.abs(f64(b)).max(), 1e-300))


# ---- 1. the hyperelastic laws against their energies -----------------------------------------------------------------------
def energy(name, F):
    lam, mu = [mp.mpf(float(x)) for x in dr.constants()[:2]]
    dim = F.rows
    C = F.T * F
    if name == "neohook":
        J = mp.det(F)
        return mu / 2 * (sum(C[i, i] for i in range(dim)) - dim) - mu * mp.log(J) + lam / 2 * (J - 1) ** 2
    E = (C - mp.eye(dim)) / 2
    return lam / 2 * sum(E[i, i] for i in range(dim)) ** 2 + mu * sum(E[i, j] ** 2 for i in range(dim) for j in range(dim))


def energy_derivatives(name, F, dF):
    """(dW/dF, d/dt dW/dF (F + t dF)) by central differences at 50 digits, step 1e-12: truncation 1e-24, rounding 1e-26"""
    dim = F.shape[0]
    with mp.workdps(50):
        h = mp.mpf("1e-12")
        Fm, dFm = rr._mat(F), rr._mat(dF)

        def first(G):
            out = mp.zeros(dim, dim)
            for i in range(dim):
                for j in range(dim):
                    E = mp.zeros(dim, dim)
                    E[i, j] = h
                    out[i, j] = (energy(name, G + E) - energy(name, G - E)) / (2 * h)
            return out

        return rr._np(first(Fm)), rr._np((first(Fm + h * dFm) - first(Fm - h * dFm)) / (2 * h))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["neohook", "stvk"])
def test_hyperelastic_laws_are_the_derivatives_of_their_energies(name, dim):
    rng = np.random.default_rng(100 + dim)
    F = np.eye(dim) + 0.15 * rng.standard_normal((20, dim, dim))
    dF = rng.standard_normal((20, dim, dim))
    assert np.linalg.det(F).min() > 0.25
    pt = dr.point_law(dr.material(name), F, dFs=[dF])
    worst_P = worst_dP = 0.0
    for k in range(len(F)):
        P, dP = energy_derivatives(name, F[k], dF[k])
        worst_P = max(worst_P, relmax(pt.P[k], P))
        worst_dP = max(worst_dP, relmax(pt.dP[0][k], dP))
    print(f"{name} dim {dim}: P {worst_P:.2e}, dP {worst_dP:.2e} against the energy's derivatives")
    assert worst_P <= 1e-15 and worst_dP <= 1e-15


# ---- 2. the J2 point laws against the 50-digit return map --------------------------------------------------------------------
J2_PAIRS = [(c, m) for c, m in dc.PAIRS if dc.is_j2(m)]


def sample(plastic, n, rng):
    """n point indices, half plastic and half elastic as far as there are such points"""
    yes, no = np.nonzero(plastic)[0], np.nonzero(~plastic)[0]
    k = min(n // 2, len(yes))
    k = max(k, n - len(no))
    return np.concatenate([rng.choice(yes, k, replace=False), rng.choice(no, n - k, replace=False)])


@pytest.mark.parametrize("case,matname", J2_PAIRS, ids=lambda v: v)
def test_j2_point_law_against_the_50_digit_return_map(case, matname):
    ref = dc.reference(case, matname)
    law = rr.Law(dc.law_of(matname) or "JohnsonCookTempRate")
    geo, dim = ref.geo, ref.geo.sp.dim
    rng = np.random.default_rng(17)
    n_pts = geo.sp.n_points
    worst = dict(P=0.0, dP=0.0, eqps=0.0, ep=0.0, T=0.0)
    seen = set()
    for u, state, plastic in ((ref.u0, None, ref.commit.plastic), (ref.u, ref.state, ref.asm.pt.plastic)):
        idx = sample(np.asarray(plastic), min(8, n_pts), rng)
        # the inputs of both sides: F and the state rounded to doubles
        F = f64(dr.deformation_gradient(geo, u)[idx])
        dF = rng.standard_normal(F.shape)
        st = dr.virgin_state(ref.mat, len(idx), dim) if state is None else dr.take(state, idx)
        st.eqps, st.plastic_strain, st.temperature = (f64(x).astype(LD) for x in (st.eqps, st.plastic_strain, st.temperature))
        pt = dr.point_law(ref.mat, F, st, dc.DT, [dF])
        for k in range(len(idx)):
            args = (f64(st.plastic_strain[k]), float(st.eqps[k]), float(st.temperature[k]))
            exact = rr.radial_return(law, F[k], dc.DT, *args)
            dP = rr.directional_derivative(law, F[k], dF[k], dc.DT, *args)
            assert exact.plastic == bool(pt.plastic[k])
            seen.add(exact.plastic)
            worst["P"] = max(worst["P"], relmax(pt.P[k], exact.P))
            worst["dP"] = max(worst["dP"], relmax(pt.dP[0][k], dP))
            worst["eqps"] = max(worst["eqps"], abs(float(pt.new.eqps[k]) - exact.eqps) / max(exact.eqps, 1e-300))
            worst["ep"] = max(worst["ep"], relmax(pt.new.plastic_strain[k], exact.plastic_strain) if exact.eqps > 0 else 0.0)
            worst["T"] = max(worst["T"], abs(float(pt.new.temperature[k]) - exact.temperature) / exact.temperature)
    print(f"{case} {matname}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert seen == {True, False}
    assert max(worst.values()) <= 1e-13


def j2linear_mp(F, ep, beta, eqps, dF=None, h=None):
    """J2Linear::PlasticStress (materials.hpp:187-236) at 50 digits: (P, eqps, plastic strain, beta) after the step"""
    K, G = rr._elastic()
    h_iso, h_kin, sigma_y = mp.mpf(40), mp.mpf(25), mp.mpf(70)
    dim = np.asarray(F).shape[0]
    Fm = rr._mat(F) if dF is None else rr._mat(F) + h * rr._mat(dF)
    I = mp.eye(dim)
    ep, beta, e0 = rr._mat(ep), rr._mat(beta), mp.mpf(float(eqps))
    eps = (Fm + Fm.T) / 2 - I - ep
    t = sum(eps[i, i] for i in range(dim))
    s = 2 * G * (eps - t / dim * I)
    eta = s - beta
    norm = mp.sqrt(sum(v ** 2 for v in eta))
    phi = mp.sqrt(mp.mpf(3) / 2) * norm - (sigma_y + h_iso * e0)
    if phi > 0:
        inc = phi / (3 * G + h_kin + h_iso)
        n = eta / norm
        s = s - mp.sqrt(6) * G * inc * n
        e0, ep, beta = e0 + inc, ep + mp.sqrt(mp.mpf(3) / 2) * inc * n, beta + mp.sqrt(mp.mpf(2) / 3) * h_kin * inc * n
    P = mp.det(Fm) * (s + K * t * I) * mp.inverse(Fm).T
    return P, e0, ep, beta, phi > 0


@pytest.mark.parametrize("case", [c for c, m in dc.PAIRS if m == "j2linear"])
def test_j2linear_point_law(case):
    import test_closed_form_gpu as cf
    ref = dc.reference(case, "j2linear")
    geo, dim = ref.geo, ref.geo.sp.dim
    rng = np.random.default_rng(23)
    # from the virgin state: the closed forms of test_closed_form_gpu.py::pk1
    idx = sample(np.asarray(ref.commit.plastic), 16, rng)
    F = f64(dr.deformation_gradient(geo, ref.u0)[idx])
    pt = dr.point_law(ref.mat, F, None, dc.DT)
    worst = 0.0
    for k in range(len(idx)):
        kind = "j2linear_plastic" if pt.plastic[k] else "j2linear"
        assert (cf.von_mises(F[k]) > 70.0) == bool(pt.plastic[k])
        worst = max(worst, relmax(pt.P[k], cf.pk1(kind, F[k])))
    # from the committed state (back stress at the points that yielded at the commit): box 7.5 restated at 50 digits
    idx = sample(np.asarray(ref.asm.pt.plastic), 16, rng)
    F = f64(dr.deformation_gradient(geo, ref.u)[idx])
    dF = rng.standard_normal(F.shape)
    st = dr.take(ref.state, idx)
    st.eqps, st.plastic_strain, st.beta = (f64(x).astype(LD) for x in (st.eqps, st.plastic_strain, st.beta))
    assert (np.abs(f64(st.beta)).reshape(len(idx), -1).max(axis=1) > 0.1).sum() >= 8      # points that do carry a back stress
    pt = dr.point_law(ref.mat, F, st, dc.DT, [dF])
    worst2 = dict(P=0.0, dP=0.0, state=0.0)
    with mp.workdps(50):
        h = mp.mpf("1e-15")
        for k in range(len(idx)):
            args = (f64(st.plastic_strain[k]), f64(st.beta[k]), float(st.eqps[k]))
            P, e1, ep1, b1, plastic = j2linear_mp(F[k], *args)
            assert bool(plastic) == bool(pt.plastic[k])
            dP = (j2linear_mp(F[k], *args, dF=dF[k], h=h)[0] - j2linear_mp(F[k], *args, dF=dF[k], h=-h)[0]) / (2 * h)
            worst2["P"] = max(worst2["P"], relmax(pt.P[k], rr._np(P)))
            worst2["dP"] = max(worst2["dP"], relmax(pt.dP[0][k], rr._np(dP)))
            worst2["state"] = max(worst2["state"], abs(float(pt.new.eqps[k]) - float(e1)) / max(float(e1), 1e-300),
                                  relmax(pt.new.plastic_strain[k], rr._np(ep1)), relmax(pt.new.beta[k], rr._np(b1)))
    print(f"{case} j2linear: virgin P {worst:.2e}; with back stress " + ", ".join(f"{k} {v:.2e}" for k, v in worst2.items()))
    assert worst <= 1e-13 and max(worst2.values()) <= 1e-13


# ---- 2b. the eigen-solver and the finite-strain point laws ---------------------------------------------------------------------
def _rotations(dim):
    import _finite_strain_inputs as fi
    return [np.eye(dim), fi.spin(dim), fi.axes(dim), fi.axes(dim, 1) @ fi.spin(dim)]


def eigen_inputs(dim):
    """symmetric matrices Q diag(lam) Q^T (formed in long double from doubles): the identity, exactly coincident pairs and
    triples, pairs that differ by 1e-9 and by 1e-17, well separated spectra; on the coordinate axes and on rotated ones"""
    spectra = {3: [(1, 1, 1), (2.5, 2.5, 2.5), (1.3, 1.3, 0.7), (0.7, 1.3, 1.3), (1.3, 0.7, 1.3), (1 + 1e-9, 1, 0.8), (1, 1 + 1e-9, 1 - 1e-9),
                   (LD(1) + LD(1e-17), 1, 0.8), (LD(1) + LD(1e-17), 1, LD(1) - LD(1e-17)), (1.21, 0.95, 0.83), (3.0, 1e-2, 0.5)],
               2: [(1, 1), (2.5, 2.5), (1 + 1e-9, 1), (LD(1) + LD(1e-17), 1), (1.21, 0.83), (3.0, 1e-2)]}[dim]
    out = []
    for lam in spectra:
        for Q in _rotations(dim):
            Q = np.asarray(Q, dtype=LD)
            out.append(np.einsum("ia,a,ja->ij", Q, np.array(lam, dtype=LD), Q))
    return np.stack(out)


@pytest.mark.parametrize("dim", [2, 3])
def test_eigen_solver_on_its_own(dim):
    A = eigen_inputs(dim)
    A = (A + dr.T(A)) / 2
    lam, Q = dr.sym_eig(A)
    size = np.abs(A).max(axis=(1, 2))
    fig = dict(residual=(np.abs(dr.mm(A, Q) - Q * lam[:, None, :]).max(axis=(1, 2)) / size).max(),
               orthogonality=np.abs(dr.mm(dr.T(Q), Q) - dr.eye(dim)).max(),
               exp_log=(np.abs(dr.sym_fun(dr.sym_fun(A, np.log), np.exp) - A).max(axis=(1, 2)) / size).max(),
               half_log=(np.abs(dr.sym_fun(2 * dr.sym_fun(A, lambda x: np.log(x) / 2), np.exp) - A).max(axis=(1, 2)) / size).max())
    print(f"dim {dim}, {len(A)} matrices: " + ", ".join(f"{k} {float(v):.2e}" for k, v in fig.items()))
    assert lam.min() > 0
    assert max(fig.values()) <= 1e-17


def finite_sample(ref, pt, state_before, earlier, n, rng):
    """at most n point indices of a step: the smallest |margin|, the largest carry, the smallest and the largest gap between
    eigenvalues (of C_e | the trial be), an elastic point, a plastic point that was virgin and one that was not (where there
    are such), and a seeded random fill"""
    plastic = np.asarray(pt.plastic)
    virgin = np.asarray(state_before.eqps == 0)
    lam = np.sort(f64(pt.spectrum), axis=1)
    gap = np.diff(lam, axis=1).min(axis=1)
    carried = dc.carry(ref.matname, pt, earlier) if earlier is not None else f64(pt.cond if hasattr(pt, "cond") else pt.fbar2)
    picks = [int(np.abs(f64(pt.margin)).argmin()), int(carried.argmax()), int(gap.argmin()), int(gap.argmax())]
    for mask in (~plastic, plastic & virgin, plastic & ~virgin):
        if mask.any():
            picks.append(int(np.nonzero(mask)[0][0]))
    picks = list(dict.fromkeys(picks))
    rest = rng.permutation(np.setdiff1d(np.arange(len(plastic)), picks))
    return np.array(picks + list(rest[:max(0, n - len(picks))])), plastic, virgin


FINITE_SAMPLE = 24          # points per (case, material, step)


@pytest.mark.parametrize("case,matname", dc.FINITE_PAIRS, ids=lambda v: v)
def test_finite_strain_point_laws_against_the_50_digit_maps(case, matname):
    import _finite_strain_return as fs
    ref = dc.reference(case, matname)
    model, law = dc.model_of(matname), fs.Law(dc.law_of(matname) or "JohnsonCookTempRate")
    geo, dim = ref.geo, ref.geo.sp.dim
    rng = np.random.default_rng(29)
    steps = [(ref.u0, ref.state_before["commit"], ref.commit, None), (ref.u, ref.state, ref.asm.pt, ref.commit)]
    if ref.second:
        steps.append((ref.second.u, ref.second.state, ref.second.asm.pt, ref.second.commit))
    worst = dict(P=0.0, dP=0.0, state=0.0, delta=0.0)
    kinds = set()
    for u, before, full, earlier in steps:
        idx, plastic, virgin = finite_sample(ref, full, before, earlier, FINITE_SAMPLE, rng)
        kinds |= {(bool(plastic[i]), bool(virgin[i])) for i in idx}
        # both sides see the same numbers: F and the state rounded to doubles
        F = f64(dr.deformation_gradient(geo, u)[idx])
        dF = rng.standard_normal(F.shape)
        st = dr.take(before, idx)
        for k, v in vars(st).items():
            setattr(st, k, f64(v).astype(LD))
        pt = dr.point_law(ref.mat, F, st, dc.DT, [dF])
        exact, exact_dP = [], []
        for k in range(len(idx)):
            args = (f64(dc.first_matrix(matname, st)[k]), f64(st.F_old[k]) if model == "j2simo" else None, float(st.eqps[k]), float(st.temperature[k]))
            exact.append(fs.finite_strain_return(model, law, F[k], dc.DT, *args))
            exact_dP.append(fs.directional_derivative(model, law, F[k], dF[k], dc.DT, *args))
            assert exact[-1].plastic == bool(pt.plastic[k])
        stack = lambda name: np.stack([np.asarray(getattr(e, name)) for e in exact])
        worst["P"] = max(worst["P"], relmax(pt.P, stack("P")))
        worst["dP"] = max(worst["dP"], relmax(pt.dP[0], np.stack(exact_dP)))
        worst["delta"] = max(worst["delta"], float(np.abs(f64(pt.delta) - stack("delta")).max()))
        state = [(pt.new.eqps, stack("eqps")), (pt.new.temperature, stack("temperature")), (dc.first_matrix(matname, pt.new), stack("m1"))]
        if model == "j2simo":
            state.append((pt.new.F_old, stack("m2")))
        worst["state"] = max([worst["state"]] + [relmax(a, b) for a, b in state if np.abs(b).max() > 0])
        assert all(np.abs(f64(a)).max() == 0 for a, b in state if np.abs(b).max() == 0)
    print(f"{case} {matname}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if dc.is_elastic(matname):
        assert kinds == {(False, True)}
    else:
        assert {(False, True), (True, True), (True, False)} <= kinds
    assert worst["P"] <= 1e-15 and worst["state"] <= 1e-15 and worst["dP"] <= 1e-14 and worst["delta"] <= 1e-17


def test_seeds_are_recorded_with_their_plastic_shares():
    """the comments of _domain_cases.SEEDS on the finite-strain pairs are what the reference gives"""
    import re
    text = open(dc.__file__).read()
    seen = 0
    for case, matname, figures in re.findall(r'\("(\w+)", "(j2(?:log|simo)[^"]*)"\): \([\d, ]+\),\s+# plastic ([\d. /]+)', text):
        ref = dc.reference(case, matname)
        shares = [ref.commit.plastic.mean(), ref.asm.pt.plastic.mean()] + ([ref.second.asm.pt.plastic.mean()] if ref.second else [])
        assert [f"{float(x):.2f}" for x in shares] == figures.strip().split(" / "), (case, matname, shares)
        seen += 1
    assert seen == len([k for k in dc.SEEDS if dc.is_finite(k[1])]) == 10


# ---- 3. the conditions on the inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,matname", dc.PAIRS + dc.WALK_PAIRS, ids=lambda v: v)
def test_inputs_satisfy_the_conditions(case, matname):
    ref = dc.reference(case, matname)
    bad, fig = dc.conditions(ref)
    print(f"{case} {matname}: {ref.geo.sp.n_points} points, " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert ref.geo.sp.n_points <= 3100
    assert not bad, bad


def test_every_family_has_every_material_class():
    for family in dc.EXTRA:
        cases = [c for c, v in dc.CASES.items() if v["family"] == family]
        for m in dc.BASE_MATERIALS + dc.EXTRA_MATERIALS:
            assert any((c, m) in dc.PAIRS for c in cases), (family, m)
        for m in dc.FINITE_MODELS:
            assert any((c, m) in dc.PAIRS and (c, m + "[elastic]") in dc.PAIRS for c in cases), (family, m)


def test_layout_and_boxes_by_parameter_range():
    """the (element, point) layout of a box is the layout of the whole patch restricted to the elements of the box"""
    sp_ = dc.geometry(dc.BOX_CASE).sp
    whole = dr.layout(sp_)
    m = sp_.n_spans
    e = np.arange(int(np.prod(m)))
    ez = e // (m[0] * m[1])
    total = np.zeros(sp_.n_points, dtype=int)
    for begin, end in dc.BOXES:
        own = np.nonzero((ez >= begin[2]) & (ez < end[2]))[0]
        assert np.array_equal(dr.layout(sp_, begin, end), whole[own])
        mask = dr.in_box(sp_, begin, end)
        assert np.array_equal(np.sort(whole[own].ravel()), np.nonzero(mask)[0])
        total += mask
    assert np.all(total == 1)


# ---- 4. the oracle against the reference ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(case, matname):
    from oracle import ref_path as rp
    ref = dc.reference(case, matname)
    P = dc.oracle_patch(case)
    D = rp.DomainOracle(P, dc.oracle_material(matname), quadrature_order=dc.arrays(case).order, n_threads=2)
    D.set_dt(dc.DT)
    if D.has_states:
        D.domain_post_time_advance(ref.u0)
    r0, r, A = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs), np.zeros(D.nnz)
    D.add_domain_residual(ref.u, r0)
    D.add_domain_residual_and_grad(ref.u, dc.GRAD_FACTOR, r, A, rp.TANGENT_EXACT)
    K = sp.csr_matrix((A / dc.GRAD_FACTOR, D.col, D.rowptr), shape=(P.n_vdofs, P.n_vdofs))
    return P, D, r0, r, [K @ v for v in ref.vectors]


def oracle_state(D):
    return dict(accumulated_plastic_strain=D.eqps, plastic_strain=D.plastic_strain, temperature=D.temperature, state2=D.state2).get


@pytest.mark.parametrize("case,matname", dc.PAIRS + dc.WALK_PAIRS, ids=lambda v: v)
def test_oracle_against_the_reference(case, matname):
    ref = dc.reference(case, matname)
    P, D, r0, r, Kv = oracle_run(case, matname)
    rowptr, col, conn = dc.pattern(case)
    assert np.array_equal(rowptr, D.rowptr) and np.array_equal(col, D.col) and np.array_equal(conn, D.conn)
    fig = {}
    if D.has_states:
        grid = dr.layout(ref.geo.sp)
        fig["state/bar"] = dc.compare_state(ref, oracle_state(D), grid, f"{case} {matname}")
    bar = dc.residual_bar(ref)
    want = f64(ref.asm.r)
    fig["residual"] = relmax(r, want)
    fig["residual/bar"] = max(float((np.abs(x - want) / bar).max()) for x in (r0, r))
    fig["Kv"] = max(relmax(a, b) for a, b in zip(Kv, ref.asm.Kv))
    print(f"{case} {matname}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["residual/bar"] <= MARGIN
    if dc.has_solver(matname) and not dc.is_elastic(matname):
        assert fig["Kv"] <= dc.tangent_bar(matname)
    else:
        assert fig["Kv"] <= MARGIN * dc.TANGENT_BAR


@pytest.mark.parametrize("case,matname", dc.SECOND_PAIRS, ids=lambda v: v)
def test_oracle_second_step_against_the_reference(case, matname):
    """the second step of _domain_cases.SECOND_PAIRS on a fresh oracle: commit at u0, commit at u, the state, then the
    assemblies at u2 -- the tangent figure of this step enters _domain_cases.FINITE_TANGENT_MEASURED"""
    fig = oracle_second_step(case, matname)
    print(f"{case} {matname} second step: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["state/bar"] <= 1.0 and fig["residual/bar"] <= MARGIN and fig["Kv"] <= dc.tangent_bar(matname)


@functools.lru_cache(maxsize=None)
def oracle_second_step(case, matname):
    from oracle import ref_path as rp
    ref = dc.reference(case, matname)
    P = dc.oracle_patch(case)
    D = rp.DomainOracle(P, dc.oracle_material(matname), quadrature_order=dc.arrays(case).order, n_threads=2)
    D.set_dt(dc.DT)
    D.domain_post_time_advance(ref.u0)
    D.domain_post_time_advance(ref.u)
    fig = {"state/bar": dc.compare_state(ref, oracle_state(D), dr.layout(ref.geo.sp), f"{case} {matname} second commit", step=2)}
    r0, r, A = np.zeros(P.n_vdofs), np.zeros(P.n_vdofs), np.zeros(D.nnz)
    D.add_domain_residual(ref.second.u, r0)
    D.add_domain_residual_and_grad(ref.second.u, dc.GRAD_FACTOR, r, A, rp.TANGENT_EXACT)
    K = sp.csr_matrix((A / dc.GRAD_FACTOR, D.col, D.rowptr), shape=(P.n_vdofs, P.n_vdofs))
    bar, want = dc.residual_bar(ref, step=2), f64(ref.second.asm.r)
    fig["residual/bar"] = max(float((np.abs(x - want) / bar).max()) for x in (r0, r))
    fig["Kv"] = max(relmax(K @ v, b) for v, b in zip(ref.vectors, ref.second.asm.Kv))
    return fig


def test_finite_tangent_table():
    """the measurement behind _domain_cases.FINITE_TANGENT_MEASURED, by the protocol of test_j2_tangent_table: worst over the
    cases (and the second step where there is one) per (model, law)"""
    worst = {}
    for case, matname in dc.FINITE_PAIRS:
        if dc.is_elastic(matname):
            continue
        ref = dc.reference(case, matname)
        err = max(relmax(a, b) for a, b in zip(oracle_run(case, matname)[4], ref.asm.Kv))
        second = oracle_second_step(case, matname)["Kv"] if ref.second else 0.0
        print(f"  {case} {matname}: {err:.2e}" + (f", second step {second:.2e}" if ref.second else ""))
        worst[matname] = max(worst.get(matname, 0.0), err, second)
    print("FINITE_TANGENT_MEASURED = {" + ", ".join(f'"{k}": {v:.1e}' for k, v in worst.items()) + "}")
    assert set(worst) == set(dc.FINITE_TANGENT_MEASURED)
    for k, v in worst.items():
        assert v <= 1.5 * dc.FINITE_TANGENT_MEASURED[k], (k, v)
    assert dc.FINITE_TANGENT_BAR == {k: min(1e-8, 10 * v) for k, v in dc.FINITE_TANGENT_MEASURED.items()}


def test_j2_tangent_table():
    """the measurement behind _domain_cases.J2_TANGENT_MEASURED: the oracle's exact tangent times the three probe vectors
    against the reference's K v, worst over the cases, per law -- the table holds these figures"""
    worst = {}
    for case, matname in J2_PAIRS:
        ref = dc.reference(case, matname)
        Kv = oracle_run(case, matname)[4]
        err = max(relmax(a, b) for a, b in zip(Kv, ref.asm.Kv))
        print(f"  {case} {matname}: {err:.2e}")
        worst[matname] = max(worst.get(matname, 0.0), err)
    print("J2_TANGENT_MEASURED = {" + ", ".join(f'"{k}": {v:.1e}' for k, v in worst.items()) + "}")
    assert set(worst) == set(dc.J2_TANGENT_MEASURED)
    for k, v in worst.items():
        assert v <= 1.5 * dc.J2_TANGENT_MEASURED[k], (k, v)           # (the table is what a run prints, to rounding noise)
    assert dc.J2_TANGENT_BAR == {k: min(1e-8, 10 * v) for k, v in dc.J2_TANGENT_MEASURED.items()}


def test_oracle_on_element_boxes():
    from oracle import ref_path as rp
    case = dc.BOX_CASE
    for matname in ("neohook", "j2", "j2log", "j2simo"):
        ref = dc.reference(case, matname)
        P = dc.oracle_patch(case)
        ez = P.element_multi_index()[2]
        for begin, end in dc.BOXES:
            own = np.nonzero((ez >= begin[2]) & (ez < end[2]))[0]
            D = rp.DomainOracle(P, dc.oracle_material(matname), n_threads=2, elements=own)
            D.set_dt(dc.DT)
            if D.has_states:
                D.domain_post_time_advance(ref.u0)
                dc.compare_state(ref, oracle_state(D), dr.layout(ref.geo.sp, begin, end), f"{case} box {begin}")
            r = np.zeros(P.n_vdofs)
            D.add_domain_residual(ref.u, r)
            mask = dr.in_box(ref.geo.sp, begin, end)
            want = f64(dr.nodal(ref.geo, ref.asm.pt.P, mask))
            assert (np.abs(r - want) / dc.residual_bar(ref, mask)).max() <= MARGIN


def test_oracle_on_the_walk_boxes():
    """the boxes of tests/test_wgsym_walk_gpu.py, cut in x: they partition the points by parameter range, and the oracle on the
    elements of each agrees with the reference restricted to it"""
    from oracle import ref_path as rp
    case, matname = dc.WALK_BOX_CASE, dc.WALK_MATERIAL
    ref = dc.reference(case, matname)
    P = dc.oracle_patch(case)
    ex = P.element_multi_index()[0]
    total = np.zeros(ref.geo.sp.n_points, dtype=int)
    for (begin, end), _ in dc.WALK_BOXES:
        own = np.nonzero((ex >= begin[0]) & (ex < end[0]))[0]
        assert len(own) == int(np.prod(np.array(end) - np.array(begin)))
        D = rp.DomainOracle(P, dc.oracle_material(matname), n_threads=2, elements=own)
        D.set_dt(dc.DT)
        r = np.zeros(P.n_vdofs)
        D.add_domain_residual(ref.u, r)
        mask = dr.in_box(ref.geo.sp, begin, end)
        total += mask
        want = f64(dr.nodal(ref.geo, ref.asm.pt.P, mask))
        assert (np.abs(r - want) / dc.residual_bar(ref, mask)).max() <= MARGIN
    assert np.all(total == 1)


def test_the_walk_cases_are_what_the_walks_need():
    """the shapes the walks of tests/test_wgsym_walk_gpu.py are written for: element counts, columns with tables of their own
    on walk335_p2, rational weights on walk542_p2"""
    for case, n_el, seg_len, walks in dc.WALKS:
        a = dc.arrays(case)
        assert tuple(n - 2 for n in a.n_ctrl) == n_el and a.degrees == (2, 2, 2) and a.family == "tensor_p2_two_phase"
        assert n_el[2] % seg_len == 0
        units = n_el[0] * n_el[1] * (n_el[2] // seg_len)
        for value, cols, tail in walks:
            assert cols == min(4, units // value) > 1
            assert tail == units - (-(-units // cols) - 1) * cols
    a = dc.arrays("walk335_p2")
    for k in a.knots:
        spans = np.diff(np.unique(k))
        assert len(set(np.round(spans, 12))) == len(spans)          # no two spans of an axis alike
    assert dc.arrays("walk542_p2").weights is not None and np.ptp(dc.arrays("walk542_p2").weights) > 0.1
    assert dc.arrays("walk761_p2").weights is None


@pytest.mark.parametrize("case", dc.FORMS_CASES)
def test_oracle_linear_forms_against_the_reference(case):
    from oracle import harness as hz
    P, D = oracle_run(case, "neohook")[:2]
    geo = dc.geometry(case)
    n = P.n_vdofs
    b = dc.B3[:P.dim]
    M = sp.csr_matrix((hz.assemble_mass(P, D.tables, dc.RHO, D.rowptr, D.col), D.col, D.rowptr), shape=(n, n))
    C = sp.csr_matrix((hz.assemble_viscosity(P, D.tables, dc.NU, D.rowptr, D.col), D.col, D.rowptr), shape=(n, n))
    fig = dict(body=relmax(hz.assemble_body_force(P, D.tables, b), dr.body_force(geo, b)), mass=0.0, viscosity=0.0)
    for v in dc.probes(case):
        fig["mass"] = max(fig["mass"], relmax(M @ v, dr.mass_times(geo, dc.RHO, v)))
        fig["viscosity"] = max(fig["viscosity"], relmax(C @ v, dr.diffusion_times(geo, dc.NU, v)))
    print(f"{case}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert max(fig.values()) <= MARGIN * dc.FORMS_BAR


@pytest.mark.parametrize("case", [c for c in dc.CASES if dc.CASES[c].get("flat")])
def test_flat_tables_of_the_reference_against_the_oracle(case):
    """the tables the flat-table handles of tests/test_domain_reference_gpu.py are created from (the reference's, rounded to
    double, in the (element, point) layout) against the oracle's own"""
    D = oracle_run(case, "neohook")[1]
    t = dc.flat_tables(case)
    assert np.array_equal(t["dofs"], D.conn)
    fig = dict(dN_dX=relmax(D.dN_dX, t["dN_dX"]), weight_det=relmax(D.weight * D.det, t["weight_det"]), N=relmax(D.tables["N"], t["N"]))
    print(f"{case}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert max(fig.values()) <= 1e-13
