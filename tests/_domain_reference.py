"""What the domain integrator (csrc/kernels_tensor_*.hpp, tensor_p3.hip, kernels_general.hpp, kernels_forms.hpp) sums over a
patch, in numpy long double -- written from the definitions, from plain arrays (degrees, knot vectors, control points, NURBS
weights, displacement, quadrature order, material constants), sharing neither code nor scheme with the oracle,
mimi_amd.splines or the kernels.  Only the Cox-de Boor basis and the polished Gauss rule of tests/_face_reference.py are
imported (they are independent already).

    points       the tensor grid of the per-span Gauss rules (order // 2 + 1 points per direction and span, order =
                 2 max(degrees) + 3 by default), first direction fastest, carried as dense N[q, A], dN[q, d, A] over ALL nodes
                 of the patch (A = A0 + n0 (A1 + n1 A2)): no span index, no element connectivity.  Every point carries its
                 parameter coordinates xi[q, d], so a sum is restricted to an element box by parameter range alone
                 (`in_box`) and the product's (element, point) state layout is mapped onto the grid from the coordinates
                 (`layout`: element e = e0 + m0 (e1 + m1 e2), point q = q0 + nq (q1 + nq q2), include/mimi_hip.h).
    rational     R_A = w_A N_A / W, W = sum_B w_B N_B;  dR_A / dxi_d = w_A (dN_A W - N_A dW) / W^2  (quotient rule).
    geometry     dX/dxi = sum_A X_A (x) dR_A/dxi, its determinant (asserted positive) and inverse by explicit cofactors
                 (numpy.linalg has no long double); dN_A/dX_J = sum_d dR_A/dxi_d dxi_d/dX_J.
    point laws   from the reference's source lines, as tests/test_closed_form_gpu.py cites them:
                   neohook   P = mu (F - F^-T) + lambda J (J - 1) F^-T                      (materials.cpp:96-118, 60-71)
                   stvk      E = (F^T F - I) / 2, S = lambda tr(E) I + 2 mu E, P = F S        (materials.cpp:73-94)
                   j2        eps = sym(F) - I - eps_p, p = K tr eps, s = 2 G dev_dim eps, q = sqrt(3/2) |s|,
                             R(d) = q - 3 G d - H(eqps + d) rate(d / dt) thermo(T); beyond yield (R(0) > 0) d = the root of
                             R in [0, (q - H(eqps) thermo) / 3G] by PLAIN BISECTION (100 halvings, vectorised over the
                             points: the bracket is below long-double resolution long before), s <- s - 2 G d N_p,
                             N_p = 3/2 s / q, P = J (s + p I) F^-T; committed eqps + d, eps_p + d N_p,
                             T + chi q d / (rho c) for the temperature-dependent law  (materials.hpp:311-391); every
                             hardening law of _cases.HARDENING_LAWS with its rate and thermal factor
                             (material_hardening.hpp:79-346)
                   j2linear  eta = s - beta, q = sqrt(3/2) |eta|, phi = q - (sigma_y + H_iso eqps); beyond yield
                             inc = phi / (3 G + H_kin + H_iso), s <- s - sqrt(6) G inc eta / |eta|; committed eqps + inc,
                             eps_p + sqrt(3/2) inc eta / |eta|, beta + sqrt(2/3) H_kin inc eta / |eta|
                             (materials.hpp:187-236)
                   j2log     F_e = F Fp_inv, E_e = 1/2 log(F_e^T F_e) (through `sym_eig`), p = K tr E_e, s = 2 G dev_dim E_e,
                             q = sqrt(3/2) |s|, the scalar equation, root and radial return of j2, P = det F (s + p / det F I)
                             F^-T; committed eqps + d, Fp_inv exp(-d N_p), the temperature untouched
                             (materials.hpp:636-735, material_utils.hpp:91-114, materials.cpp:60-71, 221-241)
                   j2simo    f_bar = (F_old F^-1)^-1 cbrt(det .) (multiplied, as written), be = f_bar be_old f_bar^T,
                             s = G dev_dim be, N_p = sqrt(3/2) s / |s| (sqrt(1/2) I where |s| < DBL_EPSILON), s_eff = N_p : s,
                             R(d) = s_eff - G tr(be) d - H(eqps + d) rate(d / dt) thermo(T), the root in
                             [0, (s_eff - H(eqps) thermo) / (G tr be)] by the same bisection, be <- be - 2/3 d tr(be) N_p,
                             P = (G dev_dim be + K/2 (det F^2 - 1) I) F^-T; committed eqps + d, T + chi s_eff d / (rho c)
                             (temperature-dependent law), and, yielding or not, F_old = F, be_old = be
                             (materials.hpp:455-564, materials.cpp:184-203)
                 dP/dF : dF by hand for the hyperelastic laws; for the J2 laws by implicit differentiation of the scalar
                 equation, d delta = dq / (3 G + (H' rate + H rate' / dt) thermo) -- no difference quotient anywhere.  j2log:
                 d E_e = Q ((Q^T dC Q) o Gamma) Q^T with Gamma_ab the divided differences of 1/2 log on the eigenvalues,
                 (log a - log b) / (a - b) = 2 atanh(z) / (z (a + b)), z = (a - b) / (a + b), atanh(z) / z by its series where
                 |z| < 1e-3: accurate where eigenvalues are close or equal, and Q need not be well determined there because
                 Gamma is then constant to the same order.  j2simo: the product rule through f_bar, be, N_p, and
                 d delta = (d s_eff - G delta d tr be) / (G tr be + (H' rate + H rate' / dt) thermo).
    symmetric    `sym_eig`: cyclic Jacobi in long double, vectorised over the points (2 x 2 and 3 x 3), rotations skipped
    functions    where the off-diagonal entry is exactly 0; `sym_fun` = Q f(lam) Q^T for 1/2 log and exp.
    sums         r_(A,i) = sum_q w det P_iJ dN_A/dX_J;  (K v)_(A,i) = sum_q w det dN_A/dX_J (dP/dF : dF_q(v))_iJ with
                 dF_q(v) = sum_B v_B (x) dN_B/dX;  the committed state per point;  and the three linear forms of
                 kernels_forms.hpp applied to a vector: mass rho sum w det N_A N_B v_(B,i), viscosity nu sum w det
                 (dN_A/dX . dN_B/dX) v_(B,i), body force b_i sum w det N_A.

Vectors are [n_nodes * dim], node-major (entry A * dim + i).  State matrices are [q, i, J]; the state of the finite-strain laws
is named as mimi_hip_domain_get_state orders it: eqps, temperature, the first matrix (Fp_inv | be_old), the second (F_old,
j2simo only)."""
import functools
import types

import numpy as np

import _face_reference as fr
from _cases import HARDENING_LAWS, POISSON, YOUNG, thermal_of

LD = np.longdouble
BISECTIONS = 100
DBL_EPSILON = LD(2.220446049250313e-16)                 # AlmostZero (material_utils.hpp:14-17)
SOLVER_LAWS = ("j2", "j2log", "j2simo")                 # the laws with a hardening law and a scalar equation


# ---- points --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _space(degrees, knots, weights, order):
    dim = len(degrees)
    nq = fr.points_per_direction(degrees, order)
    N, dN, w = fr._volume_basis(degrees, knots, order)
    x1d = [fr.rule_on_spans(k, p, nq)[0] for k, p in zip(knots, degrees)]
    idx = [g.ravel(order="F") for g in np.meshgrid(*[np.arange(len(x)) for x in x1d], indexing="ij")]
    xi = np.stack([x1d[d][idx[d]] for d in range(dim)], axis=1)
    if weights is not None:
        wa = np.array(weights, dtype=LD)
        W = N @ wa
        dW = dN @ wa                                                            # [q, d]
        N, dN = (N * wa / W[:, None],
                 wa * (dN * W[:, None, None] - N[:, None, :] * dW[:, :, None]) / (W * W)[:, None, None])
    for a in (N, dN, w, xi):
        a.setflags(write=False)
    n_ctrl = [len(k) - p - 1 for k, p in zip(knots, degrees)]
    breaks = [np.unique(np.asarray(k, dtype=np.float64)) for k in knots]
    return types.SimpleNamespace(dim=dim, degrees=degrees, N=N, dN=dN, w=w, xi=xi, nq=nq, n_ctrl=n_ctrl, breaks=breaks,
                                 n_nodes=int(np.prod(n_ctrl)), n_points=len(w), n_spans=[len(b) - 1 for b in breaks])


def space(degrees, knots, weights=None, order=-1):
    """the quadrature points of the patch: dense (rational) N [q, A], dN/dxi [q, d, A], the product weights w [q], the
    parameter coordinates xi [q, d].  Cached; never modified."""
    key = fr._key(degrees, knots)
    return _space(*key, None if weights is None else tuple(float(v) for v in np.asarray(weights).ravel()), int(order))


def in_box(sp, begin, end):
    """mask of the points whose parameters lie in the spans [begin_d, end_d) of every direction: by parameter range alone"""
    m = np.ones(sp.n_points, dtype=bool)
    for d in range(sp.dim):
        lo, hi = sp.breaks[d][begin[d]], sp.breaks[d][end[d]]
        m &= (sp.xi[:, d] > lo) & (sp.xi[:, d] < hi)
    return m


def layout(sp, begin=None, end=None):
    """grid[e, q]: the index on the grid of point q of element e in the (element, point) layout of include/mimi_hip.h, the
    elements those of the box in ascending order, both first direction fastest -- from the parameter coordinates: the span of
    a point is where its coordinate falls among the distinct knots, its place in the span its rank there"""
    dim, nq = sp.dim, sp.nq
    begin = [0] * dim if begin is None else list(begin)[:dim]
    end = sp.n_spans if end is None else list(end)[:dim]
    span, rank = [], []
    for d in range(dim):
        x = np.asarray(sp.xi[:, d], dtype=np.float64)
        s = np.searchsorted(sp.breaks[d], x, side="right") - 1
        distinct = np.unique(x)
        k = np.searchsorted(distinct, x)                                        # rank of the coordinate in the direction
        first = np.searchsorted(distinct, sp.breaks[d][s], side="left")         # rank of the first coordinate of the span
        span.append(s)
        rank.append(k - first)
    inside = in_box(sp, begin, end)
    m = [end[d] - begin[d] for d in range(dim)]
    e = np.zeros(sp.n_points, dtype=np.int64)
    q = np.zeros(sp.n_points, dtype=np.int64)
    for d in reversed(range(dim)):
        e = e * m[d] + (span[d] - begin[d])
        q = q * nq + rank[d]
    grid = np.full((int(np.prod(m)), nq ** dim), -1, dtype=np.int64)
    grid[e[inside], q[inside]] = np.nonzero(inside)[0]
    assert grid.min() >= 0 and len(np.unique(grid)) == grid.size
    return grid


# ---- small dense algebra in long double ----------------------------------------------------------------------------------
def det(M):
    if M.shape[-1] == 2:
        return M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 1, 0]
    return (M[..., 0, 0] * (M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1])
            - M[..., 0, 1] * (M[..., 1, 0] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 0])
            + M[..., 0, 2] * (M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]))


def inverse(M):
    """adjugate / determinant, by explicit cofactors"""
    n = M.shape[-1]
    C = np.empty_like(M)
    if n == 2:
        C[..., 0, 0], C[..., 0, 1] = M[..., 1, 1], -M[..., 0, 1]
        C[..., 1, 0], C[..., 1, 1] = -M[..., 1, 0], M[..., 0, 0]
    else:
        for i in range(3):
            for j in range(3):
                a, b = (j + 1) % 3, (j + 2) % 3          # rows of M
                c, d = (i + 1) % 3, (i + 2) % 3          # columns of M
                C[..., i, j] = M[..., a, c] * M[..., b, d] - M[..., a, d] * M[..., b, c]
    return C / det(M)[..., None, None]


def mm(A, B):
    return np.einsum("...ij,...jk->...ik", A, B)


def tr(A):
    return np.einsum("...ii->...", A)


def T(A):
    return np.swapaxes(A, -1, -2)


def ddot(A, B):
    return np.einsum("...ij,...ij->...", A, B)


def frob(A):
    return np.sqrt(ddot(A, A))


def eye(dim):
    return np.eye(dim, dtype=LD)


def dev(A):
    return A - tr(A)[..., None, None] / A.shape[-1] * eye(A.shape[-1])


def sym_eig(A, sweeps=30):
    """(lam [n, d], Q [n, d, d]) with A = Q diag(lam) Q^T for symmetric A [n, d, d]: cyclic Jacobi, every point rotated in
    every step (by the identity where its off-diagonal entry is exactly 0), until every off-diagonal entry is below
    1e-25 of the largest diagonal one"""
    A = np.array(A, dtype=LD)
    A = (A + T(A)) / 2
    n, d = A.shape[0], A.shape[-1]
    Q = np.broadcast_to(eye(d), A.shape).copy()
    off = ~np.eye(d, dtype=bool)
    for _ in range(sweeps):
        if np.abs(A[:, off]).max(initial=0) <= LD(1e-25) * np.abs(A[:, ~off]).max(initial=0):
            break
        for p in range(d):
            for q in range(p + 1, d):
                apq = A[:, p, q]
                on = apq != 0
                tau = (A[:, q, q] - A[:, p, p]) / (2 * np.where(on, apq, LD(1)))
                t = np.where(on, np.where(tau >= 0, LD(1), LD(-1)) / (np.abs(tau) + np.sqrt(1 + tau * tau)), LD(0))
                c = 1 / np.sqrt(1 + t * t)
                sn = t * c
                R = np.broadcast_to(eye(d), A.shape).copy()
                R[:, p, p], R[:, q, q], R[:, p, q], R[:, q, p] = c, c, sn, -sn
                A = mm(mm(T(R), A), R)
                A = (A + T(A)) / 2
                A[:, p, q] = A[:, q, p] = 0
                Q = mm(Q, R)
    else:
        raise AssertionError("the Jacobi sweeps do not converge")
    return np.einsum("nii->ni", A).copy(), Q


def spectral(Q, f):
    """Q diag(f) Q^T"""
    return np.einsum("nia,na,nja->nij", Q, f, Q)


def sym_fun(A, f):
    lam, Q = sym_eig(A)
    return spectral(Q, f(lam))


def half_log_differences(lam):
    """Gamma[n, a, b] = (1/2 log lam_a - 1/2 log lam_b) / (lam_a - lam_b), 1 / (2 lam_a) on the diagonal"""
    a, b = lam[:, :, None], lam[:, None, :]
    z = (a - b) / (a + b)
    z2 = z * z
    series = 1 + z2 * (LD(1) / 3 + z2 * (LD(1) / 5 + z2 * (LD(1) / 7 + z2 * (LD(1) / 9 + z2 / 11))))
    small = np.abs(z) < LD(1e-3)
    zs = np.where(small, LD(0.5), z)
    return np.where(small, series, np.arctanh(zs) / zs) / (a + b)


# ---- geometry ------------------------------------------------------------------------------------------------------------
def geometry(sp, X):
    """dX/dxi [q, I, d], its determinant (positive), w det, and dN_A/dX_J [q, A, J] on the control points X [n_nodes, dim]"""
    X = np.asarray(X, dtype=LD).reshape(sp.n_nodes, sp.dim)
    G = np.einsum("qdA,AI->qId", sp.dN, X)
    dt = det(G)
    assert np.all(dt > 0), "the geometry map is not orientation preserving"
    dNdX = np.einsum("qdA,qdJ->qAJ", sp.dN, inverse(G))
    return types.SimpleNamespace(sp=sp, G=G, det=dt, wdet=sp.w * dt, dNdX=dNdX)


def gradient(geo, v):
    """sum_A v_A (x) dN_A/dX: [q, i, J]"""
    v = np.asarray(v, dtype=LD).reshape(geo.sp.n_nodes, geo.sp.dim)
    return np.einsum("Ai,qAJ->qiJ", v, geo.dNdX)


def deformation_gradient(geo, u):
    return eye(geo.sp.dim) + gradient(geo, u)


# ---- materials -----------------------------------------------------------------------------------------------------------
def constants():
    """MaterialBase::SetYoungPoisson (materials.cpp:7-14), in the doubles the codes under test hold"""
    lam = YOUNG * POISSON / ((1 + POISSON) * (1 - 2 * POISSON))
    mu = YOUNG / (2.0 * (1.0 + POISSON))
    K = YOUNG / (3.0 * (1.0 - (2.0 * POISSON)))
    return LD(lam), LD(mu), LD(K), LD(mu)


class Hardening:
    """a law of _cases.HARDENING_LAWS in long double, vectorised: H, H', rate, rate', thermo (material_hardening.hpp:79-346)"""

    def __init__(self, law, table=None, **thermal):
        oracle, _, attrs = (HARDENING_LAWS if table is None else table)[law]
        self.law, self.kind = law, oracle["kind"]
        self.a = {k: LD(float(v)) for k, v in attrs.items()}
        self.a.setdefault("C", LD(0))                     # (JohnsonCookRateDependentHardening::C_ unset: the fixtures' 0)
        self.thermal = {k: LD(float(v)) for k, v in thermal_of(law, **thermal).items()}
        self.sigma_y = float(attrs["sigma_y"] if "sigma_y" in attrs else attrs["A"])
        self.johnson_cook = self.kind.startswith("JohnsonCook")
        self.has_rate = self.kind in ("JohnsonCookRate", "JohnsonCookTempRate", "JohnsonCookConstTemp") and self.a["C"] != 0
        self.temperature_dependent = self.kind == "JohnsonCookTempRate"

    def H(self, e):
        a = self.a
        if self.kind == "PowerLaw":
            return a["sigma_y"] * (1 + e / a["eps0"]) ** (1 / a["n"])
        if self.kind == "Voce":
            return a["sigma_sat"] - (a["sigma_sat"] - a["sigma_y"]) * np.exp(-e / a["strain_constant"])
        small = np.abs(e) < LD(1e-13)                      # material_hardening.hpp:138
        return np.where(small, a["A"], a["A"] + a["B"] * np.where(small, LD(1), e) ** a["n"])

    def dH(self, e):
        a = self.a
        if self.kind == "PowerLaw":
            return a["sigma_y"] / (a["n"] * a["eps0"]) * (1 + e / a["eps0"]) ** (1 / a["n"] - 1)
        if self.kind == "Voce":
            return (a["sigma_sat"] - a["sigma_y"]) / a["strain_constant"] * np.exp(-e / a["strain_constant"])
        small = np.abs(e) < LD(1e-13)
        return np.where(small, LD(0), a["B"] * a["n"] * np.where(small, LD(1), e) ** (a["n"] - 1))

    def rate(self, r):
        if not self.has_rate:
            return np.ones_like(r)
        on = r > self.a["eps0_dot"]
        return np.where(on, 1 + self.a["C"] * np.log(np.where(on, r, self.a["eps0_dot"]) / self.a["eps0_dot"]), LD(1))

    def drate(self, r):
        if not self.has_rate:
            return np.zeros_like(r)
        on = r > self.a["eps0_dot"]
        return np.where(on, self.a["C"] / np.where(on, r, LD(1)), LD(0))

    def _homologous(self, temp):
        Tr, Tm = self.a["reference_temperature"], self.thermal["melting_temperature"]
        return 1 - ((temp - Tr) / (Tm - Tr)) ** self.a["m"]

    def thermo(self, temp):
        if self.kind == "JohnsonCookTempRate":
            Tr, Tm = self.a["reference_temperature"], self.thermal["melting_temperature"]
            mid = (temp >= Tr) & (temp <= Tm)
            return np.where(temp < Tr, LD(1), np.where(temp > Tm, LD(0), self._homologous(np.where(mid, temp, Tr))))
        if self.kind == "JohnsonCookConstTemp":            # SetTemperature(initial): the state's temperature is ignored
            return np.full_like(temp, self._homologous(self.thermal["initial_temperature"]))
        return np.ones_like(temp)


def material(name, law=None, table=None, **thermal):
    """'neohook' | 'stvk' | 'j2' (law: a name of HARDENING_LAWS, the default JohnsonCookTempRate = _cases.JC_TEST) |
    'j2log' | 'j2simo' (law: the same) | 'j2linear' (the constants of _cases.oracle_material / product_material);
    table: a dict in the format of HARDENING_LAWS to take the law from instead (tests/_status_cases.py)"""
    m = types.SimpleNamespace(name=name, stateful=name in SOLVER_LAWS + ("j2linear",), solver=name in SOLVER_LAWS)
    if m.solver:
        m.hardening = Hardening(law or "JohnsonCookTempRate", table, **thermal)
        m.density = LD(1)
    if name == "j2linear":
        m.h_iso, m.h_kin, m.sigma_y = LD(40.0), LD(25.0), LD(70.0)
    return m


def virgin_state(mat, n, dim):
    """eqps, plastic strain, temperature (j2), back stress (j2linear) of n points; eqps, temperature, Fp_inv = I (j2log);
    eqps, temperature, be_old = F_old = I (j2simo); None for the stateless laws"""
    if not mat.stateful:
        return None
    if mat.name in ("j2log", "j2simo"):
        st = types.SimpleNamespace(eqps=np.zeros(n, dtype=LD), temperature=np.full(n, mat.hardening.thermal["initial_temperature"], dtype=LD))
        one = np.broadcast_to(eye(dim), (n, dim, dim))
        if mat.name == "j2log":
            st.Fp_inv = one.copy()
        else:
            st.be_old, st.F_old = one.copy(), one.copy()
        return st
    st = types.SimpleNamespace(eqps=np.zeros(n, dtype=LD), plastic_strain=np.zeros((n, dim, dim), dtype=LD))
    if mat.name == "j2":
        st.temperature = np.full(n, mat.hardening.thermal["initial_temperature"], dtype=LD)
    else:
        st.beta = np.zeros((n, dim, dim), dtype=LD)
    return st


def take(state, idx):
    return None if state is None else types.SimpleNamespace(**{k: v[idx] for k, v in vars(state).items()})


def _pk1_from_cauchy(F, sigma, dsigmas, dFs):
    """P = J sigma F^-T and its derivative J tr(F^-1 dF) sigma F^-T + J dsigma F^-T - J sigma F^-T dF^T F^-T"""
    J, Fi = det(F), inverse(F)
    FiT = T(Fi)
    P = J[:, None, None] * mm(sigma, FiT)
    dPs = [tr(mm(Fi, dF))[:, None, None] * P + J[:, None, None] * mm(ds, FiT) - mm(mm(P, T(dF)), FiT)
           for ds, dF in zip(dsigmas, dFs)]
    return P, dPs, frob(J[:, None, None] * FiT)


def _root(R, plastic, upper, scale):
    """the root of the decreasing R in [0, upper] at the points of `plastic` (0 elsewhere) by plain bisection"""
    lo, hi = np.zeros(len(upper), dtype=LD), np.where(plastic, upper, LD(0))
    assert np.all(R(lo)[plastic] > 0) and np.all(R(hi)[plastic] <= 1e-15 * scale[plastic]), "the root is not bracketed"
    for _ in range(BISECTIONS):
        mid = (lo + hi) / 2
        up = R(mid) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return np.where(plastic, (lo + hi) / 2, LD(0))


def trial_state(mat, F, state):
    """the trial state of a law with a scalar equation (j2, j2log, j2simo) at the points F [q, i, J] from `state`, before any
    root is sought: q [q] (the trial q | s_eff) and limit [q] = H(eqps) thermo(T), the yield stress the trial q is held
    against (sigma_y thermo on the virgin state) -- a point yields where q > limit -- with the pieces the law goes on with
    (p, s, thermo, and for the finite-strain laws slope0 and their kinematics).  point_law and _finite_strain_law start from
    it; tests/_status_cases.py takes its predicate "this point yields" from it"""
    F = np.asarray(F, dtype=LD)
    dim = F.shape[-1]
    I = eye(dim)
    _, _, K, G = constants()
    h = mat.hardening
    r32 = np.sqrt(LD(3) / 2)
    thermo = h.thermo(state.temperature)
    t = types.SimpleNamespace(thermo=thermo, limit=h.H(state.eqps) * thermo, r32=r32)
    if mat.name == "j2":
        eps = (F + T(F)) / 2 - I - state.plastic_strain
        t.p = K * tr(eps)
        t.s = 2 * G * (eps - tr(eps)[:, None, None] / dim * I)
        t.q = r32 * frob(t.s)
        return t
    n = F.shape[0]
    t.J, t.Fi = det(F), inverse(F)
    t.FiT = T(t.Fi)
    if mat.name == "j2log":
        t.Fe = mm(F, state.Fp_inv)
        t.lam, t.Q = sym_eig(mm(T(t.Fe), t.Fe))
        E = spectral(t.Q, np.log(t.lam) / 2)
        t.p, t.s = K * tr(E), 2 * G * dev(E)
        t.q = r32 * frob(t.s)
        t.slope0 = np.full(n, 3 * G, dtype=LD)
    else:
        t.f0 = inverse(mm(state.F_old, t.Fi))
        t.c = np.cbrt(det(t.f0))
        t.fb = t.f0 * t.c[:, None, None]
        t.be = mm(mm(t.fb, state.be_old), T(t.fb))
        t.s = G * dev(t.be)
        t.sn = frob(t.s)
        t.small = t.sn < DBL_EPSILON
        t.sns = np.where(t.small, LD(1), t.sn)
        t.Np = np.where(t.small[:, None, None], np.sqrt(LD(1) / 2) * I, (r32 / t.sns)[:, None, None] * t.s)
        t.q = ddot(t.Np, t.s)                                                    # s_effective
        t.tr_be = tr(t.be)
        t.slope0 = G * t.tr_be
    return t


def _finite_strain_law(mat, F, state, dt, dFs, delta=None):
    """j2log and j2simo (module docstring).  Beyond what point_law returns for j2: slope0 [q] (the coefficient of d in the
    scalar equation: 3 G | G tr be), stress_scale [q] (|dP| / |d delta| of the one-step bar derived in
    tests/_finite_strain_return.py: 2 G sqrt(3/2) |det F F^-T|_F | G 2/3 tr(be) sqrt(3/2) |F^-T|_F), spectrum [q, dim] (the
    eigenvalues of C_e | of the trial be), and cond [q] = cond(C_e) (j2log) or fbar2 [q] = |f_bar|_2^2 and tr_be [q] = tr of the
    trial be (j2simo)"""
    n, dim = F.shape[0], F.shape[-1]
    I = eye(dim)
    _, _, K, G = constants()
    h = mat.hardening
    t = trial_state(mat, F, state)
    J, Fi, FiT, thermo, e0, r32, q, slope0, s = t.J, t.Fi, t.FiT, t.thermo, state.eqps, t.r32, t.q, t.slope0, t.s
    dJs = [J * tr(mm(Fi, dF)) for dF in dFs]
    out = types.SimpleNamespace()
    if mat.name == "j2log":
        Fe, lam, Q, p = t.Fe, t.lam, t.Q, t.p
        out.spectrum, out.cond = lam, lam.max(axis=1) / lam.min(axis=1)
    else:
        f0, c, fb, be, sn, small, sns, Np, tr_be = t.f0, t.c, t.fb, t.be, t.sn, t.small, t.sns, t.Np, t.tr_be
        out.tr_be, out.fbar2, out.spectrum = tr_be, sym_eig(mm(T(fb), fb))[0].max(axis=1), sym_eig(be)[0]
    margin = q - t.limit
    plastic = margin > 0
    if delta is None:
        delta = _root(lambda d: q - slope0 * d - h.H(e0 + d) * h.rate(d / dt) * thermo, plastic, margin / slope0, q)
    e1 = e0 + delta
    slope = slope0 + (h.dH(e1) * h.rate(delta / dt) + h.H(e1) * h.drate(delta / dt) / dt) * thermo
    new = types.SimpleNamespace(eqps=e1, temperature=state.temperature.copy())
    if mat.name == "j2log":
        qs = np.where(q > 0, q, LD(1))
        Np = (LD(1.5) / qs)[:, None, None] * s
        shrink = 1 - 3 * G * delta / qs                                          # s_new = s - 2 G delta N_p = s shrink
        sigma = shrink[:, None, None] * s + (p / J)[:, None, None] * I
        new.Fp_inv = mm(state.Fp_inv, sym_fun(-delta[:, None, None] * Np, np.exp))
        Gamma = half_log_differences(lam)
        dsigmas = []
        for dF, dJ in zip(dFs, dJs):
            dFe = mm(dF, state.Fp_inv)
            dC = mm(T(dFe), Fe) + mm(T(Fe), dFe)
            dE = mm(mm(Q, mm(mm(T(Q), dC), Q) * Gamma), T(Q))
            dp, ds = K * tr(dE), 2 * G * dev(dE)
            dq = LD(1.5) * ddot(s, ds) / qs
            dd = np.where(plastic, dq / slope, LD(0))
            dsn = shrink[:, None, None] * ds - (3 * G * (dd / qs - delta * dq / (qs * qs)))[:, None, None] * s
            dsigmas.append(dsn + (dp / J - p * dJ / (J * J))[:, None, None] * I)
        out.P, out.dP, out.JFinvT_norm = _pk1_from_cauchy(F, sigma, dsigmas, dFs)
        out.stress_scale = 2 * G * r32 * out.JFinvT_norm
    else:
        flow = LD(2) / 3 * delta * tr_be
        be_new = be - flow[:, None, None] * Np
        tau = G * dev(be_new) + (K / 2 * (J * J - 1))[:, None, None] * I
        out.P = mm(tau, FiT)
        if h.temperature_dependent:
            new.temperature = state.temperature + h.thermal["heat_fraction"] * q * delta / (mat.density * h.thermal["specific_heat"])
        new.be_old, new.F_old = be_new, F.copy()
        f0i = inverse(f0)
        out.dP = []
        for dF, dJ in zip(dFs, dJs):
            dFi = -mm(mm(Fi, dF), Fi)
            df0 = -mm(mm(f0, mm(state.F_old, dFi)), f0)
            dc = c / 3 * tr(mm(f0i, df0))
            dfb = df0 * c[:, None, None] + f0 * dc[:, None, None]
            dbe = mm(mm(dfb, state.be_old), T(fb)) + mm(mm(fb, state.be_old), T(dfb))
            ds = G * dev(dbe)
            dn = ddot(s, ds) / sns
            dq = np.where(small, LD(0), r32 * dn)
            dNp = np.where(small[:, None, None], LD(0), r32 * (ds / sns[:, None, None] - (dn / (sns * sns))[:, None, None] * s))
            dtr = tr(dbe)
            dd = np.where(plastic, (dq - G * delta * dtr) / slope, LD(0))
            dflow = LD(2) / 3 * (dd * tr_be + delta * dtr)
            dbe_new = dbe - dflow[:, None, None] * Np - flow[:, None, None] * dNp
            dtau = G * dev(dbe_new) + (K * J * dJ)[:, None, None] * I
            out.dP.append(mm(dtau, FiT) + mm(tau, T(dFi)))
        out.stress_scale = G * LD(2) / 3 * tr_be * r32 * frob(FiT)
    out.new, out.plastic, out.margin, out.delta, out.q, out.slope0 = new, plastic, margin, delta, q, slope0
    return out


def point_law(mat, F, state=None, dt=1.0, dFs=(), delta=None):
    """the law at the points F [q, i, J] from `state`: a namespace with P [q, i, J], dP (one [q, i, J] per direction of
    dFs), and for the stateful laws the committed state `new`, plastic [q], margin [q] (the yield function of the trial
    state), delta [q], q [q] (the trial q | s_eff), JFinvT_norm [q]; more for j2log and j2simo (_finite_strain_law).
    delta [q]: take this increment at the plastic points instead of the root (to see what a root that is off does to the
    result: _domain_cases.root_shift; never as an answer)"""
    F = np.asarray(F, dtype=LD)
    dFs = [np.asarray(d, dtype=LD) for d in dFs]
    n, dim = F.shape[0], F.shape[-1]
    if mat.name in ("j2log", "j2simo"):
        return _finite_strain_law(mat, F, virgin_state(mat, n, dim) if state is None else state, LD(dt), dFs, delta)
    I = eye(dim)
    lam, mu, K, G = constants()
    out = types.SimpleNamespace(new=None)
    if mat.name == "neohook":
        J, Fi = det(F), inverse(F)
        FiT = T(Fi)
        out.P = mu * (F - FiT) + (lam * J * (J - 1))[:, None, None] * FiT
        out.dP = []
        for dF in dFs:
            t = tr(mm(Fi, dF))
            B = mm(mm(FiT, T(dF)), FiT)
            out.dP.append(mu * (dF + B) + lam * (((2 * J - 1) * J * t)[:, None, None] * FiT - (J * (J - 1))[:, None, None] * B))
        return out
    if mat.name == "stvk":
        E = (mm(T(F), F) - I) / 2
        S = lam * tr(E)[:, None, None] * I + 2 * mu * E
        out.P = mm(F, S)
        out.dP = []
        for dF in dFs:
            dE = (mm(T(dF), F) + mm(T(F), dF)) / 2
            out.dP.append(mm(dF, S) + mm(F, lam * tr(dE)[:, None, None] * I + 2 * mu * dE))
        return out
    state = virgin_state(mat, n, dim) if state is None else state
    dt = LD(dt)
    if mat.name == "j2":
        t = trial_state(mat, F, state)
        p, s = t.p, t.s
    else:
        eps = (F + T(F)) / 2 - I - state.plastic_strain
        p = K * tr(eps)
        s = 2 * G * (eps - tr(eps)[:, None, None] / dim * I)
    deps = [(dF + T(dF)) / 2 for dF in dFs]
    dp = [K * tr(de) for de in deps]
    ds = [2 * G * (de - tr(de)[:, None, None] / dim * I) for de in deps]
    r32 = np.sqrt(LD(3) / 2)
    if mat.name == "j2":
        h = mat.hardening
        q, thermo = t.q, t.thermo
        e0 = state.eqps
        margin = q - t.limit

        def R(d):
            return q - 3 * G * d - h.H(e0 + d) * h.rate(d / dt) * thermo

        plastic = margin > 0
        if delta is None:
            delta = _root(R, plastic, margin / (3 * G), q)
        out.slope0 = np.full(n, 3 * G, dtype=LD)
        qs = np.where(q > 0, q, LD(1))
        Np = (LD(1.5) / qs)[:, None, None] * s
        sigma = s - (2 * G * delta)[:, None, None] * Np + p[:, None, None] * I
        # implicit differentiation of R(delta; q) = 0:  dq - (3 G + (H' rate + H rate' / dt) thermo) d delta = 0
        e1 = e0 + delta
        slope = 3 * G + (h.dH(e1) * h.rate(delta / dt) + h.H(e1) * h.drate(delta / dt) / dt) * thermo
        dsigmas = []
        for dsk, dpk in zip(ds, dp):
            dq = LD(1.5) * ddot(s, dsk) / qs
            dd = np.where(plastic, dq / slope, LD(0))
            # s_new = s (1 - 3 G delta / q)
            dsn = dsk * (1 - 3 * G * delta / qs)[:, None, None] - (3 * G * (dd / qs - delta * dq / (qs * qs)))[:, None, None] * s
            dsigmas.append(dsn + dpk[:, None, None] * I)
        new = types.SimpleNamespace(eqps=e1, plastic_strain=state.plastic_strain + delta[:, None, None] * Np,
                                    temperature=state.temperature.copy())
        if h.temperature_dependent:
            new.temperature = state.temperature + h.thermal["heat_fraction"] * q * delta / (mat.density * h.thermal["specific_heat"])
    else:
        eta = s - state.beta
        en = frob(eta)
        q = r32 * en
        margin = q - (mat.sigma_y + mat.h_iso * state.eqps)
        plastic = margin > 0
        denom = 3 * G + mat.h_kin + mat.h_iso
        delta = np.where(plastic, margin / denom, LD(0))
        ens = np.where(en > 0, en, LD(1))
        nh = eta / ens[:, None, None]
        r6 = np.sqrt(LD(6))
        sigma = s - (r6 * G * delta)[:, None, None] * nh + p[:, None, None] * I
        dsigmas = []
        for dsk, dpk in zip(ds, dp):
            dn = ddot(nh, dsk)                                                  # d |eta|
            dd = np.where(plastic, r32 * dn / denom, LD(0))
            dnh = (dsk - dn[:, None, None] * nh) / ens[:, None, None]
            dsigmas.append(dsk - r6 * G * (dd[:, None, None] * nh + delta[:, None, None] * dnh) + dpk[:, None, None] * I)
        new = types.SimpleNamespace(eqps=state.eqps + delta, plastic_strain=state.plastic_strain + (r32 * delta)[:, None, None] * nh,
                                    beta=state.beta + (np.sqrt(LD(2) / 3) * mat.h_kin * delta)[:, None, None] * nh)
    out.P, out.dP, out.JFinvT_norm = _pk1_from_cauchy(F, sigma, dsigmas, dFs)
    out.new, out.plastic, out.margin, out.delta, out.q = new, plastic, margin, delta, q
    return out


# ---- sums ----------------------------------------------------------------------------------------------------------------
def nodal(geo, M, mask=None):
    """sum_q w det M[q, i, J] dN_A/dX_J: [n_nodes * dim]"""
    wd = geo.wdet if mask is None else np.where(mask, geo.wdet, LD(0))
    return np.einsum("q,qiJ,qAJ->Ai", wd, M, geo.dNdX).reshape(-1)


def assemble(geo, mat, u, state=None, dt=1.0, vectors=(), mask=None):
    """residual r, K v for every v of `vectors`, and the point results `pt` (point_law) at the displacement u from `state`;
    mask: only those points"""
    pt = point_law(mat, deformation_gradient(geo, u), state, dt, [gradient(geo, v) for v in vectors])
    return types.SimpleNamespace(r=nodal(geo, pt.P, mask), Kv=[nodal(geo, dP, mask) for dP in pt.dP], pt=pt)


def mass_times(geo, density, v, mask=None):
    sp = geo.sp
    wd = geo.wdet if mask is None else np.where(mask, geo.wdet, LD(0))
    vq = sp.N @ np.asarray(v, dtype=LD).reshape(sp.n_nodes, sp.dim)
    return LD(density) * (sp.N.T @ (wd[:, None] * vq)).reshape(-1)


def diffusion_times(geo, viscosity, v, mask=None):
    return LD(viscosity) * nodal(geo, gradient(geo, v), mask)


def body_force(geo, b, mask=None):
    wd = geo.wdet if mask is None else np.where(mask, geo.wdet, LD(0))
    return np.outer(geo.sp.N.T @ wd, np.asarray(b, dtype=LD)).reshape(-1)


def support_pattern(sp, dim=None):
    """(rowptr, col) of the union of the element blocks over the vdofs, columns ascending -- from the values: node B is in the
    row of node A when some point sees both.  Also the connectivity conn[e, a] (ascending node ids) in the layout's element
    order"""
    dim = sp.dim if dim is None else dim
    seen = sp.N != 0
    grid = layout(sp)
    conn = np.stack([np.nonzero(seen[g].any(axis=0))[0] for g in grid])
    pair = np.zeros((sp.n_nodes, sp.n_nodes), dtype=bool)
    for c in conn:
        pair[np.ix_(c, c)] = True
    rowptr, col = [0], []
    for A in range(sp.n_nodes):
        nb = np.nonzero(pair[A])[0]
        cols = (nb[:, None] * dim + np.arange(dim)).ravel()
        for _ in range(dim):
            col.append(cols)
            rowptr.append(rowptr[-1] + len(cols))
    return np.array(rowptr, dtype=np.int64), np.concatenate(col).astype(np.int32), conn.astype(np.int32)
