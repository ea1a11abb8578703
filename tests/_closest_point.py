"""The closest point on a rigid B-spline / NURBS curve or surface, and what the reference's MortarContact does with it,
in numpy long double -- written from the definitions and from integrators/mortar_contact.cpp:148-261, sharing neither code
nor scheme with mimi_amd/csrc/spline_body.hpp or oracle/contact_path.c.

    evaluation   Cox-de Boor recursion over ALL basis functions, N_{i,0} = [U_i <= x < U_{i+1}] (the upper end belongs to
                 the last non-empty span), derivatives by N'_{i,d} = d (N_{i,d-1} / (U_{i+d} - U_i) - N_{i+1,d-1} /
                 (U_{i+d+1} - U_{i+1})), 0/0 = 0; the rational S, S_k, S_kl by the quotient rule.  One-sided derivatives on
                 a knot are therefore those FROM THE RIGHT (from the left at the upper end), as sb_find_span takes them.
    closest      brute force: the squared distance on a dense parametric grid (GRID_CURVE points, GRID_SURFACE^2 for
                 surfaces), EVERY local minimum of the grid kept, each polished in long double (curves: bisection on the
                 sign of S' . (S - x); surfaces: bound-constrained Newton inside the grid cells around it, its KKT residual
                 checked afterwards), the best returned with its margin over the second best.  A direction with
                 S(lo) == S(hi) is periodic: the grid wraps and a polish may cross the seam.
    downstream   nodal_gap_area: x_q, tangents, |J|, the body normal (t_y, -t_x) / S_u x S_v, g = -n . (S - x_q) clipped
                 to min(g, 0) and zeroed beyond the angle tolerance, A_i, G_i, p_i = eps G_i / A_i, GapNorm.

Bodies are the dicts of tests/test_contact.py: kind="spline", degrees, knots, control_points [n][dim] (first parametric
direction fastest, as RigidSpline), weights or None, resolution."""
import numpy as np

LD = np.longdouble
GRID_CURVE = 4001
GRID_SURFACE = 301


# ---- evaluation --------------------------------------------------------------------------------------------------------
def _basis_table(U, p, x):
    """tabs[d][:, i] = N_{i,d}(x), d = 0..p, straight from the Cox-de Boor definition"""
    m = len(U)
    N0 = np.zeros((len(x), m - 1), dtype=LD)
    nonempty = [i for i in range(m - 1) if U[i] < U[i + 1]]
    for i in nonempty:
        N0[:, i] = (U[i] <= x) & (x < U[i + 1])
    N0[x == U[-1], nonempty[-1]] = 1
    tabs = [N0]
    for d in range(1, p + 1):
        prev, Nd = tabs[-1], np.zeros((len(x), m - d - 1), dtype=LD)
        for i in range(m - d - 1):
            a, b = U[i + d] - U[i], U[i + d + 1] - U[i + 1]
            if a > 0:
                Nd[:, i] += (x - U[i]) / a * prev[:, i]
            if b > 0:
                Nd[:, i] += (U[i + d + 1] - x) / b * prev[:, i + 1]
        tabs.append(Nd)
    return tabs


def _derive(U, d, lower):
    """derivative (of any order r) of the degree-d functions from the order r - 1 derivative of the degree d - 1 ones"""
    out = np.zeros((lower.shape[0], len(U) - d - 1), dtype=LD)
    for i in range(out.shape[1]):
        a, b = U[i + d] - U[i], U[i + d + 1] - U[i + 1]
        if a > 0:
            out[:, i] += d / a * lower[:, i]
        if b > 0:
            out[:, i] -= d / b * lower[:, i + 1]
    return out


def basis(U, p, x):
    """(N, N', N'') [n_x][n_ctrl] of the degree-p B-splines on U at x, long double"""
    U, x = np.asarray(U, dtype=LD), np.asarray(x, dtype=LD)
    tabs = _basis_table(U, p, x)
    N = tabs[p]
    D1 = _derive(U, p, tabs[p - 1]) if p >= 1 else np.zeros_like(N)
    D2 = _derive(U, p, _derive(U, p - 1, tabs[p - 2])) if p >= 2 else np.zeros_like(N)
    return N, D1, D2


class Body:
    def __init__(self, body):
        self.p = [int(d) for d in body["degrees"]]
        self.U = [np.asarray(k, dtype=LD) for k in body["knots"]]
        self.pd = len(self.p)
        self.n = [len(U) - p - 1 for U, p in zip(self.U, self.p)]
        ctrl = np.asarray(body["control_points"], dtype=np.float64)
        self.dim = ctrl.shape[1]
        w = body.get("weights")
        self.w = np.ones(len(ctrl), dtype=LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)
        self.cw = ctrl.astype(LD) * self.w[:, None]
        self.lo = np.array([U[p] for U, p in zip(self.U, self.p)], dtype=LD)
        self.hi = np.array([U[-p - 1] for U, p in zip(self.U, self.p)], dtype=LD)
        self.resolution = int(body.get("resolution", 100))
        # closed directions, from the geometry itself: the two end curves / end points coincide
        self.closed = []
        probe = np.linspace(0.0, 1.0, 33).astype(LD)
        for k in range(self.pd):
            ends = []
            for e in (self.lo[k], self.hi[k]):
                xi = np.zeros((1 if self.pd == 1 else len(probe), self.pd), dtype=LD)
                xi[:, k] = e
                if self.pd == 2:
                    xi[:, 1 - k] = self.lo[1 - k] + (self.hi[1 - k] - self.lo[1 - k]) * probe
                ends.append(self._raw(xi)[0])
            scale = max(float(np.abs(self.cw / self.w[:, None]).max()), 1.0)
            self.closed.append(bool(np.abs(ends[0] - ends[1]).max() < 1e-14 * scale))

    def wrap(self, xi):
        """map unwrapped coordinates of the closed directions back into [lo, hi]"""
        xi = np.array(xi, dtype=LD)
        for k in range(self.pd):
            if self.closed[k]:
                L = self.hi[k] - self.lo[k]
                out = (xi[:, k] < self.lo[k]) | (xi[:, k] > self.hi[k])
                xi[out, k] = self.lo[k] + np.mod(xi[out, k] - self.lo[k], L)
        return xi

    def _raw(self, xi):
        B = [basis(self.U[k], self.p[k], xi[:, k]) for k in range(self.pd)]
        if self.pd == 1:
            A = [B[0][o] @ np.concatenate([self.cw, self.w[:, None]], axis=1) for o in range(3)]
            orders = {(0,): A[0], (1,): A[1], (2,): A[2]}
        else:
            H = np.concatenate([self.cw, self.w[:, None]], axis=1).reshape(self.n[1], self.n[0], self.dim + 1)
            orders = {}
            for o0, o1 in ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)):
                orders[(o0, o1)] = np.einsum("qa,qb,bac->qc", B[0][o0], B[1][o1], H)
        dim, pd = self.dim, self.pd

        def order(*ks):
            """the homogeneous sum differentiated once in each of the directions ks"""
            o = [0] * pd
            for k in ks:
                o[k] += 1
            return orders[tuple(o)]

        A0 = order()
        W = A0[:, dim:]
        S = A0[:, :dim] / W
        S1 = np.zeros((len(xi), pd, dim), dtype=LD)
        S2 = np.zeros((len(xi), pd, pd, dim), dtype=LD)
        for k in range(pd):
            Ak = order(k)
            S1[:, k] = (Ak[:, :dim] - Ak[:, dim:] * S) / W
        for k in range(pd):
            for l in range(pd):
                Akl, Wk, Wl = order(k, l), order(k)[:, dim:], order(l)[:, dim:]
                S2[:, k, l] = (Akl[:, :dim] - Akl[:, dim:] * S - Wk * S1[:, l] - Wl * S1[:, k]) / W
        return S, S1, S2

    def evaluate(self, xi):
        """S [n][dim], S_k [n][pd][dim], S_kl [n][pd][pd][dim] at xi [n][pd] (closed directions may be unwrapped)"""
        xi = np.asarray(xi, dtype=LD).reshape(-1, self.pd)
        return self._raw(self.wrap(xi))

    def sample_spacing(self):
        """largest distance between neighbouring samples of the body's own initial-guess grid (`resolution` per direction)"""
        res = self.resolution
        t = [np.asarray(self.lo[k] + (self.hi[k] - self.lo[k]) * np.arange(res, dtype=LD) / (res - 1)) for k in range(self.pd)]
        if self.pd == 1:
            S = self.evaluate(t[0][:, None])[0].astype(np.float64)
            return float(np.linalg.norm(np.diff(S, axis=0), axis=1).max())
        g1, g0 = np.meshgrid(t[1], t[0], indexing="ij")
        S = self.evaluate(np.stack([g0.ravel(), g1.ravel()], axis=1))[0].astype(np.float64).reshape(res, res, -1)
        return float(max(np.linalg.norm(np.diff(S, axis=0), axis=2).max(), np.linalg.norm(np.diff(S, axis=1), axis=2).max()))


# ---- brute-force global closest point ----------------------------------------------------------------------------------
class Closest:
    """xi [n][pd], S [n][dim], S1 [n][pd][dim], distance [n], margin [n] (distance of the second-best local minimum minus
    the best; inf where there is only one), well_conditioned [n] (the Hessian of the squared distance on the free
    coordinates is positive definite with condition < 1e6 and no coordinate sits on a bound)"""


def _grid(body, k):
    n = GRID_CURVE if body.pd == 1 else GRID_SURFACE
    t = np.asarray(body.lo[k] + (body.hi[k] - body.lo[k]) * np.arange(n, dtype=LD) / (n - 1))
    return t[:-1] if body.closed[k] else t


def _curve_candidates(body, xq):
    t = _grid(body, 0)
    h = (body.hi[0] - body.lo[0]) / (GRID_CURVE - 1)
    S = body.evaluate(t[:, None])[0]
    d2 = ((S[None, :, :] - xq[:, None, :]) ** 2).sum(axis=2).astype(np.float64)          # [query][grid]
    if body.closed[0]:
        left, right = np.roll(d2, 1, axis=1), np.roll(d2, -1, axis=1)
    else:
        inf = np.full((len(xq), 1), np.inf)
        left, right = np.concatenate([inf, d2[:, :-1]], axis=1), np.concatenate([d2[:, 1:], inf], axis=1)
    iq, ig = np.nonzero((d2 <= left) & (d2 < right))
    a, b = t[ig] - h, t[ig] + h
    if not body.closed[0]:
        a, b = np.maximum(a, body.lo[0]), np.minimum(b, body.hi[0])
    q = xq[iq]

    def grad(x):
        P, P1, _ = body.evaluate(x[:, None])
        return (P1[:, 0] * (P - q)).sum(axis=1)

    ga, gb = grad(a), grad(b)
    at_a = (ga >= 0) & (a <= body.lo[0]) & (not body.closed[0])
    at_b = (gb <= 0) & (b >= body.hi[0]) & (not body.closed[0])
    inner = ~(at_a | at_b)
    if not np.all((ga[inner] < 0) & (gb[inner] > 0)):
        raise AssertionError("a local minimum of the grid is not bracketed by its neighbours: refine the grid")
    for _ in range(80):
        mid = 0.5 * (a + b)
        neg = grad(mid) < 0
        a, b = np.where(inner & neg, mid, a), np.where(inner & ~neg, mid, b)
    x = np.where(at_a, a, np.where(at_b, b, 0.5 * (a + b)))
    return iq, x[:, None], (at_a | at_b)[:, None]


def _surface_candidates(body, xq):
    t0, t1 = _grid(body, 0), _grid(body, 1)
    h = np.array([(body.hi[k] - body.lo[k]) / (GRID_SURFACE - 1) for k in range(2)], dtype=LD)
    if getattr(body, "_grid_S", None) is None:
        g1, g0 = np.meshgrid(t1, t0, indexing="ij")
        body._grid_S = body.evaluate(np.stack([g0.ravel(), g1.ravel()], axis=1))[0].astype(np.float64).reshape(len(t1), len(t0), -1)
    S = body._grid_S
    xq64 = xq.astype(np.float64)
    n1, n0 = S.shape[:2]
    found = []
    for start in range(0, len(xq), 32):                      # (chunks of queries: the distance table is [query][i1][i0])
        d2 = sum((S[None, :, :, d] - xq64[start:start + 32, None, None, d]) ** 2 for d in range(body.dim))
        big = np.pad(d2, ((0, 0), (1, 1), (1, 1)), mode="constant", constant_values=np.inf)
        if body.closed[0]:
            big[:, :, 0], big[:, :, -1] = big[:, :, -2], big[:, :, 1]
        if body.closed[1]:
            big[:, 0, :], big[:, -1, :] = big[:, -2, :], big[:, 1, :]
        is_min = np.ones(d2.shape, dtype=bool)
        for s1 in (-1, 0, 1):
            for s0 in (-1, 0, 1):
                if (s1, s0) == (0, 0):
                    continue
                nb = big[:, 1 + s1:1 + s1 + n1, 1 + s0:1 + s0 + n0]
                is_min &= (d2 < nb) if (s1, s0) > (0, 0) else (d2 <= nb)
        cq, c1, c0 = np.nonzero(is_min)
        found.append((cq + start, c1, c0))
    iq, i1, i0 = (np.concatenate([f[j] for f in found]) for j in range(3))
    q = xq[iq]
    x = np.stack([t0[i0], t1[i1]], axis=1)
    a, b = x - h, x + h
    for k in range(2):
        if not body.closed[k]:
            a[:, k], b[:, k] = np.maximum(a[:, k], body.lo[k]), np.minimum(b[:, k], body.hi[k])

    def state(x):
        P, P1, P2 = body.evaluate(x)
        r = P - q
        g = np.einsum("nkd,nd->nk", P1, r)
        H = np.einsum("nkd,nld->nkl", P1, P1) + np.einsum("nkld,nd->nkl", P2, r)
        return (r * r).sum(axis=1), g, H

    f, g, H = state(x)
    slack = 64 * np.finfo(LD).eps * ((q * q).sum(axis=1) + f)      # rounding of |S - x|^2 at coordinates of size |x|
    for _ in range(60):
        # a coordinate on a DOMAIN bound with the gradient pointing outwards stays; the cell walls a, b inside the domain
        # only keep the iteration near its grid point and are checked not to be active at the end
        pin = ((x <= a) & (g > 0)) | ((x >= b) & (g < 0))
        gf = np.where(pin, 0, g)
        Hf = H.copy()
        for k in range(2):
            Hf[pin[:, k], k, :] = 0
            Hf[pin[:, k], :, k] = 0
            Hf[pin[:, k], k, k] = 1
        det = Hf[:, 0, 0] * Hf[:, 1, 1] - Hf[:, 0, 1] * Hf[:, 1, 0]
        ok = (det > 0) & (Hf[:, 0, 0] > 0)
        det = np.where(ok, det, 1)
        step = np.stack([-(Hf[:, 1, 1] * gf[:, 0] - Hf[:, 0, 1] * gf[:, 1]) / det,
                         -(Hf[:, 0, 0] * gf[:, 1] - Hf[:, 1, 0] * gf[:, 0]) / det], axis=1)
        step = np.where(ok[:, None], step, -gf / np.maximum(np.abs(np.diagonal(Hf, axis1=1, axis2=2)), 1e-30))
        moved = False
        scale = np.ones(len(x), dtype=LD)
        todo = np.ones(len(x), dtype=bool)
        for _half in range(30):
            xn = np.clip(x + scale[:, None] * step, a, b)
            fn, gn, Hn = state(xn)
            acc = todo & (fn <= f + slack) & np.any(xn != x, axis=1)   # (equal to rounding: Newton's last steps)
            if acc.any():
                moved = True
                x[acc], f[acc], g[acc], H[acc] = xn[acc], fn[acc], gn[acc], Hn[acc]
            todo &= ~acc & np.any(xn != x, axis=1)
            if not todo.any():
                break
            scale = np.where(todo, 0.5 * scale, scale)
        if not moved:
            break
    wall = np.zeros(x.shape, dtype=bool)
    for k in range(2):
        on_domain = ((x[:, k] <= body.lo[k]) | (x[:, k] >= body.hi[k])) & (not body.closed[k])
        pinned = ((x[:, k] <= a[:, k]) & (g[:, k] > 0)) | ((x[:, k] >= b[:, k]) & (g[:, k] < 0))
        if np.any(pinned & ~on_domain):
            raise AssertionError("a polish ran into the wall of its grid cells: refine the grid")
        wall[:, k] = pinned
    # KKT: the free gradient vanishes to the rounding of long double (relative to |S_k| |S - x|)
    _, P1, _ = body.evaluate(x)
    scale_g = np.sqrt((P1 ** 2).sum(axis=2)) * np.sqrt(f)[:, None] + 1e-300
    if np.any(np.where(wall, 0, np.abs(g) / scale_g) > 1e-15):
        raise AssertionError("a polish did not converge")
    return iq, x, wall


def closest(body, xq):
    """the global closest point of every query xq [n][dim] on the Body"""
    xq = np.asarray(xq, dtype=LD).reshape(-1, body.dim)
    iq, x, pinned = (_curve_candidates if body.pd == 1 else _surface_candidates)(body, xq)
    P, P1, P2 = body.evaluate(x)
    r = P - xq[iq]
    dist = np.sqrt((r * r).sum(axis=1))
    out = Closest()
    n = len(xq)
    out.xi = np.zeros((n, body.pd), dtype=LD)
    out.S, out.S1 = np.zeros((n, body.dim), dtype=LD), np.zeros((n, body.pd, body.dim), dtype=LD)
    out.distance, out.margin = np.zeros(n, dtype=LD), np.full(n, np.inf)
    out.well_conditioned = np.zeros(n, dtype=bool)
    out.pinned = np.zeros((n, body.pd), dtype=bool)
    H = np.einsum("nkd,nld->nkl", P1, P1) + np.einsum("nkld,nd->nkl", P2, r)
    period = [float(body.hi[k] - body.lo[k]) if body.closed[k] else 0.0 for k in range(body.pd)]
    h = [float(body.hi[k] - body.lo[k]) / ((GRID_CURVE if body.pd == 1 else GRID_SURFACE) - 1) for k in range(body.pd)]
    for i in range(n):
        c = np.nonzero(iq == i)[0]
        assert len(c) > 0
        c = c[np.argsort(dist[c].astype(np.float64), kind="stable")]
        b = c[0]
        out.xi[i], out.S[i], out.S1[i], out.distance[i], out.pinned[i] = body.wrap(x[b:b + 1])[0], P[b], P1[b], dist[b], pinned[b]
        # the second best: the nearest candidate that is another point of the parameter space (two neighbouring grid
        # minima may polish to one point)
        for o in c[1:]:
            sep = 0.0
            for k in range(body.pd):
                dk = abs(float(x[o, k] - x[b, k]))
                if period[k]:
                    dk = min(dk % period[k], period[k] - dk % period[k])
                sep = max(sep, dk / h[k])
            if sep > 1.0:
                out.margin[i] = float(dist[o] - dist[b])
                break
        ev = np.linalg.eigvalsh(H[b].astype(np.float64))
        out.well_conditioned[i] = bool(not pinned[b].any() and ev[0] > 0 and ev[-1] < 1e6 * ev[0])
    return out


# ---- downstream of the query: mortar_contact.cpp:148-261 ---------------------------------------------------------------
def body_normal(S1):
    """Results::ComputeNormal<true>: (t_y, -t_x) of the curve tangent, S_u x S_v of a surface, normalised"""
    if S1.shape[1] == 1:
        n = np.stack([S1[:, 0, 1], -S1[:, 0, 0]], axis=1)
    else:
        n = np.cross(S1[:, 0].astype(LD), S1[:, 1].astype(LD))
    return n / np.sqrt((n * n).sum(axis=1))[:, None]


def _angle(n, pmq, true_g):
    """acos(min(|g| / distance, 1)) of mortar_contact.cpp:182-186, evaluated as atan2(|tangential part|, |normal part|)
    of x_rigid - x_q: the same angle, without the cancellation of acos near 1"""
    tang = pmq + true_g[:, None] * n                      # pmq - (n . pmq) n,  g = -n . pmq
    return np.arctan2(np.sqrt((tang * tang).sum(axis=1)), np.abs(true_g))


class Nodal:
    """nodes (sorted marked node ids), area, gap, pressure [n_marked]; gap_norm; and per quadrature point [n_faces][n_q]:
    xq, true_g, distance, angle, margin, kept (angle <= angle_tol)"""


def nodal_gap_area(patch, tables, u, body, penalty=1.0e4, angle_tol=1.0e-5):
    """patch: anything with .ctrl [n_nodes][dim]; tables: (dofs, N, dN, w) of splines.face_tables; body: Body"""
    dofs, N, dN, w = tables
    dim = body.dim
    x = (np.asarray(patch.ctrl, dtype=np.float64) + np.asarray(u, dtype=np.float64).reshape(-1, dim)).astype(LD)
    N, dN, w = N.astype(LD), dN.astype(LD), w.astype(LD)
    xe = x[dofs]                                                    # [f][a][dim]
    xq = np.einsum("fqa,fad->fqd", N, xe)
    t = np.einsum("fqka,fad->fqkd", dN, xe)                         # tangents of the deformed face
    if dim == 2:
        J = np.sqrt((t[:, :, 0] ** 2).sum(axis=2))
    else:
        m = np.cross(t[:, :, 0], t[:, :, 1])
        J = np.sqrt((m * m).sum(axis=2))
    nf, nq = w.shape
    cp = closest(body, xq.reshape(-1, dim))
    n = body_normal(cp.S1)
    pmq = cp.S - xq.reshape(-1, dim)
    true_g = -(n * pmq).sum(axis=1)
    angle = _angle(n, pmq, true_g)
    g = np.minimum(true_g, 0)
    g = np.where(angle > LD(angle_tol), 0, g).reshape(nf, nq)
    fac = w * J
    la = np.einsum("fq,fqa->fa", fac, N)
    lg = np.einsum("fq,fqa->fa", fac * g, N)
    out = Nodal()
    out.nodes = np.unique(dofs)
    loc = np.searchsorted(out.nodes, dofs)
    out.area, out.gap = np.zeros(len(out.nodes), dtype=LD), np.zeros(len(out.nodes), dtype=LD)
    np.add.at(out.area, loc.ravel(), la.ravel())
    np.add.at(out.gap, loc.ravel(), lg.ravel())
    out.pressure = LD(penalty) * out.gap / out.area
    out.gap_norm = np.sqrt((np.minimum(true_g, 0) ** 2).sum())
    out.total_area = fac.sum()
    out.xq, out.closest = xq, cp
    out.true_g, out.distance = true_g.reshape(nf, nq), cp.distance.reshape(nf, nq)
    out.angle, out.margin = angle.reshape(nf, nq).astype(np.float64), cp.margin.reshape(nf, nq)
    out.kept = out.angle <= angle_tol
    return out


def check_conditions(nodal, body, clipping=False):
    """what every comparison presupposes, asserted on the reference alone"""
    a = nodal.angle
    assert not np.any((a > 1e-7) & (a < 1e-3)), "a quadrature point is neither clearly kept nor clearly dropped"
    assert np.all(nodal.margin >= body.sample_spacing()), "a query sits near the medial axis of the body"
    assert np.all(nodal.distance > 0)
    assert np.any(nodal.kept & (nodal.true_g < 0)), "no point in contact"
    if clipping:
        assert np.any(~nodal.kept), "no point dropped by the angle rule"
