"""The explicit central-difference step with a lumped mass and its energy ledger, restated in numpy from the formulas
(mimi_amd/csrc/explicit.hip states the same scheme; nothing is shared).  Any floating type: float64 to compare a device run
operation by operation, longdouble as the exact side of a sum.

Per dof, with the masks F (fixed) and P (constant velocity; P wins where both are set):
  predict   free: v <- v + (dt/2) a, x <- x + dt v;   P: v <- vbar, x <- x + dt vbar;   F: v <- 0
  correct   free: a <- ((f - r) - d) / m, v <- v + (dt/2) a;   P: a <- 0, v <- vbar;   F: a <- 0, v <- 0
  ledger    with vh the velocity after predict (dx = dt vh):
            W_int  += (dt/2) sum_all (r0 + r1) vh          W_damp += (dt/2) sum_free (d0 + d1) vh
            W_ext  += dt sum_free f vh + (dt/2) sum_P (r0 + r1) vbar
            KE = 1/2 sum m v^2 (free and P dofs),  Q = dt^2/8 sum_free m a^2,  E* = KE - Q + W_int + W_damp - W_ext
"""
import numpy as np


def masks(fixed, pres, n):
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    pres = np.zeros(n, dtype=bool) if pres is None else np.asarray(pres).astype(bool)
    return fixed & ~pres, pres, ~fixed & ~pres


def predict(dt, x, v, a, fixed, pres, vbar):
    """(x, v) after the predictor; fixed / pres as masks() returns them"""
    T = x.dtype.type
    dt, hdt = T(dt), T(0.5) * T(dt)
    free = ~fixed & ~pres
    v = np.where(free, v + hdt * a, np.where(pres, vbar, T(0)))
    x = np.where(fixed, x, x + dt * v)
    return x, v


def correct_terms(dt, f, r0, r1, d0, d1, m, vh, fixed, pres, vbar, start=False):
    """(a, v, terms) of the corrector: terms[name] holds the per-dof terms of the six sums of the ledger, before their
    factors (the sums the device forms)"""
    T = vh.dtype.type
    hdt = T(0.5) * T(dt)
    free = ~fixed & ~pres
    zero = np.zeros_like(vh)
    f = zero if f is None else f
    d1 = zero if d1 is None else d1
    d0 = zero if d0 is None else d0
    a = np.where(free, ((f - r1) - d1) / np.where(free, m, T(1)), T(0))
    v = np.where(free, vh if start else vh + hdt * a, np.where(pres, vbar, T(0)))
    terms = dict(mv2=np.where(fixed, T(0), (m * v) * v), ma2=np.where(free, (m * a) * a, T(0)))
    if not start:
        vv = np.where(pres, vbar, vh)
        terms["int"] = np.where(fixed, T(0), (r0 + r1) * vv)
        terms["damp"] = np.where(free, (d0 + d1) * vh, T(0))
        terms["load"] = np.where(free, f * vh, T(0))
        terms["react"] = np.where(pres, (r0 + r1) * vbar, T(0))
    return a, v, terms


class Stepper:
    """the scheme around a force function: force(x) -> r (raw, of every dof), damping(v) -> d or None, commit(x) the state
    commit after a step.  Sums in the arrays' own type, numpy's order."""

    def __init__(self, m, fixed=None, pres=None, vbar=None, dtype=np.float64):
        self.T = np.dtype(dtype).type
        self.m = np.asarray(m, dtype=dtype)
        n = len(self.m)
        self.fixed, self.pres, self.free = masks(fixed, pres, n)
        self.vbar = np.zeros(n, dtype=dtype) if vbar is None else np.asarray(vbar, dtype=dtype)

    def start(self, x, v, f, force, damping=None, commit=None):
        T = self.T
        self.force, self.damping, self.commit = force, damping, commit
        self.x, self.f = np.asarray(x, dtype=T).copy(), (None if f is None else np.asarray(f, dtype=T))
        self.r = np.asarray(force(self.x), dtype=T)
        v = np.asarray(v, dtype=T)
        self.d = None if damping is None else np.asarray(damping(np.where(self.free, v, np.where(self.pres, self.vbar, T(0)))), dtype=T)
        self.a, self.v, t = correct_terms(0.0, self.f, None, self.r, None, self.d, self.m, v, self.fixed, self.pres, self.vbar, start=True)
        self.mv2, self.ma2 = t["mv2"].sum(), t["ma2"].sum()
        self.W_int = self.W_ext = self.W_damp = T(0)
        self.steps = 0
        return self

    def step(self, dt):
        T = self.T
        dt = T(dt)
        hdt = T(0.5) * dt
        self.x, vh = predict(dt, self.x, self.v, self.a, self.fixed, self.pres, self.vbar)
        r1 = np.asarray(self.force(self.x), dtype=T)
        d1 = None if self.damping is None else np.asarray(self.damping(vh), dtype=T)
        self.a, self.v, t = correct_terms(dt, self.f, self.r, r1, self.d, d1, self.m, vh, self.fixed, self.pres, self.vbar)
        self.r, self.d = r1, d1
        self.mv2, self.ma2 = t["mv2"].sum(), t["ma2"].sum()
        self.W_int = self.W_int + hdt * t["int"].sum()
        self.W_damp = self.W_damp + hdt * t["damp"].sum()
        self.W_ext = self.W_ext + (dt * t["load"].sum() + hdt * t["react"].sum())
        if self.commit is not None:
            self.commit(self.x)
        self.steps += 1

    def energies(self, dt):
        T = self.T
        ke, q = T(0.5) * self.mv2, (T(dt) * T(dt) * T(0.125)) * self.ma2
        return dict(KE=ke, W_int=self.W_int, W_ext=self.W_ext, W_damp=self.W_damp, Q=q,
                    E_star=ke - q + self.W_int + self.W_damp - self.W_ext)
