"""Coulomb friction on the matrix-free route (csrc/kernels_face_friction_action.hpp) through the C ABI:
MortarContact.SetFrictionAction / Linearize / ApplyTangent, the Krylov solvers' boundary term and the facade's
"friction_matrix_free" flag.  Inputs: the staged history of tests/_friction_cases.py on the device (commit at u0, Linearize at
u1), on its small faces and nothing larger; tests/test_friction_action_cpu.py asserts what those cases give.

(1) the frozen and the consistent action with friction on every case, kind of body and face, two vectors per face, against the
    long-double reference of tests/_friction_action_reference.py: |y - K v|_inf / max_i (|K| |v|)_i within
    _face_cases.TOL["contact_K"] (1e-11), the bar of the assembled tangent; the frozen action also against the handle's own
    assembled tangent (AddBoundaryResidualAndGrad at u1) applied to v on the host, on the same bar;
(2) the consistent action is the derivative of the device's own residual: (r(u1 + h v) - r(u1 - h v)) / 2 h from
    AddBoundaryResidual (trial state only), h = 1e-6, within 10 x _friction_action_cases.F64_WORST; the frozen action with
    friction misses that bar by more than WIDE;
(3) semantics: the action off, mu = 0 with the action on, equal bytes, accumulation, host and device arguments, the bytes of
    record, the snapshot, the friction state left alone, a far-away body, sharded handles;
(4) GMRES with the Kronecker preconditioner on rho M + fac0 K plus the contact action with friction against the
    extended-precision solve of the assembled Jacobian (friction in the CSR), and for the consistent action of that Jacobian
    plus the reference's dense new parts;
(5) the facade: the implicit slide of tests/test_friction_solid_gpu.py on the assembled route, on the matrix-free route with
    "friction_matrix_free", and on the latter with "contact_consistent_tangent".

Worst figures measured on an MI355X: (1) frozen 1.0e-14 (rep3d_p1 order 15, plane), consistent 2.6e-15, against the handle's
assembled tangent 6.6e-16, of the bar 1e-11; (2) 3.7e-10 (rep2d_p3, plane) of the bar 2.4e-9, the frozen action with friction at
least 0.24 away; (5) 71 Newton iterations over the 9 steps on the assembled route, 71 with the frozen friction action (980 GMRES
iterations), 27 with the consistent one (377)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _face_cases as fc
import _face_reference as fr
import _friction_action_cases as fa
import _friction_cases as fx
import _friction_reference as fq
import _kronecker_cases as kc
import _kronecker_reference as ref
from _cases import product_material
from test_boundary_action_cpu import vectors

pytestmark = pytest.mark.gpu
T = fc.TOL


def handle(case, axis, side, order, kind, **friction):
    from test_friction_gpu import handle as make
    return make(case, axis, side, order, kind, **friction)


def dense(case, values):
    from test_friction_gpu import dense as make
    return make(case, values)


def staged(case, axis, side, order, kind, action=True):
    """a handle with the friction of the cases, committed at u0"""
    eps_t = fx.reference(case, axis, side, order, kind).eps_t
    G = handle(case, axis, side, order, kind, friction=fx.MU, tangential_coefficient=eps_t)
    G.BoundaryPostTimeAdvance(fx.displacements(case)[0])
    if action:
        G.SetFrictionAction(True)
    return G


def action(G, v, factor=1.0):
    """the increment of ApplyTangent in accumulate form on a random y0"""
    y0 = np.random.default_rng(11).standard_normal(len(v))
    y = y0.copy()
    G.ApplyTangent(np.array(v), y, factor)
    return y - y0


# ---- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fa.KINDS)
@pytest.mark.parametrize("case,order", fa.CASES, ids=lambda c: str(c))
def test_friction_action_against_the_reference(case, order, kind):
    u1 = fx.displacements(case)[1]
    worst = dict(frozen=0.0, consistent=0.0, assembled=0.0)
    for axis, side in fc.faces(case):
        P = fa.products(case, axis, side, order, kind)                 # (its K carries GRAD_FACTOR)
        G = staged(case, axis, side, order, kind)
        # the handle's own assembled tangent, on a twin without the action: G allocates no tangent block
        twin = staged(case, axis, side, order, kind, action=False)
        A = np.zeros(twin.pattern_.nnz)
        twin.AddBoundaryResidualAndGrad(u1, fc.GRAD_FACTOR, np.zeros(len(u1)), A)
        K_dev = dense(case, A)
        twin._history()
        assert (twin.n_stick_, twin.n_slip_) == (int((P.branch == 1).sum()), int((P.branch == 2).sum())) and twin.n_slip_ > 0
        for mode in (False, True):
            G.SetConsistentTangent(mode)
            G.Linearize(u1)
            assert G.HoldsFrictionRecord() and G.HoldsConsistentRecord() == mode and not G.HoldsTangentBlocks()
            for k, v in enumerate(vectors(case, axis, side)):
                y = action(G, v, fc.GRAD_FACTOR)
                if mode:
                    worst["consistent"] = max(worst["consistent"], float(np.abs(y - P.Kv[k]).max() / P.scale[k].max()))
                else:
                    worst["frozen"] = max(worst["frozen"], float(np.abs(y - P.Kv_frozen[k]).max() / P.scale_frozen[k].max()))
                    worst["assembled"] = max(worst["assembled"], float(np.abs(y - K_dev @ v).max() / P.scale_frozen[k].max()))
    print(f"figures friction action {case} order {order} {kind}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert worst["frozen"] <= T["contact_K"]
    assert worst["consistent"] <= T["contact_K"]
    assert worst["assembled"] <= T["contact_K"]


# ---- (2) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fa.KINDS)
@pytest.mark.parametrize("case", fa.FD_CASES)
def test_consistent_action_is_the_derivative_of_the_device_residual(case, kind):
    from test_contact_consistent_gpu import WIDE, device_quotient
    u1 = np.array(fx.displacements(case)[1])
    on, off = 0.0, np.inf
    for axis, side in fc.faces(case):
        P = fa.products(case, axis, side, -1, kind)
        G = staged(case, axis, side, -1, kind)
        before = tuple(a.tobytes() for a in G.FrictionState())
        vs = vectors(case, axis, side)
        quotients = [device_quotient(G, u1, np.array(v), fa.FD_STEP) for v in vs]
        assert tuple(a.tobytes() for a in G.FrictionState()) == before      # (the evaluations wrote trial state only)
        scales = P.scale.max(axis=1) / fc.GRAD_FACTOR
        dev = {}
        for mode in (True, False):
            G.SetConsistentTangent(mode)
            G.Linearize(u1)
            assert G.HoldsFrictionRecord() and G.HoldsConsistentRecord() == mode
            dev[mode] = max(float(np.abs(action(G, v) - q).max() / s) for v, q, s in zip(vs, quotients, scales))
        on, off = max(on, dev[True]), min(off, dev[False])
    bar = 10 * fa.F64_WORST
    print(f"figures device quotient with friction {case} {kind}: consistent {on:.2e} (bar {bar:.2e}), frozen at least {off:.2e}")
    assert on <= bar
    assert off > WIDE * bar


# ---- (3) ---------------------------------------------------------------------------------------------------------------------
SEMANTICS = [("rep3d_p2", 2, 1), ("rep2d_p3", 1, 0)]


@pytest.mark.parametrize("case,axis,side", SEMANTICS)
def test_semantics_of_the_friction_action(case, axis, side):
    import torch
    from mimi_amd import _capi
    from mimi_amd.integrators import MortarContact, RigidPlane
    from test_friction_gpu import pattern_of
    kind, order = "plane", -1
    B = fc.product_patch(case)
    dim = B.dim
    u0, u1, u2 = (np.array(u) for u in fx.displacements(case))
    ref_ = fx.reference(case, axis, side, order, kind)
    v = np.array(vectors(case, axis, side)[0])
    y0 = np.random.default_rng(3).standard_normal(len(v))
    n_q = fc.face_basis(case, axis, side).n_q_face

    def apply(G):
        y = y0.copy()
        G.ApplyTangent(v, y, 0.7)
        return y

    state = lambda G: tuple(a.tobytes() for a in G.FrictionState())

    # the action off: today's refusals, by the front end and by the C entries, and the bytes of an untouched handle
    rough = staged(case, axis, side, order, kind, action=False)
    assert not rough.friction_action_ and not rough.HoldsFrictionRecord()
    for refused in (lambda: rough.Linearize(u1), lambda: rough.ApplyTangent(v, np.zeros_like(v)), lambda: rough.SetConsistentTangent(True)):
        with pytest.raises(RuntimeError, match="friction"):
            refused()
    L = _capi.lib()
    for call in (lambda: L.mimi_hip_contact_linearize(rough._handle(), _capi.fptr(u1)),
                 lambda: L.mimi_hip_contact_apply_tangent(rough._handle(), 1.0, _capi.fptr(v), _capi.fptr(np.zeros_like(v))),
                 lambda: L.mimi_hip_contact_set_consistent_tangent(rough._handle(), 1)):
        with pytest.raises(RuntimeError, match=r"not available on a contact handle with friction \(mu = 0\.3\): the friction tangent is "
                                                 r"assembled only"):
            _capi.check(call())
    rough.SetFrictionAction(True)
    rough.SetFrictionAction(False)
    with pytest.raises(RuntimeError, match="friction"):
        rough.Linearize(u1)
    untouched = handle(case, axis, side, order, kind)
    untouched.Linearize(u1)
    frozen = apply(untouched)
    n_faces = untouched.n_marked_boundaries_
    n_marked = len(untouched.MarkedNodes())
    frozen_bytes = n_faces * n_q * (1 + (dim - 1) * dim) * 8 + n_faces
    consistent_bytes = n_faces * n_q * (2 + dim + (dim - 1) * dim) * 8 + 16 * n_marked + n_faces
    friction_bytes = n_faces * n_q * (8 * (dim + 1) + 1) + 8
    assert untouched.LinearizationBytes() == frozen_bytes
    off = handle(case, axis, side, order, kind)
    off.SetFrictionAction(False)
    off.Linearize(u1)
    assert np.array_equal(apply(off), frozen) and off.LinearizationBytes() == frozen_bytes and not off.HoldsFrictionRecord()
    # mu = 0 with the action on: the bytes of the frictionless action, frozen and consistent
    smooth = handle(case, axis, side, order, kind)
    smooth.SetFrictionAction(True)
    smooth.Linearize(u1)
    assert np.array_equal(apply(smooth), frozen) and smooth.LinearizationBytes() == frozen_bytes and not smooth.HoldsFrictionRecord()
    untouched.SetConsistentTangent(True)
    untouched.Linearize(u1)
    smooth.SetConsistentTangent(True)
    smooth.Linearize(u1)
    consistent = apply(untouched)
    assert np.array_equal(apply(smooth), consistent) and smooth.LinearizationBytes() == consistent_bytes
    assert not smooth.HoldsFrictionRecord() and not np.array_equal(consistent, frozen)
    # a body whose friction was switched off again records none either
    G = staged(case, axis, side, order, kind)
    G.SetFriction(0.0)
    G.Linearize(u1)
    assert np.array_equal(apply(G), frozen) and not G.HoldsFrictionRecord() and G.LinearizationBytes() == frozen_bytes
    # with friction: two runs give equal bytes, and they are not the frictionless action's
    G = staged(case, axis, side, order, kind)
    assert G.friction_action_ and not G.HoldsFrictionRecord() and G.LinearizationBytes() == 0
    with pytest.raises(RuntimeError, match="before any mimi_hip_contact_linearize"):
        G.ApplyTangent(v, np.zeros_like(v))
    # the friction state and the history are left alone by Linearize + ApplyTangent: an evaluation at u2 wrote the trial state
    twin = staged(case, axis, side, order, kind)
    for H in (G, twin):
        H.AddBoundaryResidual(u2, np.zeros_like(v))
        H._history()
    committed, counts = state(G), (G.n_stick_, G.n_slip_)
    G.Linearize(u1)
    assert G.HoldsFrictionRecord() and not G.HoldsConsistentRecord() and G.LinearizationBytes() == frozen_bytes + friction_bytes
    runs = [apply(G), apply(G)]
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], frozen) and np.abs(runs[0] - y0).max() > 0
    G._history()
    assert state(G) == committed and (G.n_stick_, G.n_slip_) == counts and state(twin) == committed
    G.CommitFriction()
    twin.CommitFriction()
    assert state(G) == state(twin) and state(G) != committed           # (the trial state of u2, untouched)
    # ... and the record is still the one of the state committed at u0
    assert np.array_equal(apply(G), runs[0])
    # accumulation: what a zero y gets is the increment (one addition per entry, off the face none)
    z = np.zeros_like(v)
    G.ApplyTangent(v, z, 0.7)
    assert np.array_equal(y0 + z, runs[0]) and np.any(z == 0)
    # device arguments
    G = staged(case, axis, side, order, kind)
    dev = torch.device("cuda", 0)
    G.Linearize(torch.from_numpy(u1).to(dev))
    yd = torch.from_numpy(y0.copy()).to(dev)
    G.ApplyTangent(torch.from_numpy(v).to(dev), yd, 0.7)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), runs[0]) and np.array_equal(apply(G), runs[0])
    # the consistent record with friction: its bytes, and another action
    G.SetConsistentTangent(True)
    assert G.consistent_tangent_
    G.Linearize(u1)
    expect = consistent_bytes + friction_bytes
    assert G.LinearizationBytes() == expect and G.HoldsConsistentRecord() and G.HoldsFrictionRecord() and not G.HoldsTangentBlocks()
    full = [apply(G), apply(G)]
    assert np.array_equal(full[0], full[1]) and not np.array_equal(full[0], runs[0]) and not np.array_equal(full[0], consistent)
    # the snapshot survives whatever else the handle does
    G.SetFriction(0.5, 3.0 * ref_.eps_t)
    G.SetBodyIncrement(ref_.d)
    G.UpdateBody(penalty=3.0 * fc.PENALTY)
    G.GapNorm(1.7 * u1)
    G.AddBoundaryResidual(u2, np.zeros_like(v))
    G.CommitFriction()
    G.BoundaryPostTimeAdvance(u1)
    assert np.array_equal(apply(G), full[0]) and G.LinearizationBytes() == expect
    G.ResetFriction()
    G.SetConsistentTangent(False)
    assert np.array_equal(apply(G), full[0]) and G.HoldsFrictionRecord() and G.HoldsConsistentRecord()
    # ... and a new linearisation reads the handle as it is now: after the reset no point is in contact, so none carries a traction
    G.Linearize(u1)
    now = apply(G)
    assert G.HoldsFrictionRecord() and not G.HoldsConsistentRecord() and not np.array_equal(now, runs[0])
    plain = handle(case, axis, side, order, kind)
    plain.UpdateBody(penalty=3.0 * fc.PENALTY)
    plain.Linearize(u1)
    smooth_now = apply(plain)                                           # (every branch 0: the frictionless action's values)
    assert np.abs(now - smooth_now).max() <= 1e-13 * np.abs(smooth_now - y0).max()
    # a far-away body: y keeps its bits
    pts = fc.points(case, axis, side).x.astype(np.float64)
    normal = np.zeros(dim)
    normal[0] = 1.0
    far = MortarContact(RigidPlane(list(pts.min(axis=0) - 100.0), list(normal), fc.PENALTY, friction=fx.MU), "contact",
                        pattern_of(case)[0], B, axis, side).Prepare()
    far.BoundaryPostTimeAdvance(u0)
    far.SetFrictionAction(True)
    for mode in (False, True):
        far.SetConsistentTangent(mode)
        far.Linearize(u1)
        assert far.HoldsFrictionRecord() and np.array_equal(apply(far), y0)
    # the reference-FD tangent mode stays refused
    from mimi_amd.integrators import TANGENT_REFERENCE_FD
    with pytest.raises(RuntimeError, match="friction"):
        G.SetTangentMode(TANGENT_REFERENCE_FD)
    with pytest.raises(RuntimeError, match="reference-FD tangent mode is not available"):
        _capi.check(L.mimi_hip_contact_set_tangent_mode(G._handle(), TANGENT_REFERENCE_FD))


def test_a_sharded_contact_is_refused():
    G = handle("rep2d_p3", 1, 0, -1, "plane")
    G.sharded_ = True
    with pytest.raises(RuntimeError, match="ShardedContact"):
        G.SetFrictionAction(True)
    assert not G.friction_action_
    G.SetFrictionAction(False)


# ---- (4) ---------------------------------------------------------------------------------------------------------------------
def _rough_contact_system(name, fac0):
    """test_contact_consistent_gpu.py::_contact_system with friction on the plane: the state is committed at 0.8 u, the Jacobian
    is assembled at u with friction in the CSR.  The tangential penalty is sized on the reference's points so that stick and
    slip both occur (the cut of tests/_friction_cases.py)."""
    from mimi_amd.integrators import CSRPattern, MortarContact, NonlinearSolid, RigidPlane
    from test_kronecker_gpu import _kronecker_solver
    P, B = kc.solve_patch(name)
    ess, u, b = kc.solve_inputs(name)
    u = np.array(u)
    u_commit = 0.8 * u
    rowptr, col = P.sparsity()
    pattern = CSRPattern(rowptr.astype(np.int64), col.astype(np.int32), len(col))
    G = NonlinearSolid("domain", product_material("neohook"), pattern, patch=B).Prepare()
    G.dt_ = 1.0
    x = B.control_points + u.reshape(-1, P.dim)
    top = x[:, 2] >= x[:, 2].max() - 0.35 * (x[:, 2].max() - x[:, 2].min())
    body = dict(kind="plane", point=[0.0, 0.0, float(x[top, 2].mean())], normal=[0.0, 0.0, -1.0])
    # the reference's side: the state committed at 0.8 u and the sizing of eps_T at u
    fb = fr.face_basis(B.degrees, B.knots, 2, 1)
    X = B.control_points.astype(np.longdouble)
    pts = [fr.face_points(fb, X + w.reshape(-1, P.dim).astype(np.longdouble)) for w in (u_commit, u)]
    con = [fr.mortar_contact(p, body, 1e4, with_tangent=False) for p in pts]
    committed = fq.evaluate(pts[0], con[0], fq.initial_state(len(pts[0].x), P.dim), fx.MU, 1.0, with_tangent=False).trial
    tr = fq.tractions(pts[1], fq.point_pressure(pts[1], con[1]), committed, fx.MU, 1.0)
    assert tr.on.sum() >= 2
    cut, margin = fx._cut((tr.sn[tr.on] / tr.pn[tr.on]).astype(np.float64))
    eps_t = float(fx.MU / cut)
    tr = fq.tractions(pts[1], fq.point_pressure(pts[1], con[1]), committed, fx.MU, eps_t)
    counts = (int((tr.branch == 1).sum()), int((tr.branch == 2).sum()))
    assert margin > 1e-6 and min(counts) > 0
    contact = MortarContact(RigidPlane(body["point"], body["normal"], 1e4, friction=fx.MU, tangential_coefficient=eps_t), "contact",
                            pattern, B, 2, 1).Prepare()
    contact.BoundaryPostTimeAdvance(u_commit)
    vals = np.zeros(len(col))
    G.AddMass(kc.RHO, vals)
    G.AddDomainResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    before = vals.copy()
    contact.AddBoundaryResidualAndGrad(u, fac0, np.zeros(P.n_vdofs), vals)
    contact._history()
    assert contact.last_area_ > 0 and np.abs(vals - before).max() > 0 and (contact.n_stick_, contact.n_slip_) == counts
    S = _kronecker_solver(pattern, B, ess, P.dim, kc.RHO, kc.stiff(P.dim, fac0))
    S.Eliminate(None, vals)
    J = sp.csr_matrix((vals, col, rowptr), shape=(P.n_vdofs, P.n_vdofs))
    K_new = fa.dense_new_parts(pts[1], body, 1e4, committed, fx.MU, eps_t, fac0)
    return G, contact, S, J, P, ess, u, b, K_new


def test_gmres_with_the_friction_action():
    name, fac0 = "p2_6x4x2", 1e-2
    G, contact, S, J, P, ess, u, b, K_new = _rough_contact_system(name, fac0)
    assert np.abs(K_new).max() > 0
    keep = np.ones(P.n_vdofs)
    keep[np.asarray(list(ess), dtype=np.int64)] = 0.0
    systems = {False: J.toarray(), True: J.toarray() + keep[:, None] * K_new * keep[None, :]}
    x_ref = {mode: np.array([float(v) for v in ref.solve_extended(A, b)]) for mode, A in systems.items()}
    S.max_iter = 3000
    S.preconditioner = "kronecker"
    nan = lambda: np.full(len(b), np.nan)
    G.Linearize(u)
    contact.SetFrictionAction(True)
    dev = {}
    for mode in (False, True):
        contact.SetConsistentTangent(mode)
        contact.Linearize(u)
        assert contact.HoldsFrictionRecord() and contact.HoldsConsistentRecord() == mode
        S.SetOperator(G, kc.RHO, fac0, 0.0)
        S.AddBoundaryOperator(contact, fac0)
        x = S.Mult(None, b, nan())
        assert S.converged_ and np.isfinite(x).all()
        dev[mode] = np.abs(x - x_ref[mode]).max() / np.abs(x_ref[mode]).max()
        print(f"\n{name} fac0 {fac0:g} with the {'consistent' if mode else 'frozen'} friction action: iterations {S.final_iter_}, x "
              f"deviates {dev[mode]:.3g} (bar {kc.BAR * kc.DEV_SOLVE:.3g})")
    apart = np.abs(x_ref[False] - x_ref[True]).max() / np.abs(x_ref[True]).max()
    print(f"the two systems' solutions are {apart:.3g} apart")
    assert dev[False] <= kc.BAR * kc.DEV_SOLVE
    assert dev[True] <= kc.BAR * kc.DEV_SOLVE
    assert apart > 1e3 * kc.BAR * kc.DEV_SOLVE       # the new parts are in the system: the frozen solution is not its solution


# ---- (5) ---------------------------------------------------------------------------------------------------------------------
def _block(flags):
    """tests/test_friction_solid_gpu.py::block with runtime flags"""
    import mimi_amd as mimi
    import _explicit_cases as ec
    from mimi_amd.integrators import RigidPlane
    from test_friction_solid_gpu import DOWN, DT, MU, PENALTY
    B = mimi.BSplinePatch.block((4, 2), 2, lengths=(4.0, 2.0))
    probe = ec.facade("sq_p2", "neohook", setup=False)
    bottom = [a - 1 for a, f in probe._faces.items() if f == (1, 0)][0]
    top = [a - 1 for a, f in probe._faces.items() if f == (1, 1)][0]
    plane = RigidPlane([0.0, 0.0], [0.0, 1.0], PENALTY, friction=MU)

    def configure(bc):
        bc.initial.constant_velocity(top, 0, 0.0)
        bc.initial.constant_velocity(top, 1, -DOWN[1] / DT)
        bc.current.contact(bottom, plane)
    nl = ec.facade("sq_p2", "neohook", flags=flags, configure=configure, setup=False)
    nl.patch = lambda: B
    nl.time_step_size = DT
    nl.setup(1)
    nl.configure_newton("nonlinear_solid", 1e-10, 1e-9, 40, False)
    return nl, plane


def test_facade_slide_on_the_matrix_free_routes():
    from test_boundary_action_gpu import MATRIX_FREE
    from test_friction_solid_gpu import DOWN, slide
    free = MATRIX_FREE + [("friction_matrix_free", 1)]
    routes = {}
    for route, flags in (("assembled", ()), ("matrix-free", free), ("consistent", free + [("contact_consistent_tangent", 1)])):
        nl, plane = _block(flags)
        c = nl.contacts_[0]
        assert nl.matrix_free_ == (route != "assembled") and c.friction_action_ == (route != "assembled")
        assert c.consistent_tangent_ == (route == "consistent")
        gmres = [0]
        if nl.matrix_free_:
            mult = nl.linear_.Mult

            def counted(A, *args, mult=mult, nl=nl, gmres=gmres):
                assert A is None
                out = mult(A, *args)
                assert nl.linear_.converged_
                gmres[0] += nl.linear_.final_iter_
                return out
            nl.linear_.Mult = counted
        log, xs = [], []
        x = slide(nl, plane, log)
        for phase, h, *_ in log:
            assert h["converged"], (route, phase, h)
        newton = sum(h["iterations"] for _, h, *_ in log)
        print(f"\nslide with friction, {route}: Newton iterations {newton} over {len(log)} steps, GMRES iterations {gmres[0]}; "
              f"stick / slip at the end {c.n_stick_} / {c.n_slip_}")
        if nl.matrix_free_:
            assert c.HoldsFrictionRecord() and c.HoldsConsistentRecord() == (route == "consistent") and not c.HoldsTangentBlocks()
        assert abs(log[DOWN[0] - 1][2]) > 0.0 and any(e[6] > 0 for e in log)    # the plane was reached, and points slipped
        routes[route] = (x, [(entry[5], entry[6]) for entry in log], c.FrictionState())
    x_a, counts_a, state_a = routes["assembled"]
    assert np.abs(x_a).max() > 0
    for route in ("matrix-free", "consistent"):
        x, counts, state = routes[route]
        assert np.allclose(x, x_a), route
        assert counts == counts_a, route
        xi, xbar, c = state
        assert np.array_equal(c, state_a[2]) and np.allclose(xbar, state_a[1]) and np.allclose(xi, state_a[0], atol=1e-8 * np.abs(state_a[1]).max())
