"""The kernels of the explicit step (mimi_amd/csrc/explicit.hip through mimi_amd.explicit.ExplicitStepper) on synthetic
vectors against the numpy restatement of tests/_explicit_reference.py.

Updates: elementwise within 4 x 2^-53 x sum|terms| of the float64 restatement (the kernels contract nothing, so the two make
the same roundings; the bar leaves room for a division that is rounded otherwise).  Sums: against long double, within
(run length + tree depth + 2) x 2^-53 x sum|terms| with the constants the library exports (mimi_amd.explicit.sum_run_length
says where each unit goes).  A work after a second step has passed through one more addition, that of the running value:
one more unit there."""
import functools

import numpy as np
import pytest

import _explicit_reference as er

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble


def lengths():
    from mimi_amd import explicit
    trip = explicit.SUM_GRID_CAP * explicit.SUM_BLOCK
    # one workgroup and less, two workgroups, several, an odd length past a full trip of the grid-stride loop
    return [1, 63, 257, 4099, trip + 77]


MASKS = ["none", "fixed", "prescribed", "both", "mixed"]


@functools.lru_cache(maxsize=None)
def inputs(n, kind):
    rng = np.random.default_rng(1000 * MASKS.index(kind) + n % 997)
    if kind == "mixed":
        code = rng.integers(0, 4, n)
    else:
        code = np.full(n, {"none": 0, "fixed": 1, "prescribed": 2, "both": 3}[kind])
    c = dict(fixed=(code & 1).astype(np.uint8), pres=((code >> 1) & 1).astype(np.uint8), vbar=rng.uniform(-1, 1, n),
             m=rng.uniform(0.5, 2.0, n), x=rng.standard_normal(n), v=rng.standard_normal(n), f=rng.standard_normal(n),
             r=[3.0 * rng.standard_normal(n) for _ in range(3)], d=[0.5 * rng.standard_normal(n) for _ in range(3)])
    # a mass that must not matter where the dof is not free
    c["m"][(code == 1)] = -1.0
    for a in list(c.values()):
        for b in (a if isinstance(a, list) else [a]):
            b.setflags(write=False)
    return c


def device(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def run(n, kind, damping, dts=(0.013, 0.007)):
    """start and two steps on the device; what the host saw after each call"""
    from mimi_amd.explicit import ExplicitStepper
    c = inputs(n, kind)
    s = ExplicitStepper(n, c["fixed"], c["pres"], c["vbar"]).Prepare()
    m, x, v, f = device(c["m"]), device(c["x"]), device(c["v"]), device(c["f"])
    r = [device(a) for a in c["r"]]
    d = [device(a) for a in c["d"]] if damping else [None] * 3
    import torch
    a = torch.empty_like(x)
    s.SetMass(m)
    s.Synchronize()
    out = []
    snap = lambda dt: dict(x=x.cpu().numpy(), v=v.cpu().numpy(), a=s.Acceleration(a).cpu().numpy(), e=s.Energies(dt),
                           prev=s.PreviousForcePointers())
    s.Start(v, f, r[0], d[0])
    out.append(snap(dts[0]))
    assert out[-1]["prev"] == (r[0].data_ptr(), d[0].data_ptr() if damping else 0)
    for k, dt in enumerate(dts):
        s.Predict(dt, x, v)
        out.append(dict(x=x.cpu().numpy(), v=v.cpu().numpy()))
        s.Correct(dt, f, r[k + 1], d[k + 1], v)
        out.append(snap(dt))
        # the swap: the handle now reads the caller's buffer of this step, by pointer
        assert out[-1]["prev"] == (r[k + 1].data_ptr(), d[k + 1].data_ptr() if damping else 0)
    assert s.Info(3) == len(dts) and s.Info(0) == n
    # nobody wrote into the force vectors
    for k in range(3):
        assert np.array_equal(r[k].cpu().numpy(), c["r"][k])
    return out


def close(got, want, bar, what):
    err = np.abs(got - want)
    assert np.all(err <= bar), f"{what}: {float((err - bar).max()):.3e} over the bar at {int(np.argmax(err - bar))}"


def check_sums(e, dt, terms, n, what, extra=0):
    """the six numbers against long-double sums of the per-dof terms (formed in long double from the device's own a and v)"""
    from mimi_amd import explicit
    units = explicit.sum_run_length(n) + explicit.SUM_TREE_DEPTH + 2
    dt = LD(dt)
    hdt = dt / 2
    want = dict(KE=terms["mv2"].sum() / 2, Q=dt * dt / 8 * terms["ma2"].sum())
    mass = dict(KE=np.abs(terms["mv2"]).sum() / 2, Q=dt * dt / 8 * np.abs(terms["ma2"]).sum())
    if "int" in terms:
        want.update(W_int=hdt * terms["int"].sum(), W_damp=hdt * terms["damp"].sum(),
                    W_ext=dt * terms["load"].sum() + hdt * terms["react"].sum())
        mass.update(W_int=hdt * np.abs(terms["int"]).sum(), W_damp=hdt * np.abs(terms["damp"]).sum(),
                    W_ext=dt * np.abs(terms["load"]).sum() + hdt * np.abs(terms["react"]).sum())
    else:
        want.update(W_int=LD(0), W_damp=LD(0), W_ext=LD(0))
        mass.update(W_int=LD(0), W_damp=LD(0), W_ext=LD(0))
    for k in want:
        err, bar = abs(LD(e[k]) - want[k]), (units + extra) * U * mass[k]
        print(f"{what} {k}: error {float(err):.3e} bar {float(bar):.3e}")
        assert err <= bar, (what, k, float(err), float(bar))
    return want, mass


def ld(c, key):
    return np.asarray(c[key], dtype=LD)


@pytest.mark.parametrize("damping", [True, False], ids=["damped", "undamped"])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", lengths())
def test_start_predict_correct_energies(n, kind, damping):
    c = inputs(n, kind)
    fixed, pres, free = er.masks(c["fixed"], c["pres"], n)
    out = run(n, kind, damping)
    d = c["d"] if damping else [None] * 3
    zero = np.zeros(n)
    # ---- start
    a0, v0, _ = er.correct_terms(0.0, c["f"], None, c["r"][0], None, d[0], c["m"], c["v"], fixed, pres, c["vbar"], start=True)
    mfree = np.where(free, c["m"], 1.0)
    bar_a = np.where(free, 4 * U * (np.abs(c["f"]) + np.abs(c["r"][0]) + np.abs(zero if d[0] is None else d[0])) / mfree, 0.0)
    close(out[0]["a"], a0, bar_a, "a_0")
    assert np.array_equal(out[0]["v"], v0) and np.array_equal(out[0]["x"], c["x"])
    _, _, t = er.correct_terms(0.0, ld(c, "f"), None, np.asarray(c["r"][0], dtype=LD), None, None if d[0] is None else np.asarray(d[0], dtype=LD),
                               ld(c, "m"), np.asarray(out[0]["v"], dtype=LD), fixed, pres, ld(c, "vbar"), start=True)
    t["ma2"] = np.where(free, ld(c, "m") * np.asarray(out[0]["a"], dtype=LD) ** 2, LD(0))
    check_sums(out[0]["e"], 0.013, t, n, "start")
    # ---- two steps, each from the device's own state before it
    state = out[0]
    W = dict(W_int=LD(0), W_damp=LD(0), W_ext=LD(0))
    Wm = dict(W)
    for k, dt in enumerate((0.013, 0.007)):
        pred, corr = out[1 + 2 * k], out[2 + 2 * k]
        x1, vh = er.predict(dt, state["x"], state["v"], state["a"], fixed, pres, c["vbar"])
        hdt = 0.5 * dt
        close(pred["v"], vh, 4 * U * (np.abs(state["v"]) + hdt * np.abs(state["a"])), f"predict v step {k}")
        x_from_v = np.where(fixed, state["x"], state["x"] + dt * pred["v"])
        close(pred["x"], x_from_v, 4 * U * (np.abs(state["x"]) + dt * np.abs(pred["v"])), f"predict x step {k}")
        # fixed dofs are untouched bit for bit, prescribed ones move by exactly dt vbar in the host's arithmetic
        assert np.array_equal(pred["x"][fixed], state["x"][fixed]) and np.all(pred["v"][fixed] == 0.0)
        assert np.array_equal(pred["v"][pres], c["vbar"][pres])
        assert np.array_equal(pred["x"][pres], (state["x"] + dt * c["vbar"])[pres])
        a1, v1, _ = er.correct_terms(dt, c["f"], c["r"][k], c["r"][k + 1], d[k], d[k + 1], c["m"], pred["v"], fixed, pres, c["vbar"])
        dk = zero if d[k + 1] is None else d[k + 1]
        bar_a = np.where(free, 4 * U * (np.abs(c["f"]) + np.abs(c["r"][k + 1]) + np.abs(dk)) / mfree, 0.0)
        close(corr["a"], a1, bar_a, f"a step {k}")
        v_from_a = np.where(free, pred["v"] + hdt * corr["a"], np.where(pres, c["vbar"], 0.0))
        close(corr["v"], v_from_a, 4 * U * (np.abs(pred["v"]) + hdt * np.abs(corr["a"])), f"correct v step {k}")
        assert np.array_equal(corr["x"], pred["x"])
        assert np.all(corr["a"][~free] == 0.0)
        asLD = lambda z: None if z is None else np.asarray(z, dtype=LD)
        _, _, t = er.correct_terms(dt, ld(c, "f"), asLD(c["r"][k]), asLD(c["r"][k + 1]), asLD(d[k]), asLD(d[k + 1]), ld(c, "m"),
                                   asLD(pred["v"]), fixed, pres, ld(c, "vbar"))
        t["mv2"] = np.where(fixed, LD(0), ld(c, "m") * asLD(corr["v"]) ** 2)
        t["ma2"] = np.where(free, ld(c, "m") * asLD(corr["a"]) ** 2, LD(0))
        if k == 0:
            want, mass = check_sums(corr["e"], dt, t, n, "step 0")
            for key in W:
                W[key], Wm[key] = want[key], mass[key]
        else:
            # KE and Q are this step's alone; a work is the running value plus this step's increment: one more addition
            from mimi_amd import explicit
            units = explicit.sum_run_length(n) + explicit.SUM_TREE_DEPTH + 2
            ldt = LD(dt)
            inc = dict(W_int=ldt / 2 * t["int"].sum(), W_damp=ldt / 2 * t["damp"].sum(), W_ext=ldt * t["load"].sum() + ldt / 2 * t["react"].sum())
            incm = dict(W_int=ldt / 2 * np.abs(t["int"]).sum(), W_damp=ldt / 2 * np.abs(t["damp"]).sum(),
                        W_ext=ldt * np.abs(t["load"]).sum() + ldt / 2 * np.abs(t["react"]).sum())
            for key in W:
                err = abs(LD(corr["e"][key]) - (W[key] + inc[key]))
                bar = (units + 1) * U * (Wm[key] + incm[key])
                assert err <= bar, (key, float(err), float(bar))
            for key, name in (("KE", "mv2"), ("Q", "ma2")):
                fac = LD(0.5) if key == "KE" else ldt * ldt / 8
                assert abs(LD(corr["e"][key]) - fac * t[name].sum()) <= units * U * fac * np.abs(t[name]).sum()
        e = corr["e"]
        assert e["E_star"] == e["KE"] - e["Q"] + e["W_int"] + e["W_damp"] - e["W_ext"]
        if not damping:
            assert e["W_damp"] == 0.0
        state = corr


@pytest.mark.parametrize("n", [4099, lengths()[-1]])
def test_two_runs_give_equal_bytes(n):
    a, b = run(n, "mixed", True), run(n, "mixed", True)
    for sa, sb in zip(a, b):
        for key in ("x", "v", "a"):
            if key in sa:
                assert sa[key].tobytes() == sb[key].tobytes()
        if "e" in sa:
            assert np.array([sa["e"][k] for k in sorted(sa["e"])]).tobytes() == np.array([sb["e"][k] for k in sorted(sb["e"])]).tobytes()


def test_refusals():
    import torch
    from mimi_amd.explicit import ExplicitStepper
    n = 300
    fixed, pres = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    fixed[5] = 1
    pres[9] = 1
    s = ExplicitStepper(n, fixed, pres, np.ones(n)).Prepare()
    x, v, f, r, r2 = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(5))
    m = torch.ones(n, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="start before set_mass"):
        s.Start(v, f, r)
    # a non-positive mass: tolerated on the fixed dof, refused on a free or a prescribed one (seen on the device, reported at the next wait)
    m[5] = 0.0
    s.SetMass(m)
    s.Synchronize()
    m[17] = 0.0
    s.SetMass(m)
    with pytest.raises(RuntimeError, match="not positive on a free or constant-velocity dof"):
        s.Synchronize()
    m[17] = 1.0
    m[9] = -2.0                 # a prescribed dof's mass enters KE
    s.SetMass(m)
    with pytest.raises(RuntimeError, match="not positive on a free or constant-velocity dof"):
        s.Synchronize()
    m[9] = 1.0
    s.SetMass(m)
    s.Synchronize()
    with pytest.raises(RuntimeError, match="correct before start"):
        s.Correct(0.1, f, r, None, v)
    with pytest.raises(RuntimeError, match="predict before start"):
        s.Predict(0.1, x, v)
    s.Start(v, f, r)
    # host pointers
    hx = np.zeros(n)
    with pytest.raises(RuntimeError, match="host pointer"):
        s.Predict(0.1, hx, v)
    with pytest.raises(RuntimeError, match="host pointer"):
        s.Correct(0.1, f, np.zeros(n), None, v)
    with pytest.raises(RuntimeError, match="host pointer"):
        s.SetMass(np.ones(n))
    # the buffer of the previous step again; a damping force that was not there at start
    with pytest.raises(RuntimeError, match="alternate two buffers"):
        s.Correct(0.1, f, r, None, v)
    with pytest.raises(RuntimeError, match="in every call since start, or in none"):
        s.Correct(0.1, f, r2, x, v)
    s.Correct(0.1, f, r2, None, v)
    s.Synchronize()
    with pytest.raises(ValueError):
        ExplicitStepper(n, np.zeros(n + 1, dtype=np.uint8))
    with pytest.raises(RuntimeError, match="needs the prescribed velocities"):
        ExplicitStepper(n, None, fixed, None).Prepare()
