"""The cases of the status-word tests (tests/_status_cases.py) checked without a GPU: the conditions on the inputs hold on the
long-double reference, and the oracle (oracle/ref_path.py, whose `_check` raises on a non-zero status of ScalarSolve) raises
exactly where the reference's predicate "some point yields" says a softening law must fail -- so the expectation that
tests/test_status_gpu.py holds the kernels to is pinned from two independent sides before a device sees it.

  1. `conditions` per (shape, model, field): every point's trial q outside 0.9 - 1.1 of the yield stress, quiet without a
     yielding point, a corner field's yielding points in its element only, many with 20 - 80 %, det F > 0.5.  The figures are
     those written next to _status_cases.FIELDS (-s prints them).
  2. the oracle's add_domain_residual, add_domain_residual_and_grad (TANGENT_EXACT) and domain_post_time_advance on a fresh
     virgin integrator per call: RuntimeError exactly on the fields the predicate marks, for the three models and the three
     softening laws; never under the hardening control.
  3. flat2d_p4 is not served by the oracle (its tables are the reference's own, there is no oracle integrator over flat
     tables); only the predicate is checked there.
  4. the facade's problem of tests/test_status_solid_gpu.py on the oracle's own GeneralizedAlpha2: the first step throws under
     the softening law (the reference would throw out of StepTime2) and leaves part of the points plastic under the control.
Bit 2 of the status word (not converged in 100 iterations) is reached by no finite input: the argument is in the docstring of
tests/_status_cases.py."""
import numpy as np
import pytest

import _domain_cases as dc
import _status_cases as sc

ORACLE_SHAPES = [s for s in sc.SHAPES if not dc.arrays(s).flat]


def test_the_shapes_are_one_per_family_plus_flat_tables():
    assert [dc.arrays(s).family for s in sc.SHAPES] == ["tensor_small", "tensor_p2_two_phase", "tensor_p3_two_phase", "general", "general"]
    assert set(sc.FAMILY_SHAPES) <= set(ORACLE_SHAPES) and [s for s in sc.SHAPES if s not in ORACLE_SHAPES] == ["flat2d_p4"]
    assert dc.BOX_CASE in sc.SHAPES


@pytest.mark.parametrize("name", sc.FIELD_NAMES)
@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_conditions_on_the_inputs(shape, model, name):
    bad, fig = sc.conditions(shape, model, name)
    print(f"{shape} {model} {name}: {fig['yielding']} / {fig['points']} points yield, nearest ratios {fig['below']:.3f} | {fig['above']:.3f}, "
          f"min det F {fig['min_det_F']:.3f}")
    assert not bad, bad
    # every softening law fails on exactly these fields, the control on none: the table the other tests read
    for law in sc.LAWS:
        assert sc.expected_to_raise(shape, model, law, name) == (law != sc.CONTROL_LAW and name != "quiet")


def test_the_fields_of_a_shape_serve_the_three_models_alike():
    """one set of yielding points per (shape, field), whatever the model: the GPU tests then need one table"""
    for shape in sc.SHAPES:
        for name in sc.FIELD_NAMES:
            sets = [sc.predicate(shape, m, name).yields for m in sc.MODELS]
            assert all(np.array_equal(sets[0], s) for s in sets[1:]), (shape, name)


def test_the_corner_fields_of_the_box_case_fall_into_one_box_each():
    """dc.BOXES cut col8_p2 into the elements [0, 3) and [3, 8) of every column: element 0 lies in the first, the last element
    in the second"""
    import _domain_reference as dr
    sp = dc.geometry(dc.BOX_CASE).sp
    for name, owner in (("corner_first", 0), ("corner_last", 1)):
        y = sc.predicate(dc.BOX_CASE, "j2", name).yields
        inside = [bool(y[dr.in_box(sp, b, e)].any()) for b, e in dc.BOXES]
        assert inside == [owner == 0, owner == 1]


def _oracle_raises(shape, model, law, name, entry):
    from oracle import ref_path as rp
    a = dc.arrays(shape)
    D = rp.DomainOracle(dc.oracle_patch(shape), sc.oracle_material(model, law), quadrature_order=a.order)
    D.set_dt(sc.DT)
    u = sc.field(shape, name)
    try:
        if entry == "residual":
            D.add_domain_residual(u, np.zeros(a.n_vdofs))
        elif entry == "residual_and_grad":
            D.add_domain_residual_and_grad(u, dc.GRAD_FACTOR, np.zeros(a.n_vdofs), np.zeros(D.nnz), rp.TANGENT_EXACT)
        else:
            D.domain_post_time_advance(u)
    except RuntimeError as e:
        assert "ScalarSolve" in str(e)
        return True
    return False


ENTRIES = ("residual", "residual_and_grad", "post_time_advance")


@pytest.mark.parametrize("law", sc.SOFT_LAWS + (sc.CONTROL_LAW,))
@pytest.mark.parametrize("model", sc.MODELS)
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_the_oracle_raises_exactly_where_the_reference_says(shape, model, law):
    for name in sc.FIELD_NAMES:
        want = sc.expected_to_raise(shape, model, law, name)
        for entry in ENTRIES:
            assert _oracle_raises(shape, model, law, name, entry) == want, (shape, model, law, name, entry)


def test_the_oracle_step_throws():
    """sq_p2 under SOLID_BODY_FORCE, one step of SOLID_STEP from rest (oracle/harness.py: Operator, GeneralizedAlpha2)"""
    import _explicit_cases as ec
    from oracle import harness as hz, ref_path as rp
    P = ec.oracle_patch(sc.SOLID_CASE)

    def step(law):
        D = rp.DomainOracle(P, sc.oracle_material("j2", law))
        op = hz.Operator(D, D.rowptr, D.col, hz.assemble_mass(P, D.tables, 1.0, D.rowptr, D.col),
                         hz.assemble_body_force(P, D.tables, [sc.SOLID_BODY_FORCE, 0.0]), np.nonzero(ec.clamped_bottom(P))[0])
        ode = hz.GeneralizedAlpha2(op, 0.5, dict(rel_tol=1e-12, abs_tol=1e-8, max_iter=10, iterative_mode=False))
        ode.step(np.zeros(P.n_vdofs), np.zeros(P.n_vdofs), 0.0, sc.SOLID_STEP)
        return D.eqps

    with pytest.raises(RuntimeError, match="ScalarSolve"):
        step(sc.MAIN_LAW)
    eqps = step(sc.CONTROL_LAW)
    print(f"control: eqps max {eqps.max():.3e}, plastic share {(eqps > 0).mean():.3f}")
    assert eqps.max() > 1e-3 and 0.05 < (eqps > 0).mean() < 0.95
