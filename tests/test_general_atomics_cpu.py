"""The cases of tests/test_general_atomics_gpu.py (the atomics fallback of the general path) vetted without a GPU, as
tests/test_domain_reference_cpu.py vets the others: the reference alone decides that the inputs are fair.

  1. long2d_p1_o3 and the one seam pair that is not among dc.PAIRS (mix3d_322 with j2simo): the conditions of
     _domain_cases.conditions (det F > 0.25 at every point, plastic shares, the solver's stop), at most 3100 points, and the
     oracle within MARGIN of the bars against the long-double reference (the solver laws: within their derived bars).
  2. the padded CSR of long2d_p1_o3: a superset of dc.pattern, sorted, no duplicates, every node's dim columns adjacent in every
     row, both rows of the node at (11, 11) full, and the longest row above GG_MAX_ROW as csrc/kernels_general.hpp has it -- the
     case follows the constant and does not silently stop triggering.
  3. every seam case is on the scatter site it is listed for, by the launcher's own conditions (csrc/domain_dispatch.hpp,
     launch_general_dim) restated on the node and point counts; the seam boxes partition the points.
  4. MIMI_HIP_DOMAIN_INFO_GENERAL_ROUTE is code 13 of the parsed header, with the three routes, and the ABI number stays 12.

Measured (x86-64): long2d_p1_o3 min det F 0.777; oracle residual 3.0e-15 (neo-Hookean), 3.5e-15 (StVK), K v 9.4e-15, 1.7e-13
(StVK's tangent is the oracle's least accurate, 1/7 of MARGIN x 1e-11, as on the other cases); mix3d_322 j2simo plastic
0.67 / 0.34, oracle residual 3.4e-4 of the row bar, state 0.086 of its bar, K v 8.1e-12 (bar 4.4e-9)."""
import os
import re

import numpy as np
import pytest

import _domain_cases as dc
import _domain_reference as dr
from _domain_cases import MARGIN, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PAIRS = dc.LONG_PAIRS + [p for p in dc.SEAM_PAIRS if p not in dc.PAIRS]


def relmax(a, b):
    return float(np.abs(f64(a) - f64(b)).max() / max(np.abs(f64(b)).max(), 1e-300))


def gg_max_row():
    with open(os.path.join(ROOT, "mimi_amd", "csrc", "kernels_general.hpp")) as f:
        found = re.findall(r"constexpr int GG_MAX_ROW = (\d+);", f.read())
    assert len(found) == 1
    return int(found[0])


# ---- 1. the inputs, and the oracle on them ---------------------------------------------------------------------------------
def test_the_new_pairs_are_the_expected_ones():
    assert NEW_PAIRS == dc.LONG_PAIRS + [("mix3d_322", "j2simo")]
    assert dc.LONG_CASE not in dc.CASES and all(c != dc.LONG_CASE for c, _ in dc.PAIRS)          # (PAIRS did not grow)
    assert all(c in dc.CASES for c, _ in dc.SEAM_PAIRS + dc.SEAM_FD_PAIRS) and dc.SEAM_BOX_CASE in dc.CASES


@pytest.mark.parametrize("case,matname", NEW_PAIRS, ids=lambda v: v)
def test_inputs_satisfy_the_conditions(case, matname):
    ref = dc.reference(case, matname)
    bad, fig = dc.conditions(ref)
    print(f"{case} {matname}: {ref.geo.sp.n_points} points, " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert ref.geo.sp.n_points <= 3100
    assert not bad, bad
    assert fig["min_detF_u"] > 0


@pytest.mark.parametrize("case,matname", NEW_PAIRS, ids=lambda v: v)
def test_oracle_against_the_reference(case, matname):
    from test_domain_reference_cpu import oracle_run, oracle_state
    ref = dc.reference(case, matname)
    P, D, r0, r, Kv = oracle_run(case, matname)
    rowptr, col, conn = dc.pattern(case)
    assert np.array_equal(rowptr, D.rowptr) and np.array_equal(col, D.col) and np.array_equal(conn, D.conn)
    fig = {}
    if D.has_states:
        fig["state/bar"] = dc.compare_state(ref, oracle_state(D), dr.layout(ref.geo.sp), f"{case} {matname}")
    bar, want = dc.residual_bar(ref), f64(ref.asm.r)
    fig["residual"] = relmax(r, want)
    fig["residual/bar"] = max(float((np.abs(x - want) / bar).max()) for x in (r0, r))
    fig["Kv"] = max(relmax(a, b) for a, b in zip(Kv, ref.asm.Kv))
    print(f"{case} {matname}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["residual/bar"] <= MARGIN
    assert fig["Kv"] <= (dc.tangent_bar(matname) if dc.has_solver(matname) else MARGIN * dc.TANGENT_BAR)


def test_the_long_case_has_the_sizes_the_long_row_needs():
    a = dc.arrays(dc.LONG_CASE)
    sp_ = dc.geometry(dc.LONG_CASE).sp
    assert a.degrees == (1, 1) and a.n_ctrl == [23, 23] and a.n_vdofs == 1058 and a.order == 3 and a.weights is None
    assert (sp_.n_points, sp_.nq, sp_.n_spans) == (1936, 2, [22, 22])


# ---- 2. the padded pattern -----------------------------------------------------------------------------------------------------
def test_padded_pattern():
    a = dc.arrays(dc.LONG_CASE)
    rowptr0, col0, _ = dc.pattern(dc.LONG_CASE)
    rowptr, col, padded = dc.atomics_pattern(dc.LONG_CASE)
    dim, n = a.dim, a.n_vdofs
    assert len(rowptr) == n + 1 and rowptr[0] == 0 and rowptr[-1] == len(col) == len(padded)
    node = dc.LONG_NODE[0] + a.n_ctrl[0] * dc.LONG_NODE[1]
    assert all(0 < g < m - 1 for g, m in zip(dc.LONG_NODE, a.n_ctrl))                      # an interior node
    longest = 0
    for v in range(n):
        row, own = col[rowptr[v]:rowptr[v + 1]], col0[rowptr0[v]:rowptr0[v + 1]]
        assert np.all(np.diff(row) > 0) and row[0] >= 0 and row[-1] < n                     # sorted, no duplicates, in range
        assert np.isin(own, row).all()                                                     # a superset
        assert np.array_equal(padded[rowptr[v]:rowptr[v + 1]], ~np.isin(row, own))
        # every node's dim columns adjacent: the row is whole nodes, each as dim consecutive columns from a multiple of dim
        assert len(row) % dim == 0 and np.array_equal(row.reshape(-1, dim), row[::dim, None] + np.arange(dim))
        assert np.all(row[::dim] % dim == 0)
        # the dim rows of a node share their columns (what rowptr[rowA + i] + off of the scatter assumes)
        assert np.array_equal(row, col[rowptr[v - v % dim]:rowptr[v - v % dim + 1]])
        if v // dim == node:
            assert np.array_equal(row, np.arange(n))
        else:
            assert np.array_equal(row, own)
        longest = max(longest, len(row))
    assert longest == 1058 > gg_max_row()
    assert int(np.diff(rowptr0).max()) <= gg_max_row()                  # (without the padding the case would take the gather)
    assert padded.sum() == len(col) - len(col0) > 0
    # every other pattern of the module stays under the row image: only the seam takes those handles to the atomics
    for case in dc.SEAM_SITES:
        assert int(np.diff(dc.pattern(case)[0]).max()) <= gg_max_row()
        assert not dc.atomics_pattern(case)[2].any()


# ---- 3. the scatter sites ---------------------------------------------------------------------------------------------------------
def site(case):
    """the tangent kernel of launch_general_dim by the launcher's conditions (LDS of four elements aside: asserted on the
    GPU through the results alone)"""
    a = dc.arrays(case)
    sp_ = dc.geometry(case).sp
    n_dof, n_q = dc.pattern(case)[2].shape[1], sp_.nq ** sp_.dim
    if n_dof * ((n_dof + 2) // 3) <= 128 and n_q <= 64:
        return f"wave per element {a.dim}-D", n_dof
    if a.dim == 3 and n_dof == 64:
        return "matrix instruction", n_dof
    return ("512-thread vector pipe" if n_dof * n_dof > 3 * 256 else "256-thread node pairs"), n_dof


def test_seam_cases_reach_their_scatter_sites():
    want = {"rep2d_p3": ("wave per element 2-D", 16), "rep3d_p1": ("wave per element 3-D", 8), "mix3d_231": ("256-thread node pairs", 24),
            "mix3d_322": ("512-thread vector pipe", 36), "rep3d_p3": ("matrix instruction", 64),
            "flat2d_p4": ("256-thread node pairs", 25), "nurbs_flat_p2": ("256-thread node pairs", 27)}
    assert set(want) == set(dc.SEAM_SITES)
    for case, w in want.items():
        assert site(case) == w, case
    assert dc.arrays("flat2d_p4").flat and dc.arrays("nurbs_flat_p2").flat and dc.arrays("nurbs_flat_p2").weights is not None
    assert site(dc.LONG_CASE) == ("wave per element 2-D", 4)
    # every site has neo-Hookean and j2; the record material's pre-pass stands in front of the vector-pipe kernel
    for case in dc.SEAM_SITES:
        assert {(case, "neohook"), (case, "j2")} <= set(dc.SEAM_PAIRS)
    assert ("mix3d_322", "j2simo") in dc.SEAM_PAIRS and ("rep3d_p3", "stvk") in dc.SEAM_PAIRS
    assert {site(c)[0] for c, _ in dc.SEAM_FD_PAIRS} == {"wave per element 2-D", "256-thread node pairs", "matrix instruction"}


def test_seam_boxes_partition_the_points():
    sp_ = dc.geometry(dc.SEAM_BOX_CASE).sp
    assert sp_.n_spans == [3, 2, 4]
    total = np.zeros(sp_.n_points, dtype=int)
    for begin, end in dc.SEAM_BOXES:
        assert begin[:2] == [0, 0] and end[:2] == sp_.n_spans[:2]
        total += dr.in_box(sp_, begin, end)
    assert np.all(total == 1)


# ---- 4. the header -------------------------------------------------------------------------------------------------------------
def test_general_route_is_code_13_of_the_header():
    from mimi_amd import _capi, _header
    with open(os.path.join(ROOT, "include", "mimi_hip.h")) as f:
        h = _header.parse(f.read())
    assert h.enums["MIMI_HIP_DOMAIN_INFO_GENERAL_ROUTE"] == 13
    assert _capi.ABI.DOMAIN_INFO_GENERAL_ROUTE == 13
    codes = {k: v for k, v in h.enums.items() if k.startswith("MIMI_HIP_DOMAIN_INFO_")}
    assert sorted(codes.values()) == list(range(14))                    # no code twice, none skipped
    assert [h.enums[f"MIMI_HIP_GENERAL_ROUTE_{k}"] for k in ("NONE", "GATHER", "ATOMICS")] == [0, 1, 2]
    assert h.defines["MIMI_HIP_ABI_VERSION"] == 12                      # a new `what` adds no symbol: the number stays
    from mimi_amd.integrators import NonlinearSolid
    assert NonlinearSolid.GENERAL_ROUTES == {0: "none", 1: "gather", 2: "atomics"}
