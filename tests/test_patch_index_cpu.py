"""The index layer of the tensor kernels without a GPU: the node side of mimi_amd/csrc/patch_index.hpp (NodeWindow<P>: the
elements of a handle's box that contain a node, the node's local index in each, its clipped column window) compiled for
the host (tests/host_patch_index.hip) against a brute-force enumeration, the forward stages of mimi_amd/csrc/sum_factor.hpp
against a dense contraction, and every header of mimi_amd/csrc compiled alone."""
import ctypes
import glob
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mimi_amd", "csrc")


@pytest.fixture(scope="module")
def host_index():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = os.path.join(ROOT, "tests", "_build", "libhost_patch_index.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result",
                           "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "host_patch_index.hip")])
    return ctypes.CDLL(out)


def brute_force(P, box_begin, box_n, n_ctrl, node):
    """span e holds the nodes e .. e + P (no repeated interior knots).  Returns the elements of the box that contain the node
    as (index in the box, local index of the node, 3 x rank of the element's first node among the node's columns), in
    ascending element order, and the columns' first index and count per direction."""
    NB = P + 1
    cols = [[b for b in range(node[d] - P, node[d] + P + 1) if 0 <= b < n_ctrl[d]] for d in range(3)]
    ranked = {b: k for k, b in enumerate((b0, b1, b2) for b2 in cols[2] for b1 in cols[1] for b0 in cols[0])}
    found = []
    for ez, ey, ex in itertools.product(*(range(box_begin[d], box_begin[d] + box_n[d]) for d in (2, 1, 0))):
        e = (ex, ey, ez)
        if all(e[d] <= node[d] <= e[d] + P for d in range(3)):
            index = (ex - box_begin[0]) + box_n[0] * ((ey - box_begin[1]) + box_n[1] * (ez - box_begin[2]))
            local = (node[0] - ex) + NB * ((node[1] - ey) + NB * (node[2] - ez))
            found.append((index, local, 3 * ranked[e]))
    return found, [c[0] for c in cols], [len(c) for c in cols]


# elements of the patch, the handle's box (begin, count), node windows (begin, count; None: the nodes the box touches)
CASES = [((6, 4, 5), (1, 1, 1), (4, 2, 3), [None, "patch", ((2, 1, 3), (3, 2, 1))]),
         ((6, 4, 5), (0, 0, 0), (6, 4, 5), [None]),
         ((5, 3, 4), (2, 0, 1), (3, 1, 3), [None, "patch"])]


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_node_window_against_brute_force(host_index, P, case):
    """every node of every node window: a box strictly inside its patch (interior nodes with full support, nodes clipped by
    the box on either side, nodes clipped by the patch), the whole patch, a box of one element across; windows: the box's
    own nodes, a part of them (mimi_hip_domain_gather), and all nodes of the patch (nodes no element of the box contains)."""
    n_el, box_begin, box_n, windows = CASES[case]
    n_ctrl = [n + P for n in n_el]
    NS = (P + 1) ** 3
    arr = lambda v: (ctypes.c_int * 3)(*v)
    for win in windows:
        if win is None:
            win_begin, win_n = list(box_begin), [n + P for n in box_n]
        elif win == "patch":
            win_begin, win_n = [0, 0, 0], list(n_ctrl)
        else:
            win_begin, win_n = list(win[0]), list(win[1])
        n_nodes = int(np.prod(win_n))
        head = np.full((n_nodes, 18), -7, dtype=np.int64)
        slots = np.full((n_nodes, NS, 3), -7, dtype=np.int64)
        rc = host_index.host_node_windows(P, arr(box_begin), arr(box_n), arr(n_ctrl), arr(win_begin), arr(win_n),
                                          head.ctypes.data_as(ctypes.c_void_p), slots.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        seen_full = seen_clipped = seen_empty = False
        for Al in range(n_nodes):
            node = [win_begin[0] + Al % win_n[0], win_begin[1] + (Al // win_n[0]) % win_n[1], win_begin[2] + Al // (win_n[0] * win_n[1])]
            found, lo, w = brute_force(P, box_begin, box_n, n_ctrl, node)
            h = head[Al]
            assert list(h[:3]) == node
            assert h[3] == node[0] + n_ctrl[0] * (node[1] + n_ctrl[1] * node[2])
            assert bool(h[4]) == (not found)
            assert list(h[11:14]) == lo and list(h[14:17]) == w and h[17] == 3 * w[0] * w[1] * w[2]
            got = [tuple(int(x) for x in s) for s in slots[Al] if s[0] >= 0]
            assert got == found, (win, node)
            if found:
                # the clipped ranges are exactly the elements found, and the slots outside them are marked absent
                ranges = [(h[5], h[6]), (h[7], h[8]), (h[9], h[10])]
                assert len(found) == int(np.prod([hi - lo_ + 1 for lo_, hi in ranges]))
                for d in range(3):
                    assert ranges[d][0] == max(node[d] - P, box_begin[d]) and ranges[d][1] == min(node[d], box_begin[d] + box_n[d] - 1)
                assert all(0 <= a < NS for _, a, _ in found) and all(0 <= t < 3 * w[0] * w[1] * w[2] for _, _, t in found)
            seen_full |= len(found) == NS
            seen_clipped |= 0 < len(found) < NS
            seen_empty |= not found
        assert seen_clipped
        if win is None and all(box_n[d] >= P + 1 for d in range(3)):
            assert seen_full
        if win == "patch" and tuple(box_n) != tuple(n_el):
            assert seen_empty


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("dim", [2, 3])
def test_forward_stages_against_dense_contraction(host_index, dim, P):
    """load_element_tables, forward_stages, parametric_gradient and point_value as one thread runs them (NT = 1, tid = 0, an
    empty barrier), with two component sets, on seeded random table blocks of three spans per direction (the element is not
    the first one of its box, and the box does not begin the patch) and a random u_e: every point's H of both sets and the
    value of set 0 against numpy.einsum over the same tables.  The direction a 2-D patch lacks is B = 1, D = 0.
    Tolerance per entry 2 gamma_n S, n = 3 (P + 1) + 3, gamma_n = n eps / (1 - n eps), S the sum of the absolute products of
    that entry: the forward error bound of three nested dot products of P + 1 terms, once for each side."""
    rng = np.random.default_rng(1000 * dim + P)
    NB, NQ, n_spans = P + 1, P + 2, 3
    NBZ, NQZ = (NB, NQ) if dim == 3 else (1, 1)
    ND, NPT, NC = NB * NB * NBZ, NQ * NQ * NQZ, 2 * dim
    tables = rng.standard_normal((dim, 2, n_spans, NB, NQ))
    ve = rng.standard_normal((NC, ND))
    box_begin, el = [1, 0, 1][:dim], [1, 2, 0][:dim]
    tab = np.full((3, 2, NB, NQ), np.nan)
    H = np.full((2, NPT, dim, dim), np.nan)
    val = np.full((NPT, dim), np.nan)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = host_index.host_forward_stages(dim, P, n_spans, (ctypes.c_int * dim)(*box_begin), (ctypes.c_int * dim)(*el), ptr(tables), ptr(ve),
                                        ptr(tab), ptr(H), ptr(val))
    assert rc == 0
    # the element's block as loaded; the direction a 2-D patch lacks: B = 1 on its one node and point, D = 0
    for d in range(dim):
        assert np.array_equal(tab[d], tables[d, :, box_begin[d] + el[d]])
    if dim == 2:
        assert tab[2, 0].ravel()[0] == 1.0 and not tab[2, 0].ravel()[1:].any() and not tab[2, 1].any()
    B = [tab[d, 0] for d in range(dim)] + [np.ones((1, 1))] * (3 - dim)
    D = [tab[d, 1] for d in range(dim)] + [np.zeros((1, 1))] * (3 - dim)
    v = ve.reshape(NC, NBZ, NB, NB)                      # [component][a2][a1][a0]
    dense = lambda t, w: np.einsum("ax,by,cz,ncba->nzyx", t[0], t[1], t[2], w).reshape(len(w), NPT)   # point = q0 + NQ (q1 + NQ q2)
    n = 3 * (P + 1) + 3
    eps = np.finfo(np.float64).eps / 2
    gamma = n * eps / (1 - n * eps)
    for m in range(dim + 1):                             # m < dim: the derivative along direction m; m == dim: the value
        t = [D[d] if m < dim and d == m else B[d] for d in range(3)]
        w = v[:dim] if m == dim else v                   # (the value is taken of component set 0)
        got = val.T if m == dim else H[..., m].transpose(0, 2, 1).reshape(NC, NPT)
        assert np.isfinite(got).all()
        err = np.abs(got - dense(t, w))
        bound = 2 * gamma * dense([np.abs(x) for x in t], np.abs(w))
        print(f"dim {dim} P {P} {'value' if m == dim else 'd/dxi_%d' % m}: largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()


def test_every_header_compiles_alone():
    """each header of mimi_amd/csrc includes what it uses: host side only, syntax only"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    headers = sorted(glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(headers) >= 20
    failed = {}
    for h in headers:
        run = subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-fsyntax-only", "-std=c++17",
                              "-Wno-unused-result", "-Wno-pragma-once-outside-header", h], cwd=CSRC, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)
        if run.returncode != 0:
            failed[os.path.basename(h)] = run.stdout[-2000:]
    assert not failed, failed


def test_dispatch_headers_include_kernel_headers_never_the_reverse():
    dispatch = {"domain_dispatch.hpp", "domain_dispatch_nodal.hpp", "tensor_dispatch.hpp", "domain_create.hpp"}
    for h in glob.glob(os.path.join(CSRC, "kernels_*.hpp")) + [os.path.join(CSRC, "patch_index.hpp"), os.path.join(CSRC, "sum_factor.hpp")]:
        text = open(h).read()
        for d in dispatch:
            assert f'#include "{d}"' not in text, (os.path.basename(h), d)
    # no function is declared ahead of the header that defines it
    for line in open(os.path.join(CSRC, "tensor_dispatch.hpp")):
        assert not (line.startswith("inline") and line.split("//")[0].rstrip().endswith(";")), line
