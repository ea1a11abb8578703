"""The launch geometry of the symmetric-half degree-2 kernel -- segments per column, elements per segment, units a workgroup
walks, workgroups -- read from the one definition the launcher compiles (mimi_amd/csrc/wgsym_geometry.hpp) through a host program
that prints it (tests/wgsym_geometry_main.cpp), for every element box with n0, n1 <= 12 and nz <= 40 and the benchmark shapes,
at the shipped WGSYM_MIN_WGS and at the values tests put in its place through MIMI_HIP_WGSYM_MIN_WGS.

  - the segments tile a column: nseg * seg_len == nz; a cut column has segments of at least four elements and the cut launch
    at most WGSYM_SPLIT_BELOW workgroups;
  - a workgroup walks 1..WGSYM_MAX_COLS units, and the grid covers the units exactly: the last workgroup has at least one and
    at most cols_per_wg of them (the kernel clips it: tensor_wgsym_kernel, n_cols);
  - at the shipped constant the walk grows at 4096, 6144 and 8192 units, and never on a launch whose columns are cut.
The switch itself: a value that is not a positive integer fails the create, before a device is asked for."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OVERRIDES = (0, 1, 2, 3, 5)          # 0: the shipped constant
BENCH_SHAPES = [(64, 64, 8), (96, 96, 12), (128, 128, 16), (256, 256, 32)]
# (box, units, cols_per_wg): either side of every threshold of the shipped constant, and the shapes of tests/test_wgsym_walk_gpu.py
THRESHOLDS = [((63, 65, 1), 4095, 1), ((64, 64, 1), 4096, 2), ((6143, 1, 1), 6143, 2), ((96, 64, 1), 6144, 3),
              ((8191, 1, 1), 8191, 3), ((128, 64, 1), 8192, 4), ((128, 128, 1), 16384, 4),
              ((65, 65, 1), 4225, 2), ((79, 79, 1), 6241, 3), ((91, 93, 1), 8463, 4), ((64, 64, 5), 4096, 2)]


@pytest.fixture(scope="module")
def geometry():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") \
        or "/opt/rocm/bin/hipcc"
    out = os.path.join(HERE, "_build", "wgsym_geometry_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", out, os.path.join(HERE, "wgsym_geometry_main.cpp")])
    import bench
    boxes = [(a, b, c) for a in range(1, 13) for b in range(1, 13) for c in range(1, 41)] + BENCH_SHAPES
    boxes += sorted({tuple(n_el) for n_el, p, _ in bench.WORKLOADS.values() if p == 2} - set(boxes))
    asked = [(*box, k) for box in boxes for k in OVERRIDES] + [(*box, 0) for box, _, _ in THRESHOLDS]
    run = subprocess.run([out], input="".join("%d %d %d %d\n" % q for q in asked), stdout=subprocess.PIPE, text=True, check=True)
    lines = run.stdout.splitlines()
    split_below, max_cols, min_wgs = (int(v) for v in lines[0].split()[1:])
    table = {}
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        table[tuple(v[:4])] = tuple(v[4:])
    assert sorted(table) == sorted(set(asked))
    return dict(split_below=split_below, max_cols=max_cols, min_wgs=min_wgs), table


def test_shipped_constants(geometry):
    consts, _ = geometry
    assert consts == dict(split_below=512, max_cols=4, min_wgs=2048)


def test_segments_tile_the_column_and_the_grid_covers_the_units(geometry):
    consts, table = geometry
    cut = walks = ragged = 0
    for (n0, n1, nz, k), (nseg, seg_len, cols_per_wg, grid) in table.items():
        key = (n0, n1, nz, k)
        assert nseg >= 1 and nseg * seg_len == nz, key
        if nseg > 1:
            assert seg_len >= 4 and n0 * n1 * nseg <= consts["split_below"], key
            cut += 1
        assert 1 <= cols_per_wg <= consts["max_cols"] == 4, key
        n_units = n0 * n1 * nseg
        assert grid * cols_per_wg >= n_units > (grid - 1) * cols_per_wg, key
        walks += cols_per_wg > 1
        ragged += cols_per_wg > 1 and n_units % cols_per_wg != 0
        # the value in place of WGSYM_MIN_WGS is the number of workgroups the walk keeps, wherever it grows and is not clamped
        min_wgs = k or consts["min_wgs"]
        if 1 < cols_per_wg < consts["max_cols"]:
            assert n_units // cols_per_wg >= min_wgs, key
        if k == 0 and nseg > 1:
            assert cols_per_wg == 1, key              # (a cut launch has at most 512 units)
    assert cut > 1000 and walks > 1000 and ragged > 1000          # (the table does hold such launches)


def test_the_cut_is_the_deepest_halving_allowed(geometry):
    """nseg is a power of two, and one more halving would break a condition"""
    consts, table = geometry
    for (n0, n1, nz, k), (nseg, seg_len, _, _) in table.items():
        assert nseg & (nseg - 1) == 0
        assert n0 * n1 * nseg * 2 > consts["split_below"] or nz % (nseg * 2) != 0 or nz // (nseg * 2) < 4, (n0, n1, nz, k)
    for box, want in (((2, 2, 16), (4, 4)), ((3, 3, 10), (2, 5)), ((3, 3, 12), (2, 6)), ((3, 3, 8), (2, 4)), ((5, 4, 8), (2, 4)),
                      ((2, 2, 8), (2, 4)), ((3, 3, 5), (1, 5)), ((5, 4, 9), (1, 9)), ((1, 1, 32), (8, 4)), ((12, 12, 8), (2, 4)),
                      ((12, 12, 16), (2, 8)), ((8, 8, 8), (2, 4)), ((8, 8, 32), (8, 4)), ((64, 64, 8), (1, 8))):
        assert table[(*box, 0)][:2] == want, box


def test_thresholds_of_the_shipped_constant(geometry):
    _, table = geometry
    for box, units, cols in THRESHOLDS:
        nseg, seg_len, cols_per_wg, grid = table[(*box, 0)]
        assert nseg == 1 and seg_len == box[2] and box[0] * box[1] == units
        assert cols_per_wg == cols, (box, units)
        assert grid == -(-units // cols)
    # the benchmark shapes: four columns per workgroup, no ragged tail
    for box in BENCH_SHAPES:
        nseg, seg_len, cols_per_wg, grid = table[(*box, 0)]
        units = box[0] * box[1]
        assert (nseg, seg_len) == (1, box[2])
        assert cols_per_wg == min(4, units // 2048) and units % cols_per_wg == 0 and grid == units // cols_per_wg


def test_the_walks_of_the_gpu_tests(geometry):
    """what tests/test_wgsym_walk_gpu.py asks for through the switch (override -> cols_per_wg, units of the last workgroup); the
    overrides 4, 21, 14, 10, 6 are not in OVERRIDES, so these come from the same arithmetic restated here"""
    _, table = geometry

    def walk(box, k):
        nseg = table[(*box, 0)][0]
        units = box[0] * box[1] * nseg
        cols = max(1, min(4, units // k))
        return cols, units - (-(-units // cols) - 1) * cols

    assert [walk((3, 3, 5), k) for k in (4, 3, 2)] == [(2, 1), (3, 3), (4, 1)]
    assert [walk((7, 6, 1), k) for k in (21, 14, 10)] == [(2, 2), (3, 3), (4, 2)]
    assert [walk((5, 4, 2), k) for k in (5, 6)] == [(4, 4), (3, 2)]
    assert [walk((2, 2, 8), k) for k in (2, 4)] == [(4, 4), (2, 2)]
    for box, k in (((3, 3, 5), 3), ((3, 3, 5), 2), ((2, 2, 8), 2)):
        assert table[(*box, k)][2] == walk(box, k)[0]


@pytest.mark.parametrize("value", ["0", "-3", "abc", "", "2x", "1.5", "99999999999"])
def test_a_value_that_is_no_positive_integer_fails_the_create(monkeypatch, value):
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    patch = mimi_amd.BSplinePatch.block((2, 2, 2), 2)
    pat = CSRPattern(np.zeros(patch.n_vdofs + 1, dtype=np.int64), np.zeros(1, dtype=np.int32), 0)
    mat = mimi_amd.CompressibleOgdenNeoHookean()
    mat.set_young_poisson(2100, 0.3)
    monkeypatch.setenv("MIMI_HIP_WGSYM_MIN_WGS", value)
    with pytest.raises(RuntimeError, match="MIMI_HIP_WGSYM_MIN_WGS must be a positive integer"):
        NonlinearSolid("domain", mat, pat, patch=patch).Prepare()
