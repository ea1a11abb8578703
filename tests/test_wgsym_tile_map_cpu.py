"""The map (chain, pair) -> (S3 tile, tile row) of the packed tiles of the symmetric-half degree-2 kernel, read from the one
definition the kernel compiles (mimi_amd/csrc/p2_tile_map.hpp) through a host program that prints it (tests/p2_tile_map_main.cpp).

A tile has 16 rows; result row r is accumulator register r // 4 of the lanes with lane >> 4 == r % 4.  Pair index = 3 a2 + b2;
the z-carry adds the pairs with a2, b2 >= 1 (4, 5, 7, 8) of an element to pair - 4 of the next one, and the kernel does that
without crossing lanes.  So:
  - the map is a bijection onto the rows it uses, and the hosts' rows are those of an unpacked tile (their code is unchanged);
  - every carried pair sits exactly four rows above pair - 4 of the same chain in the same tile (the next register of the same
    lane) -- or is one of the listed exceptions, the rider's pairs 7 and 8, which sit in the SAME row of the other tile as the
    rider's pairs 3 and 4 (the same register of the same lane);
  - the rider's operand rows are reachable by one row shift each, and the shift of its high pairs only writes rows 12..15 (the
    one lane quad the move is allowed to touch), whose rows 14, 15 are fed from operand rows 9, 10: always zero;
  - a b1 is packed only where a block contracts all three of its chains: at level 2 everywhere it does, at level 1 (shipped)
    for b1 = 0, 1 of the off-diagonal block, at level 0 nowhere; never in the nine-block kernel."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CARRIED = (4, 5, 7, 8)
# (a1, pair): carried into the same row of the other tile instead of four rows down in its own
EXCEPTIONS = {(1, 7), (1, 8)}


@pytest.fixture(scope="module")
def table():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") \
        or "/opt/rocm/bin/hipcc"
    out = os.path.join(HERE, "_build", "p2_tile_map_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", out, os.path.join(HERE, "p2_tile_map_main.cpp")])
    run = subprocess.run([out], stdout=subprocess.PIPE, text=True, check=True)
    slots, consts, packed = {}, {}, {}
    for line in run.stdout.splitlines():
        kind, *v = line.split()
        if kind == "slot":
            slots[(int(v[0]), int(v[1]))] = (int(v[2]), int(v[3]))
        elif kind == "packed":
            packed[(int(v[0]), int(v[1]), int(v[2]))] = bool(int(v[3]))
        else:
            consts[kind] = int(v[0])
    return slots, consts, packed


def test_bijection_onto_the_used_rows(table):
    slots, consts, _ = table
    assert sorted(slots) == [(a1, p) for a1 in range(3) for p in range(9)]
    assert len(set(slots.values())) == 27
    assert all(0 <= t < consts["tiles"] and 0 <= r < 16 for t, r in slots.values())
    assert consts["tiles"] == 2                       # 27 rows do not fit one tile
    # the hosts: rows 0..8 of a tile each, pair = row, as in a tile of their own
    hosts = [a1 for a1 in range(3) if a1 != consts["rider"]]
    assert sorted(slots[(a1, 0)][0] for a1 in hosts) == [0, 1]
    for a1 in hosts:
        assert all(slots[(a1, p)] == (slots[(a1, 0)][0], p) for p in range(9))


def test_carried_pairs_stay_in_their_lane(table):
    slots, consts, _ = table
    seen = set()
    for a1 in range(3):
        for p in CARRIED:
            tile, row = slots[(a1, p)]
            t_to, r_to = slots[(a1, p - 4)]
            if (tile, row) == (t_to, r_to + 4):
                continue
            # the exception: same row (same register, same lane) of the other tile
            assert (a1, p) in EXCEPTIONS, (a1, p)
            assert a1 == consts["rider"] and row == r_to and tile != t_to
            seen.add((a1, p))
    assert seen == EXCEPTIONS


def test_the_rider_rows_are_one_row_shift_each(table):
    slots, consts, _ = table
    rider, split, low, high = consts["rider"], consts["split"], consts["shift_low"], consts["shift_high"]
    for p in range(9):
        tile, row = slots[(rider, p)]
        assert row - p == (low if p < split else high)
        assert tile == (0 if p < split else 1)
        assert row >= 9                               # above the host's rows
    # the low shift leaves rows < 9 alone by itself (rows below the shift keep the host's values)
    assert low == 9
    # the high shift is restricted to rows 12..15: they take operand rows 12 - high .. 15 - high = the pairs 7, 8 and rows 9, 10
    assert [r - high for r in range(12, 16)] == [7, 8, 9, 10]


def test_which_b1_are_packed(table):
    _, _, packed = table
    for b1 in range(3):
        three_chains = {0: False, 1: True, 2: b1 == 0}   # mode 0: nine-block kernel; 1: off-diagonal; 2: diagonal, chains a1 >= b1
        for mode in range(3):
            assert not packed[(0, mode, b1)]
            assert packed[(2, mode, b1)] == three_chains[mode]
            assert packed[(1, mode, b1)] == (mode == 1 and b1 < 2)
            assert not packed[(1, mode, b1)] or packed[(2, mode, b1)]
    # matrix instructions per element: 3 waves x (diagonal 8 + 4 tiles + off-diagonal 9 + 4 tiles)
    per_element = lambda level: 3 * sum((8 if mode == 2 else 9) + 4 * sum(
        (3 if mode == 1 else 3 - b1) - (1 if packed[(level, mode, b1)] else 0) for b1 in range(3)) for mode in (2, 1))
    assert [per_element(level) for level in range(3)] == [231, 207, 183]
