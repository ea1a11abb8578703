"""The normal helpers of the wave-per-face layer (mimi_amd/csrc/face_wave.hpp) without a GPU: tests/host_face_wave_main.hip, a
stand-alone program, is built for the host with -O1 -ffp-contract=off (AddressSanitizer and UndefinedBehaviorSanitizer where
the box has their runtimes) and run as a subprocess on seeded tangents t, derivatives dN and every (b, j), DIM 2 and 3.

face_normal_column(b, j) against face_normal_rate with dt_k = dN[k n_dof + b] e_j: the two texts of dm/dx_bj -- the assembled
tangent blocks use the first, the matrix-free actions the second.  With -ffp-contract=off every product by 0 or 1 is exact, so
the two are an identity: BIT FOR BIT after x + 0.0, which canonicalises the sign of a zero and changes nothing else.  The one thing the
identity leaves open is the sign of a zero: the components that vanish identically come out as +0 on one side and -0 on the
other (2-D: -dt[0] with dt[0] = +0 is -0, where the column form writes the literal 0.0; 3-D: the differences of two signed
zeros), which no later sum or product can tell apart from +0 in a result that is not itself zero.  The test counts them and
requires that they occur ONLY where both values are zero.

Both against numpy (cross products), to a rounding bound: so that the pair cannot agree on a wrong formula."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host_face_wave_main.hip")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
N_DOF = 16
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def program():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = os.path.join(HERE, "_build", "host_face_wave_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    base = ["hipcc", "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off",
            "-Wno-unused-result", "-o", out, SOURCE]
    if subprocess.run(base + SANITIZE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0:
        return out
    print("\nhost_face_wave_main: no sanitizer runtimes on this box, built without them")
    subprocess.check_call(base)
    return out


def _value(hex16):
    return struct.unpack("<d", struct.pack("<Q", int(hex16, 16)))[0]


def _run(program, seed):
    run = subprocess.run([program, str(seed), str(N_DOF)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = {2: {"t": {}, "dN": {}, "len": None, "col": {}}, 3: {"t": {}, "dN": {}, "len": None, "col": {}}}
    for line in run.stdout.splitlines():
        kind, dim, *rest = line.split()
        d = out[int(dim)]
        if kind in ("t", "dN"):
            d[kind][int(rest[0])] = _value(rest[1])
        elif kind == "len":
            d["len"] = [_value(h) for h in rest]
        else:
            d["col"][tuple(int(v) for v in rest[:3])] = (rest[3], rest[4])
    return out


def _tangents3(d, dim):
    """t as (dim - 1) rows of 3 components (2-D: the plane z = 0 and a_2 = e_z, whose cross products are the 2-D formulas)"""
    t = np.array([d["t"][k] for k in range((dim - 1) * dim)]).reshape(dim - 1, dim)
    if dim == 3:
        return t[0], t[1]
    return np.array([t[0, 0], t[0, 1], 0.0]), np.array([0.0, 0.0, 1.0])


@pytest.mark.parametrize("seed", [1, 20260412])
def test_column_equals_rate(program, seed):
    out = _run(program, seed)
    for dim in (2, 3):
        d = out[dim]
        assert len(d["col"]) == N_DOF * dim * dim
        t1, t2 = _tangents3(d, dim)
        dN = np.array([d["dN"][k] for k in range((dim - 1) * N_DOF)]).reshape(dim - 1, N_DOF)
        bit_equal = zero_sign = 0
        for (b, j, i), (hc, hr) in sorted(d["col"].items()):
            c, r = _value(hc), _value(hr)
            # bit for bit once a zero's sign is canonicalised (x + 0.0 turns -0 into +0 and changes nothing else)
            assert struct.pack("<d", c + 0.0) == struct.pack("<d", r + 0.0), (dim, b, j, i, hc, hr)
            if hc == hr:
                bit_equal += 1
            else:
                assert c == 0.0 and r == 0.0, (dim, b, j, i, hc, hr)   # raw bits differ only in the sign of a zero
                zero_sign += 1
            # the formula itself: dm = dN_1 (e_j x a_2) + dN_2 (a_1 x e_j)
            e = np.zeros(3)
            e[j] = 1.0
            want = dN[0, b] * np.cross(e, t2) + (dN[1, b] * np.cross(t1, e) if dim == 3 else 0.0)
            scale = abs(dN[0, b]) * np.abs(t2).max() + (abs(dN[1, b]) * np.abs(t1).max() if dim == 3 else 0.0)
            assert abs(c - want[i]) <= 4 * EPS * scale, (dim, b, j, i, c, want[i])
        print(f"\nseed {seed} DIM {dim}: {bit_equal} of {len(d['col'])} entries bit-equal, {zero_sign} zeros of opposite sign, 0 unequal")
        # the identically vanishing entries: dm_i / dx_bi (2-D and 3-D: the diagonal of a skew matrix)
        assert zero_sign <= N_DOF * dim


@pytest.mark.parametrize("seed", [1, 20260412])
def test_normal_and_length(program, seed):
    out = _run(program, seed)
    for dim in (2, 3):
        d = out[dim]
        t1, t2 = _tangents3(d, dim)
        want = np.cross(t1, t2)[:dim]
        length, m = d["len"][0], np.array(d["len"][1:])
        bound = 4 * EPS * np.abs(t1).max() * np.abs(t2).max()
        assert np.abs(m - want).max() <= bound
        assert abs(length - np.linalg.norm(want)) <= 4 * EPS * np.linalg.norm(want) + 2 * bound
