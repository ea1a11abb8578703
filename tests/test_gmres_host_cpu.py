"""The least-squares side of the device GMRES (mimi_amd/csrc/gmres_host.hpp: Hessenberg column in, Givens rotations,
residual estimate out, back substitution) without a GPU.  tests/host_gmres_main.cpp, a stand-alone program, is built with the
host C++ compiler (-O1 -ffp-contract=off, AddressSanitizer and UndefinedBehaviorSanitizer where the box has their runtimes) and
run as a subprocess on the Hessenberg columns of the fp64 restatement oracle/krylov.py (its `trace`), on the Jacobi-scaled
systems of tests/_krylov_cases.py.

Residual estimates: BIT-EQUAL to the trace -- both sides run the same IEEE operations (*, +, -, /, sqrt, each rounded once) in
the same order on the same column.
Coefficients y: the header substitutes backwards, the restatement calls LAPACK, so they may differ by rounding.  The bar of a
case is BAR = 20 (tests/_krylov_cases.py) times the worst deviation max|y - y_mp| / max|y_mp| that the RESTATEMENT's solve shows
over the solves of that case from a 120-digit back substitution y_mp of the same rotated system (R, s); it is measured here
on the restatement, printed by `pytest -s`, and never on the header."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from mpmath import mp, mpf

import _krylov_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host_gmres_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = os.path.join(HERE, "_build", "host_gmres_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-o", out, SOURCE]
    # (the runtimes linked statically where the compiler can: the program then does not depend on the order libraries load in)
    for flags in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE):
        if subprocess.run(base + flags, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0:
            return out
    print("\nhost_gmres_main: no sanitizer runtimes on this box, built without them")
    subprocess.check_call(base)
    return out


def _replay(program, tmp_path, kdim, events):
    """the trace's cycles, columns and solves through the program: ([resid per column], [y per solve])"""
    lines = [f"kdim {kdim}"]
    for ev in events:
        if ev[0] == "cycle":
            lines.append(f"cycle {float(ev[1]).hex()}")
        elif ev[0] == "column":
            lines.append(f"column {ev[1]} " + " ".join(float(v).hex() for v in ev[2]))
        else:
            lines.append(f"solve {ev[1]}")
    path = tmp_path / "columns.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([program, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    resid, ys = [], []
    for line in run.stdout.splitlines():
        kind, *numbers = line.split()
        (resid if kind == "resid" else ys).append([float.fromhex(t) for t in numbers])
    return [r[0] for r in resid], [np.array(y) for y in ys]


def _back_substitution_mp(R, s):
    """y of R y = s for the fp64 numbers R (upper triangular), s at 120 digits"""
    k = len(s)
    with mp.workdps(120):
        y = [mpf(0)] * k
        for i in range(k - 1, -1, -1):
            t = mpf(float(s[i]))
            for j in range(i + 1, k):
                t -= mpf(float(R[i, j])) * y[j]
            y[i] = t / mpf(float(R[i, i]))
        return y


def _deviation(y, y_mp):
    with mp.workdps(120):
        scale = max(abs(v) for v in y_mp)
        return float(max(abs(mpf(float(a)) - b) for a, b in zip(y, y_mp)) / scale) if scale > 0 else float(np.abs(y).max())


# what each case is here for: (min cycles, the k of a solve that has to occur, or None)
CASES = {"ns36_k5": (20, 5), "ns36_k50": (1, None), "ns36_k7_cut3": (1, 3), "n1": (1, 1)}


@pytest.mark.parametrize("name", list(CASES))
def test_header_equals_the_restatement(name, program, tmp_path):
    from oracle import krylov
    A, b = kc.system(name)
    st = kc.settings(name)
    assert st["jacobi"]
    trace = []
    with np.errstate(invalid="ignore"):      # (n = 1: the unused v_1 of the restatement is 0 / 0)
        krylov.gmres(A, b.copy(), trace=trace, **st)
    cycles = [ev for ev in trace if ev[0] == "cycle"]
    columns = [ev for ev in trace if ev[0] == "column"]
    solves = [ev for ev in trace if ev[0] == "solve"]
    min_cycles, k_needed = CASES[name]
    assert len(cycles) >= min_cycles and len(solves) == len(cycles) and len(columns) == kc.reference(name)[0].iterations
    if name == "ns36_k50":
        assert len(cycles) == 1 and len(columns) > 7          # one long cycle
    if name == "ns36_k7_cut3":
        assert solves[-1][1] == 3 < st["kdim"]               # y at k < kdim
    if name == "n1":
        assert columns[0][2][-1] == 0.0                      # ||w||^2 = 0: the dy == 0 branch
    assert k_needed is None or any(ev[1] == k_needed for ev in solves)

    resid, ys = _replay(program, tmp_path, st["kdim"], trace)
    assert len(resid) == len(columns) and len(ys) == len(solves)
    differ = [(k, ev[1], float(ev[3]).hex(), float(r).hex()) for k, (ev, r) in enumerate(zip(columns, resid))
              if np.float64(ev[3]).tobytes() != np.float64(r).tobytes()]
    assert not differ, differ[:5]

    dev_oracle, dev_header = 0.0, 0.0
    for (_, k, R, s, y_oracle), y in zip(solves, ys):
        assert len(y) == k
        y_mp = _back_substitution_mp(R, s)
        dev_oracle = max(dev_oracle, _deviation(y_oracle, y_mp))
        dev_header = max(dev_header, _deviation(y, y_mp))
    print(f"\n{name}: {len(cycles)} cycles, {len(columns)} columns bit-equal; y deviates from the 120-digit solve: restatement "
          f"{dev_oracle:.3g} (bar {kc.BAR * dev_oracle:.3g}), header {dev_header:.3g}")
    assert dev_header <= kc.BAR * dev_oracle


def test_a_column_without_a_remainder(program, tmp_path):
    """||w||^2 = 0 by hand: dy == 0 takes c = 1, s = 0, so H(0, 0) = h_0 = 2 stays, the estimate is |-0 * beta| = 0 and
    y_0 = beta / h_0 = 3 / 2 -- every operation exact in fp64, so the expected values are the exact ones; then a second
    cycle on the same object with a remainder, against the rotation written out: dx = 3, dy = sqrt(16) = 4, |dy| > |dx|:
    t = 3 / 4, s = 1 / sqrt(1 + 9 / 16) = 0.8 (sqrt(1.5625) = 1.25 exactly), c = 0.6 to rounding"""
    events = [("cycle", 3.0), ("column", 0, [2.0, 0.0]), ("solve", 1),
              ("cycle", 5.0), ("column", 0, [3.0, 16.0]), ("solve", 1)]
    resid, ys = _replay(program, tmp_path, 2, events)
    assert resid[0] == 0.0 and ys[0].tolist() == [1.5]
    sn = 1.0 / np.sqrt(1.0 + 0.75 * 0.75)
    cs = 0.75 * sn
    assert sn == 0.8
    assert resid[1] == abs(-sn * 5.0) and ys[1].tolist() == [(cs * 5.0) / (cs * 3.0 + sn * 4.0)]
