"""The augmented-Lagrangian contact mode beside the penalty law (csrc/kernels_face_augmented.hpp), on the top
face of BASELINE configuration 4: 96 x 96 x 12 degree-2 elements of side 1 / 64, 9 216 contact faces of 9 nodes and 16 points.
Two handles on the same tables, one in each mode, against a plane pressed into the whole face (every face active); the
multipliers of the augmented one are -PENALTY x 0.05 cells x a random number per node.  Per mode, alternating in the same
call: milliseconds per AddBoundaryResidualAndGrad (pass 1, pressure, pass 2, tangent blocks, row gather), per
AddBoundaryResidual, per consistent ApplyTangent and Linearize, and per UpdateLagrange (pass 1, update, measure, the copy of
four numbers and a synchronisation), between device events, warmed, ROUNDS rounds: median and spread.

    python scratch/augmented_contact_rate.py      into profiles/augmented_contact_rate.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELL = 1.0 / 64
N_EL = (96, 96, 12)
PENALTY = 1.0e2
ROUNDS, REPS = 5, 200


def measure():
    import numpy as np
    import torch
    import mimi_amd as mimi
    from mimi_amd.integrators import CSRPattern, MortarContact, RigidPlane
    dev = torch.device("cuda", 0)
    L = [m * CELL for m in N_EL]
    block = mimi.BSplinePatch.block(N_EL, 2, lengths=L)
    pattern = CSRPattern.of_bspline_patch(block, on_device=True)
    handles = {}
    for mode in ("penalty", "augmented"):
        c = MortarContact(RigidPlane([0.0, 0.0, L[2] - 0.1 * CELL], [0.0, 0.0, -1.0], PENALTY), "contact", pattern, block, 2, 1).Prepare()
        c.SetConsistentTangent(True)
        if mode == "augmented":
            c.SetAugmented(True)
            c.SetLagrange(-PENALTY * 0.05 * CELL * np.random.default_rng(7).random(len(c.MarkedNodes())))
        handles[mode] = c
    u = torch.zeros(block.n_vdofs, dtype=torch.float64, device=dev)
    x = torch.randn(block.n_vdofs, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y, r = torch.zeros_like(x), torch.zeros_like(x)
    A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)

    def per_call_ms(f, reps=REPS):
        for _ in range(min(20, reps)):
            f()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def wall_ms(f, reps=REPS):
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / reps

    calls = {"residual and tangent": lambda c: per_call_ms(lambda: c.AddBoundaryResidualAndGrad(u, 1.0, r, A)),
             "residual": lambda c: per_call_ms(lambda: c.AddBoundaryResidual(u, r)),
             "consistent action": lambda c: per_call_ms(lambda: c.ApplyTangent(x, y, 1.0)),
             "linearize": lambda c: per_call_ms(lambda: c.Linearize(u))}
    times = {(m, k): [] for m in handles for k in calls}
    update = []
    for _ in range(ROUNDS):
        for k, f in calls.items():
            for m, c in handles.items():
                c.Linearize(u)
                times[(m, k)].append(f(c))
        update.append(wall_ms(lambda: handles["augmented"].UpdateLagrange(u, apply=False)))
    c = handles["augmented"]
    active = {m: int((h.AveragePressure() != 0).sum()) for m, h in handles.items()}
    lines = [f"-- plane over the whole face: {c.n_marked_boundaries_} faces, {len(c.MarkedNodes())} marked nodes; with pressure: "
             f"penalty {active['penalty']}, augmented {active['augmented']}; record bytes: penalty "
             f"{handles['penalty'].LinearizationBytes()}, augmented {c.LinearizationBytes()} --"]
    for k in calls:
        row = []
        for m in handles:
            t = times[(m, k)]
            row.append(f"{m} {statistics.median(t):.4f} ms ({min(t):.4f} .. {max(t):.4f})")
        ratio = statistics.median(times[("augmented", k)]) / statistics.median(times[("penalty", k)])
        lines.append(f"{k:22s} " + "   ".join(row) + f"   augmented / penalty {ratio:.3f}")
    lines.append(f"UpdateLagrange(apply=False), wall clock per call with its synchronisation: {statistics.median(update):.4f} ms "
                 f"({min(update):.4f} .. {max(update):.4f})")
    return lines


if __name__ == "__main__":
    lines = ["scratch/augmented_contact_rate.py on one MI355X: one contact handle per mode on the same face tables, between device events,",
             f"{REPS} calls per window, {ROUNDS} rounds alternating between the modes (median, lowest .. highest)."]
    lines += measure()
    print("\n".join(lines))
    with open(os.path.join(ROOT, "profiles", "augmented_contact_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
