"""One frozen and one consistent action of the contact tangent (csrc/kernels_face_action.hpp, csrc/kernels_face_consistent.hpp,
DESIGN.md 4.8) on the top face of BASELINE configuration 4: 96 x 96 x 12 degree-2 elements of side 1 / 64, 9 216 contact faces
of 9 nodes and 16 points, on the SAME handle.  Two bodies: the rigid sphere of bench.py's cfg4 (radius a quarter of the block's
length, pressed 10 % of its radius into the face: few faces active) and a plane pressed into the whole face (every face
active).  Per body and mode: milliseconds per ApplyTangent and per Linearize between device events (warmed, alternating the
two modes over ROUNDS rounds: median and spread), the bytes of the record, and the largest difference of the two actions.
With --registers the register table of the kernels (compiled here, no device needed) goes first.

    python scratch/consistent_action_rate.py [--registers]      into profiles/consistent_action_rate.txt"""
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELL = 1.0 / 64
N_EL = (96, 96, 12)
PENALTY = 1.0e2
ROUNDS, REPS = 7, 200


def register_table():
    """vector / scalar registers, scratch bytes and spills of the action kernels of contact.hip, from the build's own assembly"""
    from mimi_amd import isa_lint as L
    asm = L.assembly("contact.hip")
    spills = L.spill_counts(asm)
    lines = ["kernel                                                   vgpr  sgpr  scratch  spills"]
    for name in sorted(spills):
        if "consistent" not in name and "boundary_" not in name:
            continue
        i = asm.find(".amdhsa_kernel " + name)
        block = asm[i:asm.find(".end_amdhsa_kernel", i)]
        get = lambda key: re.search(key + r"\s+(\S+)", block).group(1)
        short = re.search(r"\d+((?:contact_consistent|boundary)_[a-z_]+)(ILi\d)?", name)
        label = short.group(1) + ("<%s>" % short.group(2)[-1] if short.group(2) else "")
        lines.append(f"{label:56s} {get(r'.amdhsa_next_free_vgpr'):>4s}  {get(r'.amdhsa_next_free_sgpr'):>4s}  "
                     f"{get(r'.amdhsa_private_segment_fixed_size'):>7s}  {spills[name]:>6d}")
    return lines


def measure():
    import numpy as np
    import torch
    import mimi_amd as mimi
    from mimi_amd.integrators import CSRPattern, MortarContact, RigidPlane, RigidSphere
    dev = torch.device("cuda", 0)
    L = [m * CELL for m in N_EL]
    block = mimi.BSplinePatch.block(N_EL, 2, lengths=L)
    pattern = CSRPattern.of_bspline_patch(block, on_device=True)
    R = 0.25 * L[0]
    bodies = (("sphere (bench.py cfg4)", RigidSphere([0.5 * L[0], 0.5 * L[1], L[2] + 0.9 * R], R, PENALTY)),
              ("plane over the whole face", RigidPlane([0.0, 0.0, L[2] - 0.1 * CELL], [0.0, 0.0, -1.0], PENALTY)))
    u = torch.zeros(block.n_vdofs, dtype=torch.float64, device=dev)
    x = torch.randn(block.n_vdofs, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y = torch.zeros_like(x)

    def per_call_ms(f):
        for _ in range(20):
            f()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / REPS

    lines = []
    for label, body in bodies:
        c = MortarContact(body, "contact", pattern, block, 2, 1).Prepare()
        times = {m: dict(action=[], linearize=[]) for m in (False, True)}
        bytes_, out = {}, {}
        for _ in range(ROUNDS):
            for mode in (False, True):
                c.SetConsistentTangent(mode)
                c.Linearize(u)
                bytes_[mode] = c.LinearizationBytes()
                y.zero_()
                c.ApplyTangent(x, y, 1.0)
                out[mode] = y.clone()
                times[mode]["action"].append(per_call_ms(lambda: c.ApplyTangent(x, y, 1.0)))
                times[mode]["linearize"].append(per_call_ms(lambda: c.Linearize(u)))
        active = int((c.AveragePressure() != 0).sum())
        lines.append(f"-- {label}: {c.n_marked_boundaries_} faces, {len(c.MarkedNodes())} marked nodes, {active} with pressure --")
        for mode in (False, True):
            t = times[mode]
            lines.append(f"{'consistent' if mode else 'frozen    '}  action {statistics.median(t['action']):.4f} ms "
                         f"({min(t['action']):.4f} .. {max(t['action']):.4f})   linearize {statistics.median(t['linearize']):.4f} ms "
                         f"({min(t['linearize']):.4f} .. {max(t['linearize']):.4f})   record {bytes_[mode]} bytes")
        lines.append(f"consistent / frozen action: {statistics.median(times[True]['action']) / statistics.median(times[False]['action']):.2f}; "
                     f"max |consistent - frozen| {float((out[True] - out[False]).abs().max()):.3e} of max |frozen| "
                     f"{float(out[False].abs().max()):.3e}")
    return lines


if __name__ == "__main__":
    lines = ["scratch/consistent_action_rate.py on one MI355X: ApplyTangent and Linearize of one contact handle, frozen and consistent,",
             f"between device events, {REPS} calls per window, {ROUNDS} alternating rounds (median, lowest .. highest)."]
    if "--registers" in sys.argv:
        lines += register_table()
    lines += measure()
    print("\n".join(lines))
    path = os.path.join(ROOT, "profiles", "consistent_action_rate.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
