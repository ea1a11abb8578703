"""One action of the contact tangent with Coulomb friction (csrc/kernels_face_friction_action.hpp), frozen and
consistent, beside the frictionless actions and one assembled friction tangent, on the top face of BASELINE configuration 4:
96 x 96 x 12 degree-2 elements of side 1 / 64, 9 216 contact faces of 9 nodes and 16 points, on the SAME handle.  Two bodies,
those of scratch/consistent_action_rate.py: the rigid sphere of bench.py's cfg4 (few faces active) and a plane pressed into the
whole face (every face active).  The friction state is committed at u = 0; the actions are linearised at a shear of the face
along x that grows with x, so that a part of the points sticks and a part slips.  Per body, friction (mu = 0 / 0.3, the
action on in both) and mode: milliseconds per ApplyTangent and per Linearize between device events (warmed, alternating over
ROUNDS rounds: median and spread) and the bytes of the record; per body the milliseconds of one AddBoundaryResidualAndGrad
with and without friction.  With --registers the register table of the kernels (compiled here, no device needed) goes first.

    python scratch/friction_action_rate.py [--registers]      into profiles/friction_action_rate.txt"""
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELL = 1.0 / 64
N_EL = (96, 96, 12)
PENALTY = 1.0e2
MU = 0.3
SHEAR = 1.0e-3               # the face's displacement along x at its far end
ROUNDS, REPS = 5, 200


def register_table():
    """vector / scalar registers, scratch and LDS bytes and spills of the friction action's kernels, from the build's own assembly"""
    from mimi_amd import isa_lint as L
    asm = L.assembly("contact.hip")
    spills = L.spill_counts(asm)
    lines = ["kernel                                                   vgpr  sgpr  scratch  lds  spills"]
    for name in sorted(spills):
        short = re.search(r"\d+(contact_friction_(?:action|record)_kernel)ILi(\d)(?:ELb(\d))?", name)
        if not short:
            continue
        i = asm.find(".amdhsa_kernel " + name)
        block = asm[i:asm.find(".end_amdhsa_kernel", i)]
        get = lambda key: re.search(key + r"\s+(\S+)", block).group(1)
        label = f"{short.group(1)}<{short.group(2)}" + ("" if short.group(3) is None else ", consistent" if short.group(3) == "1" else ", frozen") + ">"
        lines.append(f"{label:56s} {get(r'.amdhsa_next_free_vgpr'):>4s}  {get(r'.amdhsa_next_free_sgpr'):>4s}  "
                     f"{get(r'.amdhsa_private_segment_fixed_size'):>7s}  {get(r'.amdhsa_group_segment_fixed_size'):>3s}  {spills[name]:>6d}")
    return lines


def measure():
    import torch
    import mimi_amd as mimi
    from mimi_amd.integrators import CSRPattern, MortarContact, RigidPlane, RigidSphere
    dev = torch.device("cuda", 0)
    L = [m * CELL for m in N_EL]
    block = mimi.BSplinePatch.block(N_EL, 2, lengths=L)
    pattern = CSRPattern.of_bspline_patch(block, on_device=True)
    R = 0.25 * L[0]
    bodies = (("sphere (bench.py cfg4)", lambda: RigidSphere([0.5 * L[0], 0.5 * L[1], L[2] + 0.9 * R], R, PENALTY)),
              ("plane over the whole face", lambda: RigidPlane([0.0, 0.0, L[2] - 0.1 * CELL], [0.0, 0.0, -1.0], PENALTY)))
    u0 = torch.zeros(block.n_vdofs, dtype=torch.float64, device=dev)
    X = torch.from_numpy(block.control_points).to(dev)
    u1 = torch.zeros_like(X)
    u1[:, 0] = SHEAR * X[:, 0] / L[0]
    u1 = u1.reshape(-1).contiguous()
    x = torch.randn(block.n_vdofs, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y = torch.zeros_like(x)
    r = torch.zeros_like(x)
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

    lines = []
    for label, make in bodies:
        body = make()
        c = MortarContact(body, "contact", pattern, block, 2, 1).Prepare()
        c.SetFrictionAction(True)
        keys = [(mu, mode) for mu in (0.0, MU) for mode in (False, True)]
        times = {k: dict(action=[], linearize=[]) for k in keys}
        bytes_, counts, assembled = {}, None, {0.0: [], MU: []}
        for _ in range(ROUNDS):
            for mu in (0.0, MU):
                body.friction = mu
                if mu > 0.0:
                    c.ResetFriction()
                    c.BoundaryPostTimeAdvance(u0)
                    c.AddBoundaryResidual(u1, r)
                    c._history()
                    counts = (c.n_stick_, c.n_slip_)
                for mode in (False, True):
                    c.SetConsistentTangent(mode)
                    c.Linearize(u1)
                    assert c.HoldsFrictionRecord() == (mu > 0.0) and c.HoldsConsistentRecord() == mode
                    bytes_[(mu, mode)] = c.LinearizationBytes()
                    times[(mu, mode)]["action"].append(per_call_ms(lambda: c.ApplyTangent(x, y, 1.0)))
                    times[(mu, mode)]["linearize"].append(per_call_ms(lambda: c.Linearize(u1)))
                assembled[mu].append(per_call_ms(lambda: c.AddBoundaryResidualAndGrad(u1, 1.0, r, A), reps=20))
        active = int((c.AveragePressure() != 0).sum())
        lines.append(f"-- {label}: {c.n_marked_boundaries_} faces, {len(c.MarkedNodes())} marked nodes, {active} with pressure; "
                     f"with friction {counts[0]} points stick, {counts[1]} slip --")
        for mu, mode in keys:
            t = times[(mu, mode)]
            lines.append(f"{'friction  ' if mu else 'smooth    '} {'consistent' if mode else 'frozen    '}  action "
                         f"{statistics.median(t['action']):.4f} ms ({min(t['action']):.4f} .. {max(t['action']):.4f})   linearize "
                         f"{statistics.median(t['linearize']):.4f} ms ({min(t['linearize']):.4f} .. {max(t['linearize']):.4f})   "
                         f"record {bytes_[(mu, mode)]} bytes")
        for mode in (False, True):
            ratio = statistics.median(times[(MU, mode)]["action"]) / statistics.median(times[(0.0, mode)]["action"])
            lines.append(f"friction / smooth {'consistent' if mode else 'frozen'} action: {ratio:.2f}; friction record "
                         f"{bytes_[(MU, mode)] - bytes_[(0.0, mode)]} bytes")
        lines.append(f"assembled tangent (AddBoundaryResidualAndGrad, residual and row gather included): smooth "
                     f"{statistics.median(assembled[0.0]):.4f} ms, with friction {statistics.median(assembled[MU]):.4f} ms")
    return lines


if __name__ == "__main__":
    lines = ["scratch/friction_action_rate.py on one MI355X: ApplyTangent and Linearize of one contact handle with and without friction,",
             f"frozen and consistent, between device events, {REPS} calls per window, {ROUNDS} alternating rounds (median, lowest .. highest)."]
    if "--registers" in sys.argv:
        lines += register_table()
    lines += measure()
    print("\n".join(lines))
    path = os.path.join(ROOT, "profiles", "friction_action_rate.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
