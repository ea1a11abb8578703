"""cfg4's contact integrator (96 x 96 faces of the 96 x 96 x 12 degree-2 block, a rigid sphere over the top face) with and
without friction, and against another build of the library on the same box:

    python scratch/friction_rate.py [--other DIR] [--rounds 3]

DIR is another checkout of the project with its library built (a `git worktree` of the parent commit, say): its package and
its library are used together.  Every measurement runs in a child process of its own, one at a time, the two checkouts
alternating; a child warms up, then times WINDOWS windows of
CALLS calls each between device synchronisations and prints the median and the spread of the windows.  mu = 0 is timed on
both libraries (residual + tangent, residual only); mu = 0.3 on this tree only: the same two calls after a commit at u and
a sideways increment (so that points stick and slip), the commit by the null form, and the post-advance with evaluation."""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WINDOWS, CALLS = 7, 200


def child(friction, root):
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import bench
    import mimi_amd
    from mimi_amd.integrators import CSRPattern, MortarContact, RigidSphere
    dev = torch.device("cuda", 0)
    patch = mimi_amd.BSplinePatch.block((96, 96, 12), 2)
    pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    L = patch.control_points.max(axis=0)
    R = 0.25 * L[0]
    c = 0.5 * L
    c[2] = L[2] + 0.9 * R
    body = RigidSphere(list(c), R, 1e4, **(dict(friction=0.3) if friction else {}))
    Cn = MortarContact(body, "contact", pattern, patch, 2, 1).Prepare()
    Cn.SetStream(stream.cuda_stream)
    u0 = bench.synthetic_u(patch, scale=0.01)
    u = torch.from_numpy(u0).to(dev)
    r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
    A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)

    def timed(f):
        for _ in range(20):
            f()
        out = []
        for _ in range(WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / CALLS * 1e3)
        out.sort()
        return out[len(out) // 2], out[0], out[-1]

    what = {}
    if friction:
        Cn.BoundaryPostTimeAdvance(u)
        shift = u0.reshape(-1, 3).copy()
        shift[:, 0] += 2.0e-3 * L[0]
        shift[:, 1] += 1.0e-3 * L[1]
        u = torch.from_numpy(shift.reshape(-1)).to(dev)
    what["R+J"] = timed(lambda: Cn.AddBoundaryResidualAndGrad(u, 1.0, r, A))
    what["R"] = timed(lambda: Cn.AddBoundaryResidual(u, r))
    note = ""
    if friction:
        Cn._history()
        note = f" stick {Cn.n_stick_} slip {Cn.n_slip_} of {Cn.n_marked_boundaries_ * Cn.n_q_} points"
        what["commit"] = timed(Cn.CommitFriction)
        Cn.ResetFriction()
        what["post-advance(u)"] = timed(lambda: check_call(Cn, u))
    print(" ".join(f"{k} {m:.4f} ms [{lo:.4f}, {hi:.4f}]" for k, (m, lo, hi) in what.items()) + note, flush=True)


def check_call(Cn, u):
    from mimi_amd import _capi
    _capi.check(_capi.lib().mimi_hip_contact_post_time_advance(Cn._handle(), _capi.fptr(u)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["plain", "friction"])
    ap.add_argument("--other", help="another built checkout, timed in alternation with this tree (mu = 0)")
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        child(args.child == "friction", args.root)
        return
    print(f"contact of cfg4 (9216 faces), median of {WINDOWS} windows of {CALLS} calls [fastest, slowest window]", flush=True)
    runs = []
    for k in range(args.rounds):
        if args.other:
            runs.append((f"other  mu=0   round {k}", "plain", os.path.abspath(args.other)))
        runs.append((f"tree   mu=0   round {k}", "plain", ROOT))
    runs.append(("tree   mu=0.3", "friction", ROOT))
    for label, mode, root in runs:
        env = dict(os.environ)
        env["MIMI_HIP_LIBRARY"] = os.path.join(root, "mimi_amd", "lib", "libmimi_hip.so")      # as built: no rebuild on import
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root], env=env,
                             stdout=subprocess.PIPE, text=True, timeout=240)
        if out.returncode != 0:
            print(f"{label}: the child ended with status {out.returncode}; stopping", flush=True)
            sys.exit(1)
        print(f"{label}: {out.stdout.strip().splitlines()[-1]}", flush=True)


if __name__ == "__main__":
    main()
