"""Time of the field output against the residual-only assembly of the same handle, in one process: the north-star handle
(128 x 128 x 16, degree 2, neo-Hookean) and cfg3 (degree 3, J2, after one state commit).  After a warm-up, 20 rounds
alternate a residual-only assembly with each of: nodal von Mises stress, nodal Cauchy stress, point Cauchy stress; every
call between two device events.  Medians and spread (min, max) per call kind.

    python scratch/field_time.py [northstar cfg3] [--rounds 20] [--out profiles/fields_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import torch  # noqa: E402
import bench  # noqa: E402
import mimi_amd  # noqa: E402
from mimi_amd.integrators import CSRPattern, NonlinearSolid  # noqa: E402


def measure(workload, rounds, warmup=3):
    n_el, p, material = bench.WORKLOADS[workload][:3]
    dev = torch.device("cuda", 0)
    patch = mimi_amd.BSplinePatch.block(n_el, p)
    pattern = CSRPattern.of_bspline_patch(patch, device=0, on_device=True)
    G = NonlinearSolid(workload, bench.make_material(material), pattern, patch=patch).Prepare()
    G.dt_ = 0.05
    f = lambda a: torch.from_numpy(a).to(dev)
    u = f(bench.synthetic_u(patch, scale=0.05 if material == "neohookean" else 0.02))
    if material != "neohookean":
        G.DomainPostTimeAdvance(f(bench.synthetic_u(patch, scale=0.03, seed=7)))
    n_nodes, n_pts = patch.n_nodes, G.n_elements_ * G.n_quad_
    r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
    s1, s9 = (torch.zeros((n_nodes, c), dtype=torch.float64, device=dev) for c in (1, 9))
    w = torch.zeros(n_nodes, dtype=torch.float64, device=dev)
    pts = torch.empty((G.n_elements_, G.n_quad_, 9), dtype=torch.float64, device=dev)
    calls = {
        "residual-only assembly": lambda: G.AddDomainResidual(u, r),
        "nodal von_mises_stress": lambda: G.NodalField("von_mises_stress", u, s1, w),
        "nodal cauchy_stress": lambda: G.NodalField("cauchy_stress", u, s9, w),
        "point cauchy_stress": lambda: G.PointField("cauchy_stress", u, pts),
    }
    fields = [k for k in calls if k != "residual-only assembly"]
    times = {k: [] for k in calls}

    def timed(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        calls[name]()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(warmup):
        for name in calls:
            timed(name)
    for _ in range(rounds):
        for name in fields:                      # residual, field, residual, field, ...
            times["residual-only assembly"].append(timed("residual-only assembly"))
            times[name].append(timed(name))
    base = float(np.median(times["residual-only assembly"]))
    lines = [f"{workload}: {'x'.join(map(str, n_el))} elements, degree {p}, {material}; {n_pts} quadrature points, {n_nodes} nodes; "
             f"kernel family of the assembly: {G.LastKernelFamily()}; per-point tables held after the field calls: "
             f"{int(G.HoldsGradientTables())}"]
    for name, t in times.items():
        t = np.asarray(t)
        lines.append(f"  {name:26s} median {np.median(t):8.3f} ms   min {t.min():8.3f}   max {t.max():8.3f}   n = {len(t):3d}   "
                     f"{np.median(t) / base:5.2f} x the residual-only assembly")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["northstar", "cfg3"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"scratch/field_time.py: device events around every call, {args.rounds} rounds alternating a residual-only assembly "
             f"with each field call, after 3 warm-up rounds; {torch.cuda.get_device_name(0)}"]
    for wl in args.workloads:
        lines += measure(wl, args.rounds)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
