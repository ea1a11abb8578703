"""usage: scratch/p2_ablate.py [WORKLOAD [MATERIAL]]   (bench.WORKLOADS name, default northstar; material default: the workload's)

Phase times of the degree-2 two-phase path for the library named by MIMI_HIP_LIBRARY (same-box A/B timing: python -m
mimi_amd.build --out, one fresh process per run): material pre-pass, integration kernel and row gather of the tangent
assembly by the library's phase events, the residual-only assembly by device events around the call, after warm-up."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench, mimi_amd
from mimi_amd.integrators import CSRPattern, NonlinearSolid
n_el, p, material = bench.WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "northstar"]
if len(sys.argv) > 2:
    material = sys.argv[2]
patch = mimi_amd.BSplinePatch.block(n_el, p)
pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
G = NonlinearSolid("d", bench.make_material(material), pattern, patch=patch).Prepare()
G.dt_ = 0.5
dev = torch.device("cuda", 0)
u = torch.from_numpy(bench.synthetic_u(patch)).to(dev)
r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
for _ in range(3):
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
G.SetPhaseTiming(True)
acc = np.zeros(3)
n = 10
for _ in range(n):
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
    acc += G.PhaseMsDetail()
acc /= n
G.SetPhaseTiming(False)
r2 = torch.zeros_like(r)
for _ in range(3):
    G.AddDomainResidual(u, r2)
G.Synchronize()
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0.record()
for _ in range(n):
    G.AddDomainResidual(u, r2)
t1.record()
t1.synchronize()
print(os.environ.get("MIMI_HIP_LIBRARY", "default"), "x".join(map(str, n_el)), material,
      "pre-pass %.3f ms  phase 1 %.3f ms  phase 2 %.3f ms  sum %.3f ms  residual-only %.3f ms" % (*acc, acc.sum(), t0.elapsed_time(t1) / n))
print("   checksum r %.15e  A %.15e  r-only %.15e" % (float(r.abs().sum()), float(A.abs().sum()), float(r2.abs().sum())))
