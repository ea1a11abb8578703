"""One residual + Jacobian assembly of the north-star mesh (128 x 128 x 16 elements, degree 2) made periodic along x, as
NonlinearSolid's periodic route runs it: expand x_t, zero r_u / A_u, the domain integrator into the unwrapped structured
CSR, one fold into the folded r / J with A_base = M.  For rocprofv3 --kernel-trace --stats
(profiles/periodic_northstar.txt).  Also prints event times per phase.  Argument "cfg3": the same mesh at degree 3."""
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mimi_amd
from mimi_amd.integrators import CSRPattern, NonlinearSolid, PeriodicFold, periodic_node_map

REPS = 5
cfg3 = len(sys.argv) > 1 and sys.argv[1] == "cfg3"
n_el, p = ((128, 128, 16), 3) if cfg3 else ((128, 128, 16), 2)
patch = mimi_amd.BSplinePatch.block(n_el, p)
pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
mat = mimi_amd.CompressibleOgdenNeoHookean()
mat.density = 1.0
mat.set_young_poisson(2100, 0.3)
G = NonlinearSolid("domain", mat, pattern, patch=patch).Prepare()
dev = torch.device("cuda", 0)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
fold = PeriodicFold(pattern, periodic_node_map(patch.n_ctrl, [0]), 3).Prepare()
ev[1].record()
torch.cuda.synchronize()
print(f"{'cfg3' if cfg3 else 'north star'}: nnz_u {fold.nnz_u_}, nnz_f {fold.nnz_f_}, rows {fold.n_f_}, "
      f"fold set-up {ev[0].elapsed_time(ev[1]):.1f} ms")
rng = np.random.default_rng(0)
x_f = torch.from_numpy(0.01 * rng.standard_normal(fold.n_f_)).to(dev)
x_u = torch.zeros(fold.n_u_, dtype=torch.float64, device=dev)
r_u = torch.zeros_like(x_u)
A_u = torch.zeros(fold.nnz_u_, dtype=torch.float64, device=dev)
M = torch.from_numpy(rng.standard_normal(fold.nnz_f_)).to(dev)
y = torch.zeros(fold.n_f_, dtype=torch.float64, device=dev)
J = torch.empty_like(M)


def assembly(t=None):
    t = t or [None] * 5
    t[0] and t[0].record()
    fold.Expand(x_f, x_u)
    r_u.zero_()
    A_u.zero_()
    t[1] and t[1].record()
    G.AddDomainResidualAndGrad(x_u, 0.25, r_u, A_u)
    t[2] and t[2].record()
    fold.Add(r_u, y, A_u, M, J)
    t[3] and t[3].record()


assembly()
torch.cuda.synchronize()
acc = np.zeros(3)
for _ in range(REPS):
    t = [torch.cuda.Event(enable_timing=True) for _ in range(4)] + [None]
    assembly(t)
    torch.cuda.synchronize()
    acc += [t[0].elapsed_time(t[1]), t[1].elapsed_time(t[2]), t[2].elapsed_time(t[3])]
acc /= REPS
gb = (fold.nnz_u_ * (8 + 4) + fold.nnz_f_ * 16) / 1e9
print(f"expand + zero-fill {acc[0]:.3f} ms, domain {acc[1]:.3f} ms, fold {acc[2]:.3f} ms "
      f"({gb:.2f} GB of A_u, place map, A_base, A_f: {gb / acc[2]:.2f} TB/s)")
