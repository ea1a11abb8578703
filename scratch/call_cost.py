"""Host cost of one call: wall time per call over 1 000 back-to-back AddDomainResidualAndGrad calls on a 2-D 2 x 2 degree-3
patch with device-resident arrays (a mesh so small that the call is its host side: argument classification, dispatch,
launches).  Prints one line; run once per library (MIMI_HIP_LIBRARY) in a fresh process."""
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import torch  # noqa: E402
import mimi_amd  # noqa: E402
from mimi_amd.integrators import CSRPattern, NonlinearSolid  # noqa: E402

patch = mimi_amd.BSplinePatch.block((2, 2), 3)
pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
mat = mimi_amd.CompressibleOgdenNeoHookean()
mat.density = 1.0
mat.set_young_poisson(2100, 0.3)
G = NonlinearSolid("cost", mat, pattern, patch=patch).Prepare()
dev = torch.device("cuda", 0)
u = 0.01 * torch.randn(patch.n_vdofs, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1))
r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
for _ in range(200):
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
G.Synchronize()
t0 = time.perf_counter()
for _ in range(1000):
    G.AddDomainResidualAndGrad(u, 1.0, r, A)
t1 = time.perf_counter()
G.Synchronize()
print(f"call_cost {os.environ.get('MIMI_HIP_LIBRARY', 'tree')}: {(t1 - t0) * 1e3:.3f} us per call issued, "
      f"{(time.perf_counter() - t0) * 1e3:.3f} us per call completed ({G.LastKernelFamily()})")
