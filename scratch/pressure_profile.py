"""Follower pressure on one 128 x 128 face of the north-star mesh (128 x 128 x 16 elements, degree 2: 16 384 faces, 16
points per face): residual-only and residual + tangent assemblies on device buffers, for rocprofv3 --kernel-trace --stats
(profiles/pressure_northstar_face_kernel_stats.csv).  Also prints event times per call."""
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mimi_amd
from mimi_amd.integrators import CSRPattern, FollowerPressure

REPS = 20
patch = mimi_amd.BSplinePatch.block((128, 128, 16), 2)
pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
fp = FollowerPressure("pressure", pattern, patch, 2, 1).Prepare()
fp.SetPressure(2.0)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
u = torch.from_numpy(0.01 * rng.standard_normal(patch.n_vdofs)).to(dev)
r = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)
A = torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
print(f"faces {fp.n_faces_}, face nodes {len(fp.FaceNodes())}, nnz {pattern.nnz}")
for label, call in (("residual", lambda: fp.AddBoundaryResidual(u, r)),
                    ("residual+tangent", lambda: fp.AddBoundaryResidualAndGrad(u, 1.0, r, A))):
    call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPS):
        call()
    t1.record()
    torch.cuda.synchronize()
    print(f"{label}: {t0.elapsed_time(t1) / REPS:.4f} ms per call (events, {REPS} calls)")
