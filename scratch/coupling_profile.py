"""The coupling surface at north-star size (128 x 128 x 16 elements, degree 2; top face: 16 384 faces x 16 points):
points(u) and set_traction(t, u) as a coupling iteration calls them.  For rocprofv3 --kernel-trace --stats
(profiles/coupling_surface_northstar.txt, with the command lines).  Prints event times per call and the bytes each call
must move, from the shapes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mimi_amd
from mimi_amd.integrators import CouplingSurface

REPS = 20
patch = mimi_amd.BSplinePatch.block((128, 128, 16), 2)
s = CouplingSurface(patch, 2, 1).Prepare()
dim, nf, nq, nd = 3, s.n_faces_, s.n_q_, (patch.degrees[0] + 1) ** 2
npts = s.n_points_
n_fnodes = patch.n_ctrl[0] * patch.n_ctrl[1]
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
u = torch.from_numpy(0.01 * rng.standard_normal(patch.n_vdofs)).to(dev)
t = torch.from_numpy(rng.standard_normal((npts, dim))).to(dev)
x = torch.empty((npts, dim), dtype=torch.float64, device=dev)
n = torch.empty_like(x)
w = torch.empty(npts, dtype=torch.float64, device=dev)
f = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev)

# bytes from the shapes: tables N, dN, weight, dofs; the face nodes' X and u; the outputs / t, face vector, gather
tables = npts * nd * 8 + npts * nd * (dim - 1) * 8 + npts * 8 + nf * nd * 4
state = 2 * n_fnodes * dim * 8
points_bytes = tables + state + npts * (2 * dim + 1) * 8
face_bytes = tables + state + npts * dim * 8 + nf * nd * dim * 8
gather_bytes = nf * nd * 4 + (n_fnodes + 1) * 4 + n_fnodes * 4 + nf * nd * dim * 8 + 2 * n_fnodes * dim * 8


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(REPS):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / REPS


t_points = timed(lambda: s.Points(u, x, n, w))
t_load = timed(lambda: s.AddLoad(u, t, f))
t_set = timed(lambda: s.set_traction(t, u))
print(f"north star top face: {nf} faces x {nq} points = {npts} points, {nd} nodes per face, {n_fnodes} face nodes")
print(f"points      {t_points * 1e3:8.1f} us per call  ({points_bytes / 1e6:.1f} MB: {points_bytes / (t_points * 1e-3) / 1e12:.2f} TB/s)")
print(f"add_load    {t_load * 1e3:8.1f} us per call  (face pass {face_bytes / 1e6:.1f} MB + gather {gather_bytes / 1e6:.1f} MB: "
      f"{(face_bytes + gather_bytes) / (t_load * 1e-3) / 1e12:.2f} TB/s)")
print(f"set_traction (zero fill of f + add_load) {t_set * 1e3:8.1f} us per call")
