#!/usr/bin/env python3
"""Same launches, same bits: a fixed, seeded list of cases through the C ABI of the domain integrator, for comparing two
builds of the library (MIMI_HIP_LIBRARY=scratch/lib_parent.so, then the tree's own) across a refactor of its host side.

  python scratch/dispatch_trace.py [--atomics] > hashes.txt       one line per result: case, what, SHA-256 of the bytes
  python scratch/dispatch_trace.py --linear > hashes.txt          the linear-solver section alone (a refactor of csrc/krylov.hip)
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python scratch/dispatch_trace.py   (kernel trace alone, no counters)
  python scratch/dispatch_trace.py --compare-hashes A.txt B.txt
  python scratch/dispatch_trace.py --compare-traces DIR_A DIR_B   (kernel name, grid, workgroup, LDS) in dispatch order, of the
                                                                  library's own kernels (namespace mimi_hip); the runtime's
                                                                  copy and fill kernels are counted, not compared

Entries reached: create from tables and from a B-spline, residual, residual + tangent, from-base in its three residences,
post-time-advance, integrate + gather over partial windows, phase timing; point and nodal field output (the Cauchy stress,
and the accumulated plastic strain of a material with state), AddMass, AddDiffusion, AddBodyForce, and the tangent action
(Linearize at a seeded u, ApplyTangent with the stiffness alone, all three coefficients and the mass alone, x and a
pre-filled y on the host and in HBM) -- on every route: the
cases of the kernel families, the general kernels, flat tables with shape values, node_ids, the cut element box, the
smallest blocks with p + 2 elements along one direction and fewer than p + 1 along another (a node with full support, a
node clipped on both sides), one of them as an element box cut on both sides of its long axis, and two patches of
tests/_patches.py with a repeated interior knot (tensor route and general route).  Kernel families: 2-D degree 1-3, 3-D degree 1,
3-D degree 2 and 3 with neo-Hookean / J2 / a record material (tangent and residual-only also after a committed step), 3-D
degree 2 with node_ids and on an element box cut along the walked axis, the general kernels
(MIMI_HIP_FORCE_GENERAL) with a closed-form and a record material, the reference-FD tangent.  Switches:
MIMI_HIP_P3_CONTRACT flipped between two calls, MIMI_HIP_NO_STRUCTURED set between two creates.  Every route sums in a
fixed order, so every hash must agree.  The linear-solver section (csrc/krylov.hip; it closes every run): GMRES and CG with
preconditioner ids 0, 1, 2, every product form, a restarting and a cut solve, add_mult, eliminate, apply_preconditioner kinds
1 and 2, arrays on the host and in HBM -- SHA-256 of x, the iterations, the final norm in hex.  --atomics runs the general path's atomics route
(MIMI_HIP_GENERAL_NO_TWO_PHASE=1, read at every create and kept on the handle) instead, whose sums do not: trace it, do not compare its hashes."""
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sha(a):
    import numpy as np
    import torch
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def out(case, what, value):
    print(f"{case:44s} {what:14s} {value}", flush=True)


def run_linear():
    """csrc/krylov.hip through LinearSolver on systems of tests/_krylov_cases.py and one of tests/_kronecker_cases.py"""
    import numpy as np
    import torch
    import _krylov_cases as kc
    import _kronecker_cases as qc
    from mimi_amd.integrators import CSRPattern
    from mimi_amd.kronecker import KroneckerOperator
    from mimi_amd.linear import LinearSolver
    dev = torch.device("cuda", 0)
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()

    def solves(case, S, to, val, b, ids, kdims=(50,), max_iter=300):
        for pid in ids:
            S.preconditioner = pid
            for kdim in kdims:
                S.kdim, S.max_iter = kdim, max_iter
                x = S.Mult(to(val), to(b), to(np.full(len(b), np.nan)))
                out(case, f"gmres {pid[:4]} k{kdim}", f"{sha(host(x))} {S.final_iter_} {float(S.final_norm_).hex()} {S.converged_}")
            x = S.MultCG(to(val), to(b), to(np.full(len(b), np.nan)), max_iter=max_iter)
            out(case, f"cg {pid[:4]}", f"{sha(host(x))} {S.final_iter_} {float(S.final_norm_).hex()} {S.converged_}")

    for where in ("host", "device"):
        to = (lambda a: np.array(a, dtype=np.float64)) if where == "host" else (lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to(dev))
        ti = (lambda a: a) if where == "host" else (lambda a: torch.from_numpy(a).to(dev))
        # every product form (RowGroup 1, 2, 3 without and with node columns); kdim 5 restarts, max_iter 7 cuts mid-cycle
        for name in ("n7", "nodes17x2", "nodes12x3_dropped", "nodes12x3", "spd36_cg"):
            A, b = kc.system(name)
            rng = np.random.default_rng(83)
            ess = np.sort(rng.choice(A.shape[0], 3, replace=False)).astype(np.int64)
            S = LinearSolver(CSRPattern(ti(A.indptr.astype(np.int64)), ti(A.indices.astype(np.int32)), A.nnz), ess)
            case = f"linear {name} {where}"
            out(case, "form", f"{S.RowGroup()} {S.NodeColumns()}")
            solves(case, S, to, A.data, b, ("none", "jacobi"), kdims=(5, 50))
            solves(case + " cut7", S, to, A.data, b, ("jacobi",), kdims=(5,), max_iter=7)
            y = S.AddMult(to(A.data), to(seeded(A.shape[0], 84)), to(seeded(A.shape[0], 85)), alpha=-0.75)
            out(case, "add_mult", sha(host(y)))
            r, val = to(b), to(A.data)
            S.Eliminate(r, val)
            out(case, "eliminate r", sha(host(r)))
            out(case, "eliminate A", sha(host(val)))
            solves(case + " eliminated", S, to, host(val), host(r), ("jacobi",))
            z = S.ApplyPreconditioner(1, to(A.data), to(b), to(np.zeros(len(b))))
            out(case, "apply kind 1", sha(host(z)))
        # the Kronecker operator (id 2) on the matrices of two bent blocks, 2-D and 3-D; ids 0 and 1 on the same handle
        for name, fac0 in (("2d_p3_8x4", 1e-2), ("p2_6x4x2", 1.0)):
            o = qc.oracle_system(name, fac0)
            P, B = qc.solve_patch(name)
            S = LinearSolver(CSRPattern(ti(o.D.rowptr.astype(np.int64)), ti(o.D.col.astype(np.int32)), o.D.nnz), o.ess)
            S.SetKronecker(KroneckerOperator(B, o.ess, P.dim))
            S.SetKroneckerCoefficients(qc.RHO, qc.stiff(P.dim, fac0))
            case = f"linear kron {name} {where}"
            out(case, "form", f"{S.RowGroup()} {S.NodeColumns()}")
            solves(case, S, to, o.J.data, o.b, ("kronecker", "jacobi", "none", "kronecker"), kdims=(5, 50), max_iter=120)
            z = S.ApplyPreconditioner(2, None, to(o.b), to(np.zeros(len(o.b))))
            out(case, "apply kind 2", sha(host(z)))
            z = to(o.b)
            S.ApplyPreconditioner(2, None, z, z)
            out(case, "apply in place", sha(host(z)))
            z = S.ApplyPreconditioner(1, to(o.J.data), to(o.b), to(np.zeros(len(o.b))))
            out(case, "apply kind 1", sha(host(z)))


def seeded(n, seed, scale=1.0):
    import numpy as np
    return scale * np.random.default_rng(seed).standard_normal(n)


def run():
    import numpy as np
    import scipy.sparse as sp
    import torch
    import mimi_amd
    from _cases import product_material
    from mimi_amd.integrators import CSRPattern, NonlinearSolid
    dev = torch.device("cuda", 0)

    def handle(n_el, p, mat, env=None, **kw):
        patch = mimi_amd.BSplinePatch.block(n_el, p)
        pattern = CSRPattern.of_bspline_patch(patch)
        for k, v in (env or {}).items():
            os.environ[k] = v
        G = NonlinearSolid("trace", product_material(mat), pattern, patch=patch, **kw).Prepare()
        for k in env or {}:
            del os.environ[k]
        G.dt_ = 0.5
        return patch, pattern, G

    def assemblies(case, G, n_vdofs, nnz, mat, fd=False):
        """residual, residual + tangent, and for a material with state: commit, the state, the tangent again"""
        u = seeded(n_vdofs, 1, 0.05 if mat == "neohook" else 0.02)
        r = seeded(n_vdofs, 2)
        G.AddDomainResidual(u, r)
        out(case, "residual r", sha(r))
        r, A = seeded(n_vdofs, 2), seeded(nnz, 3)
        G.AddDomainResidualAndGrad(u, 0.37, r, A)
        out(case, "tangent r", sha(r))
        out(case, "tangent A", sha(A))
        out(case, "family", G.LastKernelFamily())
        if mat not in ("neohook", "stvk"):
            G.DomainPostTimeAdvance(seeded(n_vdofs, 4, 0.03))
            for what in ("accumulated_plastic_strain", "plastic_strain"):
                out(case, "state " + what[:7], sha(G.State(what)))
            r, A = seeded(n_vdofs, 2), seeded(nnz, 3)
            G.AddDomainResidualAndGrad(u, 0.37, r, A)
            out(case, "committed A", sha(A))
            r = seeded(n_vdofs, 2)
            G.AddDomainResidual(u, r)
            out(case, "committed r", sha(r))
        if fd:
            G.SetTangentMode(1)
            r, A = seeded(n_vdofs, 2), seeded(nnz, 3)
            G.AddDomainResidualAndGrad(u, 0.37, r, A)
            out(case, "fd A", sha(A))
            out(case, "fd family", G.LastKernelFamily())
            G.SetTangentMode(0)

    def fields_and_forms(case, G, dim, n_vdofs, nnz, mat):
        """point and nodal form of one stress field and (a material with state) one state field; the three linear forms"""
        n_nodes = n_vdofs // dim
        u = seeded(n_vdofs, 1, 0.05 if mat == "neohook" else 0.02)
        for name in ["cauchy_stress"] + ([] if mat in ("neohook", "stvk") else ["accumulated_plastic_strain"]):
            out(case, "point " + name[:6], sha(G.PointField(name, u)))
            ncomp = G.FieldComponents(name)
            s, w = seeded(n_nodes * ncomp, 6).reshape(n_nodes, ncomp), seeded(n_nodes, 7)
            G.NodalField(name, u, s, w)
            out(case, "nodal " + name[:6], sha(s))
            out(case, "weight " + name[:6], sha(w))
        M, D, f = seeded(nnz, 8), seeded(nnz, 9), seeded(n_vdofs, 10)
        G.AddMass(1.3, M)
        G.AddDiffusion(0.7, D)
        G.AddBodyForce([0.3, -0.2, 0.5][:dim], f)
        out(case, "mass", sha(M))
        out(case, "diffusion", sha(D))
        out(case, "body force", sha(f))

    def actions(case, G, n_vdofs, mat):
        """Linearize, then y += (density M + stiffness K + viscosity C) x on a pre-filled y, arrays on the host and in HBM"""
        G.Linearize(seeded(n_vdofs, 1, 0.05 if mat == "neohook" else 0.02))
        x = seeded(n_vdofs, 12)
        for density, stiffness, viscosity in ((0.0, 1.0, 0.0), (0.7, 0.37, 0.11), (1.0, 0.0, 0.0)):
            what = f"{density:g} {stiffness:g} {viscosity:g}"
            y = G.ApplyTangent(x, seeded(n_vdofs, 13), stiffness=stiffness, density=density, viscosity=viscosity)
            out(case, "action " + what, sha(y))
            y = G.ApplyTangent(torch.from_numpy(x).to(dev), torch.from_numpy(seeded(n_vdofs, 13)).to(dev), stiffness=stiffness,
                               density=density, viscosity=viscosity)
            G.Synchronize()
            out(case, "action hbm " + what, sha(y))
        out(case, "action family", G.LastActionFamily())

    def from_base(case, G, n_vdofs, nnz):
        u, base = seeded(n_vdofs, 1, 0.05), seeded(nnz, 5, 50.0)
        to = lambda a, on_dev: torch.from_numpy(a.copy()).to(dev) if on_dev else a.copy()
        for name, (base_dev, out_dev) in {"device": (True, True), "host": (False, False), "host base": (False, True)}.items():
            r, A = to(seeded(n_vdofs, 2), out_dev), to(np.full(nnz, 1e30), out_dev)
            G.AddDomainResidualAndGradFrom(to(u, out_dev), 0.37, r, to(base, base_dev), A)
            G.Synchronize()
            out(case, "from " + name, sha(A))

    if "--linear" in sys.argv:
        return run_linear()
    if "--atomics" in sys.argv:
        os.environ["MIMI_HIP_GENERAL_NO_TWO_PHASE"] = "1"
        for n_el, p, mat in [((4, 3), 2, "neohook"), ((3, 2, 2), 2, "j2simo")]:
            patch, pattern, G = handle(n_el, p, mat, env={"MIMI_HIP_FORCE_GENERAL": "1"})
            case = f"atomics {'x'.join(map(str, n_el))} p{p} {mat}"
            assemblies(case, G, patch.n_vdofs, pattern.nnz, mat)
            from_base(case, G, patch.n_vdofs, pattern.nnz)
        return

    # every kernel family, from a B-spline
    for n_el, p, mat in [((5, 4), 1, "neohook"), ((4, 3), 2, "neohook"), ((3, 3), 3, "neohook"), ((3, 3), 3, "j2"), ((4, 3), 2, "j2linear"),
                         ((4, 3, 2), 1, "neohook"), ((3, 2, 2), 1, "j2log"),
                         ((5, 4, 4), 2, "neohook"), ((4, 4, 5), 2, "j2"), ((3, 4, 4), 2, "stvk"), ((3, 3, 4), 2, "j2simo"),
                         ((3, 2, 3), 3, "neohook"), ((2, 3, 5), 3, "j2"), ((2, 3, 2), 3, "stvk"), ((2, 2, 3), 3, "j2log")]:
        patch, pattern, G = handle(n_el, p, mat)
        assemblies(f"bspline {'x'.join(map(str, n_el))} p{p} {mat}", G, patch.n_vdofs, pattern.nnz, mat, fd=len(n_el) == 2 or p == 1)
        fields_and_forms(f"bspline {'x'.join(map(str, n_el))} p{p} {mat}", G, len(n_el), patch.n_vdofs, pattern.nnz, mat)
        actions(f"bspline {'x'.join(map(str, n_el))} p{p} {mat}", G, patch.n_vdofs, mat)
        if mat == "neohook":
            from_base(f"bspline {'x'.join(map(str, n_el))} p{p} {mat}", G, patch.n_vdofs, pattern.nnz)
    # the general kernels: closed-form and record materials, small and large elements
    for n_el, p, mat in [((4, 3), 2, "neohook"), ((3, 3), 3, "j2"), ((3, 2, 2), 2, "neohook"), ((3, 2, 2), 2, "j2simo"),
                         ((2, 2, 1), 3, "neohook"), ((2, 1, 2), 3, "stvk"), ((3, 2, 2), 1, "j2linear")]:
        patch, pattern, G = handle(n_el, p, mat, env={"MIMI_HIP_FORCE_GENERAL": "1"})
        case = f"general {'x'.join(map(str, n_el))} p{p} {mat}"
        assemblies(case, G, patch.n_vdofs, pattern.nnz, mat, fd=True)
        fields_and_forms(case, G, len(n_el), patch.n_vdofs, pattern.nnz, mat)
        actions(case, G, patch.n_vdofs, mat)
        if mat == "neohook":
            from_base(case, G, patch.n_vdofs, pattern.nnz)
    # create from flat tables (the oracle's own tables)
    from _cases import oracle_material
    from oracle import iga, ref_path as rp
    for n_el, p, mat in [((2, 2), 3, "j2"), ((3, 2, 2), 2, "neohook")]:
        P = iga.Patch.block(n_el, p)
        D = rp.DomainOracle(P, oracle_material(mat), n_threads=1)
        pattern = CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)
        tables = dict(dim=P.dim, n_nodes=P.n_nodes, dofs=D.conn, dN_dX=D.dN_dX, weight_det=D.weight * D.det,
                      N=np.ascontiguousarray(D.tables["N"]))
        G = NonlinearSolid("trace", product_material(mat), pattern, tables=tables).Prepare()
        G.dt_ = 0.5
        case = f"tables {'x'.join(map(str, n_el))} p{p} {mat}"
        assemblies(case, G, P.n_vdofs, D.nnz, mat, fd=True)
        fields_and_forms(case, G, P.dim, P.n_vdofs, D.nnz, mat)
        actions(case, G, P.n_vdofs, mat)
        from_base(case, G, P.n_vdofs, D.nnz)
    # permuted numbering (node_ids), 3-D degree 2 and 3: the caller's CSR is the lexicographic one renumbered
    for n_el, p in [((5, 4, 4), 2), ((3, 3, 4), 3)]:
        patch = mimi_amd.BSplinePatch.block(n_el, p)
        lex = CSRPattern.of_bspline_patch(patch)
        perm = np.random.default_rng(11).permutation(patch.n_nodes).astype(np.int64)
        dofperm = (perm[:, None] * 3 + np.arange(3)[None, :]).ravel()
        rows = np.repeat(np.arange(patch.n_vdofs), np.diff(lex.rowptr))
        S = sp.coo_matrix((np.ones(lex.nnz), (dofperm[rows], dofperm[lex.col])), shape=(patch.n_vdofs,) * 2).tocsr()
        S.sort_indices()
        pattern = CSRPattern(S.indptr.astype(np.int64), S.indices.astype(np.int32), lex.nnz)
        for mat in ("neohook", "j2"):
            G = NonlinearSolid("trace", product_material(mat), pattern, patch=patch, node_ids=perm).Prepare()
            G.dt_ = 0.5
            assemblies(f"node_ids {'x'.join(map(str, n_el))} p{p} {mat}", G, patch.n_vdofs, pattern.nnz, mat)
            fields_and_forms(f"node_ids {'x'.join(map(str, n_el))} p{p} {mat}", G, 3, patch.n_vdofs, pattern.nnz, mat)
            actions(f"node_ids {'x'.join(map(str, n_el))} p{p} {mat}", G, patch.n_vdofs, mat)
    # integrate + gather over partial windows, phase timing on (which event pairs exist is what is printed, not the times)
    for n_el, p, mat in [((5, 7, 4), 2, "neohook"), ((4, 6, 5), 2, "j2"), ((3, 4, 4), 2, "stvk"), ((3, 5, 4), 3, "j2")]:
        patch = mimi_amd.BSplinePatch.block(n_el, p)
        pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
        G = NonlinearSolid("trace", product_material(mat), pattern, patch=patch).Prepare()
        G.dt_ = 0.5
        G.SetPhaseTiming(True)
        case = f"two-step {'x'.join(map(str, n_el))} p{p} {mat}"
        u = torch.from_numpy(seeded(patch.n_vdofs, 1, 0.02)).to(dev)
        r, A = torch.zeros(patch.n_vdofs, dtype=torch.float64, device=dev), torch.zeros(pattern.nnz, dtype=torch.float64, device=dev)
        G.AddDomainResidualAndGrad(u, 0.7, r, A)
        G.Synchronize()
        out(case, "one call A", sha(A))
        out(case, "prepass timed", G.PhaseMsDetail()[0] > 0.0)
        r2, A2 = torch.zeros_like(r), torch.zeros_like(A)
        G.Integrate(u)
        hi = [n_el[d] + p for d in range(3)]
        cuts = [0, 1, 1 + hi[1] // 2, hi[1]]
        for y0, y1 in zip(cuts[:-1], cuts[1:]):
            G.Gather(0.7, r2, A2, [0, y0, 0], [hi[0], y1, hi[2]])
            G.Synchronize()
            out(case, f"gather y<{y1}", sha(A2))
        out(case, "gather r", sha(r2))
        out(case, "prepass timed", G.PhaseMsDetail()[0] > 0.0)
        G.SetPhaseTiming(False)
        r = torch.zeros_like(r)
        G.AddDomainResidual(u, r)
        G.Synchronize()
        out(case, "residual r", sha(r))
    # degree 2, an element box cut along the walked (third) axis and along one other
    for mat in ("neohook", "j2", "j2simo"):
        patch, pattern, G = handle((5, 6, 8), 2, mat, element_box=([0, 1, 2], [5, 5, 6]))
        assemblies(f"element box 5x6x8 p2 {mat}", G, patch.n_vdofs, pattern.nnz, mat)
        fields_and_forms(f"element box 5x6x8 p2 {mat}", G, 3, patch.n_vdofs, pattern.nnz, mat)
        actions(f"element box 5x6x8 p2 {mat}", G, patch.n_vdofs, mat)
    # fields and forms on the smallest blocks with an interior node of full support and a node clipped on both sides; the
    # 3-D ones again as an element box cut on both sides of the long axis
    for p in (1, 2, 3):
        for n_el in ((p + 2, p), (p + 2, p, 2)):
            for env in (None, {"MIMI_HIP_FORCE_GENERAL": "1"}):
                patch, pattern, G = handle(n_el, p, "j2", env=env)
                case = f"{'general' if env else 'small'} {'x'.join(map(str, n_el))} p{p} j2"
                G.DomainPostTimeAdvance(seeded(patch.n_vdofs, 4, 0.03))
                fields_and_forms(case, G, len(n_el), patch.n_vdofs, pattern.nnz, "j2")
                actions(case, G, patch.n_vdofs, "j2")
        patch, pattern, G = handle((p + 4, p, 2), p, "j2", element_box=([1, 0, 0], [p + 3, p, 2]))
        G.DomainPostTimeAdvance(seeded(patch.n_vdofs, 4, 0.03))
        fields_and_forms(f"cut box {p + 4}x{p}x2 p{p} j2", G, 3, patch.n_vdofs, pattern.nnz, "j2")
        actions(f"cut box {p + 4}x{p}x2 p{p} j2", G, patch.n_vdofs, "j2")
    # repeated interior knots: the tensor route (small elements) and the general route
    import _patches
    for name in ("rep2d_p2", "rep3d_p2"):
        P, B = _patches.patches(name)
        D = rp.DomainOracle(P, oracle_material("j2"), n_threads=1)
        pattern = CSRPattern(D.rowptr.astype(np.int64), D.col.astype(np.int32), D.nnz)
        G = NonlinearSolid("trace", product_material("j2"), pattern, patch=B).Prepare()
        G.dt_ = 0.5
        assemblies(f"patches {name} j2", G, P.n_vdofs, D.nnz, "j2")
        fields_and_forms(f"patches {name} j2", G, P.dim, P.n_vdofs, D.nnz, "j2")
        actions(f"patches {name} j2", G, P.n_vdofs, "j2")
    # MIMI_HIP_P3_CONTRACT flipped between two calls of one handle
    patch, pattern, G = handle((2, 3, 4), 3, "neohook")
    u = seeded(patch.n_vdofs, 1, 0.05)
    for variant in ("cxx", "asm", "cxx"):
        os.environ["MIMI_HIP_P3_CONTRACT"] = variant
        r, A = seeded(patch.n_vdofs, 2), seeded(pattern.nnz, 3)
        G.AddDomainResidualAndGrad(u, 0.37, r, A)
        out("p3 contract switch", variant + " A", sha(A))
    del os.environ["MIMI_HIP_P3_CONTRACT"]
    # MIMI_HIP_NO_STRUCTURED set between two creates
    for env in (None, {"MIMI_HIP_NO_STRUCTURED": "1"}, None):
        patch, pattern, G = handle((4, 3, 3), 2, "neohook", env=env)
        assemblies("no-structured " + ("set" if env else "unset"), G, patch.n_vdofs, pattern.nnz, "neohook")
    run_linear()


def compare_hashes(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    la, lb = [l for l in la if not l.startswith("atomics")], [l for l in lb if not l.startswith("atomics")]
    bad = [(x, y) for x, y in zip(la, lb) if x != y]
    for x, y in bad[:20]:
        print(f"- {x}\n+ {y}")
    print(f"{len(la)} / {len(lb)} lines, {len(bad)} differ" + ("" if len(la) == len(lb) else ": DIFFERENT LENGTHS"))
    return 1 if bad or len(la) != len(lb) or not la else 0


def launches(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit(f"{directory}: {len(files)} kernel traces")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
             r["Workgroup_Size_Z"], r["LDS_Block_Size"]) for r in rows]


def own_launches(directory):
    """the library's launches, the two gathers of older builds read as the one node gather; the number of other dispatches"""
    rows = launches(directory)
    own = []
    for r in rows:
        if "mimi_hip" in r[0]:
            gather = any(k in r[0] for k in ("field_gather_kernel", "apply_gather_kernel", "node_gather_kernel"))
            own.append((("mimi_hip::node_gather_kernel" if gather else r[0]),) + r[1:])
    return own, len(rows) - len(own)


def compare_traces(a, b):
    (la, other_a), (lb, other_b) = own_launches(a), own_launches(b)
    print(f"other dispatches (the runtime's copy and fill kernels): {other_a} / {other_b}")
    bad = [(k, x, y) for k, (x, y) in enumerate(zip(la, lb)) if x != y]
    for k, x, y in bad[:10]:
        print(f"dispatch {k}:\n- {x}\n+ {y}")
    print(f"{len(la)} / {len(lb)} launches, {len(set(x[0] for x in la))} distinct kernels, {len(bad)} differ"
          + ("" if len(la) == len(lb) else ": DIFFERENT LENGTHS"))
    return 1 if bad or len(la) != len(lb) or not la else 0


if __name__ == "__main__":
    if "--compare-hashes" in sys.argv:
        sys.exit(compare_hashes(*sys.argv[-2:]))
    if "--compare-traces" in sys.argv:
        sys.exit(compare_traces(*sys.argv[-2:]))
    run()
