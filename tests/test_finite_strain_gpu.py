"""J2Simo and J2Log on every kernel family against their 50-digit return maps, with no oracle in the loop: the moment
identities of test_closed_form_gpu.py for a homogeneous deformation u(X) = (F - I) X,

    sum_a X_(a,K) r_(a,i)      = V P_iK(F)                           (assembly and residual-only call)
    sum_a X_(a,K) (A w)_(a,i)  = V (dP/dF : dF)_iK,   w_b = dF X_b   (assembled tangent)

with P, dP and the committed state from tests/_finite_strain_return.py, on the named inputs of tests/_finite_strain_inputs.py:
(1) the elastic spectra -- coincident and nearly coincident principal stretches, rotations, the identity -- on a virgin handle:
    the eigen-solver's skip path, the divided difference of the logarithm at x == 0 and next to it, J2Simo's |s| ~ 0 normal,
    through the material pre-pass, the one-direction-at-a-time dual-number tangent and the tangent records;
(2) three plastic steps with turning principal axes: DomainPostTimeAdvance at F1, F2, F3 with every quadrature point's
    eqps / Fp_inv | be / F_old / temperature after each commit, and the assembly before each commit.
Bars: residual 1e-12 of V max(|P|, G), tangent 1e-11 of V max|dP| (the rounding bars of the moment sums); on the plastic
steps plus the stress bar derived in _finite_strain_return.py for that step and plus FINITE_STRAIN_TANGENT_BAR (measured on
the oracle, on the CPU: _finite_strain_inputs.py); committed state rtol 1e-9 + 1e-13, temperature 1e-12.
The kernel family is asserted after every assembly: (6, 4) p3 tensor_small, (4, 3, 4) p2 tensor_p2_two_phase, (3, 3, 4) p3
tensor_p3_two_phase, (3, 2, 2) p2 with MIMI_HIP_FORCE_GENERAL at create time: general.

Measured on the MI355X, worst over the four shapes (and the six laws):
  elastic  J2Log   residual 1.8e-15, tangent 3.7e-15;   J2Simo  residual 1.0e-15, tangent 4.9e-15
  plastic  J2Log   residual 2.4e-11 (7.7e-3 of its bar), tangent 2.4e-11, eqps 1.8e-10, Fp_inv 2.7e-12 (relative), T bit-equal
           J2Simo  residual 1.7e-11 (2.8e-3 of its bar), tangent 1.9e-11, eqps 5.9e-11, be 3.1e-12, T 1.8e-16 (relative)
  -- the figures of the host-compiled device code (test_finite_strain_cpu.py) to two digits on every kernel family."""
import os

import numpy as np
import pytest

import _finite_strain_inputs as fi
import _finite_strain_return as fs
from _cases import product_material
from test_closed_form_gpu import csr_times

pytestmark = pytest.mark.gpu

# (elements, degree, kernel family the assembly must run on)
SHAPES = [((6, 4), 3, "tensor_small"), ((4, 3, 4), 2, "tensor_p2_two_phase"), ((3, 3, 4), 3, "tensor_p3_two_phase"),
          ((3, 2, 2), 2, "general")]
SHAPE_IDS = [f"{'x'.join(map(str, s[0]))}p{s[1]}-{s[2]}" for s in SHAPES]
MODELS = list(fs.MODELS)


class Block:
    """a block with non-unit lengths, its integrator, and the moment sums of a homogeneous deformation"""

    def __init__(self, n_el, p, family, model, law):
        import torch
        import mimi_amd
        from mimi_amd.integrators import CSRPattern, NonlinearSolid
        self.dim, self.family = len(n_el), family
        patch = mimi_amd.BSplinePatch.block(n_el, p, [1.0 + 0.5 * d for d in range(self.dim)])
        self.dev = torch.device("cuda", 0)
        self.pattern = CSRPattern.of_bspline_patch(patch, on_device=True)
        if family == "general":
            os.environ["MIMI_HIP_FORCE_GENERAL"] = "1"          # read at create time
        try:
            self.G = NonlinearSolid("domain", product_material(model, law), self.pattern, patch=patch).Prepare()
        finally:
            if family == "general":
                del os.environ["MIMI_HIP_FORCE_GENERAL"]
        self.G.dt_ = fi.DT
        self.X = torch.from_numpy(np.ascontiguousarray(patch.control_points, dtype=np.float64)).to(self.dev)    # [n_nodes][dim]
        self.V = float(np.prod(patch.control_points.max(axis=0) - patch.control_points.min(axis=0)))
        self.n_vdofs = patch.n_vdofs

    def field(self, H):
        import torch
        return (self.X @ torch.from_numpy(np.ascontiguousarray(H)).to(self.dev).T).reshape(-1).contiguous()

    def moment(self, y):
        return (self.X.T @ y.reshape(-1, self.dim)).cpu().numpy().T          # [i][K]

    def assemble(self, F, dF):
        """(V P, V P of the residual-only call, V dP) as the kernels give them"""
        import torch
        u = self.field(F - np.eye(self.dim))
        r = torch.zeros(self.n_vdofs, dtype=torch.float64, device=self.dev)
        A = torch.zeros(self.pattern.nnz, dtype=torch.float64, device=self.dev)
        self.G.AddDomainResidualAndGrad(u, 1.0, r, A)
        assert self.G.LastKernelFamily() == self.family
        r2 = torch.zeros_like(r)
        self.G.AddDomainResidual(u, r2)
        assert self.G.LastKernelFamily() == self.family
        self.G.Synchronize()
        y = csr_times(self.pattern.rowptr, self.pattern.col, A, self.field(dF))
        return self.moment(r), self.moment(r2), self.moment(y)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", MODELS)
def test_elastic_spectra(model, shape):
    n_el, p, family = shape
    B = Block(n_el, p, family, model, fi.ELASTIC_LAW)
    dF, G, V = fi.direction(B.dim), fs.shear_modulus(), B.V
    worst_r = worst_k = 0.0
    for c in fi.elastic_cases(model, B.dim):
        Mr, Mr2, Mk = B.assemble(c.F, dF)
        assert np.all(np.isfinite(Mr)) and np.all(np.isfinite(Mr2)) and np.all(np.isfinite(Mk)), c.name
        err_r = max(np.abs(M - V * c.ref.P).max() for M in (Mr, Mr2)) / (V * max(np.abs(c.ref.P).max(), G))
        err_k = np.abs(Mk - V * c.dP).max() / (V * np.abs(c.dP).max())
        worst_r, worst_k = max(worst_r, err_r), max(worst_k, err_k)
        assert err_r < 1e-12, (c.name, err_r)
        assert err_k < 1e-11, (c.name, err_k)
    # nothing was committed: the handle is still virgin
    assert np.all(B.G.State("accumulated_plastic_strain") == 0.0)
    print(f"elastic spectra {model} {n_el} p{p} {family}: residual {worst_r:.2e} (bar 1e-12), tangent {worst_k:.2e} (bar 1e-11)")


def state_close(a, b):
    return np.allclose(a, b, rtol=1e-9, atol=1e-13)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("law", fi.PLASTIC_LAWS)
def test_three_noncoaxial_steps(law, model, shape):
    n_el, p, family = shape
    B = Block(n_el, p, family, model, law)
    dF, V = fi.direction(B.dim), B.V
    cases = fi.plastic_cases(model, law, B.dim)         # (plastic, margin >= 0.1 sigma_y, |Fp_inv - Fp_inv^T| > 1e-3: asserted there)
    T0 = float(fi.law_of(law).thermal["initial_temperature"])
    assert np.all(B.G.State("temperature") == T0)
    heats = model == "j2simo" and law == "JohnsonCookTempRate"
    worst = dict(r=0.0, k=0.0, eqps=0.0, m1=0.0, T=0.0)
    for k, c in enumerate(cases):
        # the assembly before the commit, from the state the kernels themselves committed
        Mr, Mr2, Mk = B.assemble(c.F, dF)
        scale = V * np.abs(c.ref.P).max()
        tol_r = 1e-12 + c.bar / np.abs(c.ref.P).max()
        tol_k = 1e-11 + fi.FINITE_STRAIN_TANGENT_BAR
        err_r = max(np.abs(M - V * c.ref.P).max() for M in (Mr, Mr2)) / scale
        err_k = np.abs(Mk - V * c.dP).max() / (V * np.abs(c.dP).max())
        print(f"{model} {law} {n_el} p{p} step {k + 1}: residual {err_r:.2e} (bar {tol_r:.2e}), tangent {err_k:.2e} (bar {tol_k:.2e})")
        worst["r"], worst["k"] = max(worst["r"], err_r / tol_r), max(worst["k"], err_k)
        assert err_r < tol_r and err_k < tol_k, (k, err_r, tol_r, err_k, tol_k)
        B.G.DomainPostTimeAdvance(B.field(c.F - np.eye(B.dim)))
        eqps, T, m1 = B.G.State("accumulated_plastic_strain"), B.G.State("temperature"), B.G.State("plastic_strain")
        worst["eqps"] = max(worst["eqps"], rel(eqps, np.float64(c.ref.eqps)))
        worst["m1"] = max(worst["m1"], rel(m1, c.ref.m1.T.ravel()))
        worst["T"] = max(worst["T"], rel(T, np.float64(c.ref.temperature)))
        assert state_close(eqps, c.ref.eqps), (k, rel(eqps, np.float64(c.ref.eqps)))
        assert state_close(m1, c.ref.m1.T.ravel()), (k, rel(m1, c.ref.m1.T.ravel()))      # [e, q, i + J dim]
        if model == "j2simo":
            assert state_close(B.G.State("state2"), c.ref.m2.T.ravel())                    # F_old
        assert np.allclose(T, c.ref.temperature, rtol=1e-12, atol=1e-12), (k, rel(T, np.float64(c.ref.temperature)))
        if heats:
            assert T.min() > c.T                     # it rises at every point, at every step
        else:
            assert np.all(T == T0)                   # bit-equal: J2Log under every law, J2Simo under the laws that do not heat
    if heats:
        assert cases[-1].ref.temperature > T0 + 1e-4
    print(f"{model} {law} {n_el} p{p} {family}: residual {worst['r']:.2e} of its bar, tangent {worst['k']:.2e}, eqps {worst['eqps']:.2e}, "
          f"first state matrix {worst['m1']:.2e}, T {worst['T']:.2e} (relative)")
