"""The callers' steps around the assembly, device-resident: essential-dof elimination (forms/nonlinear.hpp:76-80,
112-115) and the reference's iterative linear solver (py/py_nonlinear_solid.cpp:329-339: mfem::GMRESSolver with an
mfem::DSmoother preconditioner) -- ctypes front-end of csrc/krylov.hip."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ABI, check, fptr, ptr


class LinearSolver(_capi.Handle):
    """One per CSR pattern and list of essential dofs.  Vectors / CSR values may be numpy arrays (staged) or torch
    device tensors (in place)."""
    _prefix = "linear"

    # mfem::GMRESSolver as configured by the reference (py_nonlinear_solid.cpp:331-336); kdim: mfem's default m
    rel_tol = 1e-8
    abs_tol = 1e-12
    max_iter = 300
    kdim = 50
    # "jacobi": mfem::DSmoother, the reference's; "kronecker": the fast-diagonalisation operator of SetKronecker;
    # "block_jacobi": the inverted dim x dim node blocks (SetNodeBlock); "none"
    preconditioner = "jacobi"
    _PRECONDITIONER_IDS = {"none": ABI.PRECOND_NONE, "jacobi": ABI.PRECOND_JACOBI, "kronecker": ABI.PRECOND_KRONECKER,
                           "block_jacobi": ABI.PRECOND_BLOCK_JACOBI}

    @property
    def use_jacobi(self):
        """the boolean this attribute used to be: True for "jacobi"; assigning True / False selects "jacobi" / "none" """
        return self.preconditioner == "jacobi"

    @use_jacobi.setter
    def use_jacobi(self, on):
        self.preconditioner = "jacobi" if on else "none"

    def _preconditioner_id(self):
        try:
            return self._PRECONDITIONER_IDS[self.preconditioner]
        except KeyError:
            raise ValueError(f"preconditioner {self.preconditioner!r}: one of {sorted(self._PRECONDITIONER_IDS)}") from None

    def __init__(self, pattern, essential_dofs=None, device=0):
        self.pattern_ = pattern
        self.n_ = int(len(pattern.rowptr) - 1) if not hasattr(pattern.rowptr, "numel") else int(pattern.rowptr.numel() - 1)
        ess = np.ascontiguousarray(essential_dofs if essential_dofs is not None else np.zeros(0), dtype=np.int64)
        self._keep = (pattern.rowptr, pattern.col, ess)   # device arrays are used in place by the library
        h = C.c_void_p()
        check(_capi.lib().mimi_hip_linear_create(self.n_, ptr(pattern.rowptr, "int64"), ptr(pattern.col, "int32"),
                                                 ptr(ess, "int64") if ess.size else None,
                                                 ess.size, device, C.byref(h)))
        self._h = h
        self.final_iter_, self.final_norm_, self.converged_ = 0, 0.0, False

    def RowGroup(self):
        """consecutive rows sharing one column list that the products read once (3, 2 or 1)"""
        return int(_capi.lib().mimi_hip_linear_info(self._h, ABI.LINEAR_INFO_ROW_GROUP))

    def NodeColumns(self):
        """True when the shared column list of a node's rows is made of node triples and is read as one index per node"""
        return bool(_capi.lib().mimi_hip_linear_info(self._h, ABI.LINEAR_INFO_NODE_COLUMNS))

    def Eliminate(self, r=None, A_values=None):
        """r[ess] = 0; A.EliminateRowCol(ess, DIAG_ONE)"""
        self._follow_torch(r, A_values)
        check(_capi.lib().mimi_hip_linear_eliminate(self._h, fptr(r), fptr(A_values)))

    def AddMult(self, A_values, x, y, alpha=1.0):
        """y += alpha A x (mfem::SparseMatrix::AddMult)"""
        self._follow_torch(A_values, x, y)
        check(_capi.lib().mimi_hip_linear_add_mult(self._h, fptr(A_values), fptr(x), float(alpha), fptr(y)))
        return y

    def SetKronecker(self, op):
        """the eigen-decompositions of a mimi_amd.kronecker.KroneckerOperator (copied to the device); the coefficients
        follow with SetKroneckerCoefficients"""
        n_dir = np.ascontiguousarray(op.n_dir, dtype=np.int32)
        check(_capi.lib().mimi_hip_linear_set_kronecker(self._h, int(op.dim), ptr(n_dir, "int32"), fptr(op.U), fptr(op.lam)))

    def SetKroneckerCoefficients(self, mass, stiff):
        """P_c = mass (x) M_d + sum_d stiff[c * dim + d] K_d (x) M...: rebuilds the scaling array on the device"""
        stiff = np.ascontiguousarray(stiff, dtype=np.float64).ravel()
        check(_capi.lib().mimi_hip_linear_set_kronecker_coefficients(self._h, float(mass), fptr(stiff)))

    def ApplyPreconditioner(self, kind, A_values, r, z):
        """z = M r as the solvers apply it: kind "jacobi" / 1 (needs A_values, or None with SetOperatorDiagonal armed),
        "kronecker" / 2 (A_values may be None) or "block_jacobi" / 3 (A_values, or None: the blocks of the operator)"""
        kind = self._PRECONDITIONER_IDS.get(kind, kind)
        self._follow_torch(A_values, r, z)
        check(_capi.lib().mimi_hip_linear_apply_preconditioner(self._h, int(kind), fptr(A_values), fptr(r), fptr(z)))
        return z

    def SetNodeBlock(self, dim):
        """the handle's n is n_nodes * dim in byVDIM order: what "block_jacobi" needs.  Refused when n % dim != 0."""
        check(_capi.lib().mimi_hip_linear_set_node_block(self._h, int(dim)))

    def SetOperatorDiagonal(self, on):
        """arms "jacobi" for solves without matrix values: 1 / diag then comes from the operator's domain
        (NonlinearSolid.TangentDiagonal), once per solve.  Off by default: "jacobi" with None values is refused."""
        check(_capi.lib().mimi_hip_linear_set_operator_diagonal(self._h, 1 if on else 0))

    def SetOperator(self, domain, density, stiffness, viscosity):
        """a domain integrator in place of the matrix: Mult(None, b, x) / MultCG(None, b, x) then solve with the product
        density M + stiffness K(u of domain.Linearize) + viscosity C, eliminated like the matrix.  Preconditioners "none",
        "kronecker" and "block_jacobi"; "jacobi" needs the matrix values unless SetOperatorDiagonal armed it.  Solves that pass
        values run as ever."""
        check(_capi.lib().mimi_hip_linear_set_operator(self._h, domain._handle(), float(density), float(stiffness), float(viscosity)))
        self._operator = domain          # (the library reads the handle during every solve)
        self._boundary_operators = []    # every SetOperator drops the boundary terms

    def AddBoundaryOperator(self, integrator, factor):
        """a MortarContact or FollowerPressure beside the domain of SetOperator: the product gains factor K_face(u of
        integrator.Linearize).  At most 8 terms, added in this order; SetOperator and ClearOperator drop them."""
        check(_capi.lib().mimi_hip_linear_add_boundary_operator(self._h, int(integrator._operator_kind), integrator._handle(),
                                                                float(factor)))
        self._boundary_operators.append(integrator)   # (the library reads the handle during every solve)

    def ClearOperator(self):
        check(_capi.lib().mimi_hip_linear_set_operator(self._h, None, 0.0, 0.0, 0.0))
        self._operator = None
        self._boundary_operators = []

    def SetOperatorFold(self, fold):
        """a mimi_amd.integrators.PeriodicFold between this solver (on the folded pattern) and the handles of SetOperator /
        AddBoundaryOperator (on the unwrapped one): the product becomes mask(P^T A_u P (mask x)) + x[ess].  Set it before the
        operator, whose size is checked against it; it survives SetOperator and ClearOperator; None clears it."""
        check(_capi.lib().mimi_hip_linear_set_operator_fold(self._h, fold._handle() if fold is not None else None))
        self._operator_fold = fold       # (the library reads its tables during every solve)

    def OperatorMult(self, x, y):
        """y = the eliminated product Mult(None, ...) / MultCG(None, ...) apply: mask(A (mask x)) + x[ess], folded or not"""
        self._follow_torch(x, y)
        check(_capi.lib().mimi_hip_linear_operator_mult(self._h, fptr(x), fptr(y)))
        return y

    def Mult(self, A_values, b, x):
        """x = A^-1 b to the configured tolerances (x is overwritten: iterative_mode false); A_values None: the operator of
        SetOperator"""
        it, conv, nrm = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        self._follow_torch(A_values, b, x)
        check(_capi.lib().mimi_hip_linear_gmres(self._h, fptr(A_values), fptr(b), fptr(x), self.rel_tol, self.abs_tol,
                                                int(self.max_iter), int(self.kdim), self._preconditioner_id(),
                                                C.byref(it), C.byref(nrm), C.byref(conv)))
        self.final_iter_, self.final_norm_, self.converged_ = it.value, nrm.value, bool(conv.value)
        return x

    def MultCG(self, A_values, b, x, rel_tol=1e-8, abs_tol=1e-12, max_iter=1000):
        """x = A^-1 b by preconditioned conjugate gradients: the mass solve of operators::NonlinearSolid
        (operators/nonlinear_solid.cpp:39-50,155)"""
        it, conv, nrm = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        self._follow_torch(A_values, b, x)
        check(_capi.lib().mimi_hip_linear_cg(self._h, fptr(A_values), fptr(b), fptr(x), rel_tol, abs_tol, int(max_iter),
                                             self._preconditioner_id(), C.byref(it), C.byref(nrm), C.byref(conv)))
        self.final_iter_, self.final_norm_, self.converged_ = it.value, nrm.value, bool(conv.value)
        return x
