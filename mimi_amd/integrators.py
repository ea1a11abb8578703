"""Host-side mirror of the reference's integrator interface
(src/mimi/integrators/nonlinear_base.hpp:14-154) on top of the C ABI of libmimi_hip.so.

Method names, argument meaning and accumulate-into semantics are the reference's:
  Prepare(); AddDomainResidual(u, r); AddDomainResidualAndGrad(u, grad_factor, r, A);
  DomainPostTimeAdvance(u); public members dt_, first_effective_dt_, second_effective_dt_
(snake_case aliases are provided as well).  `u`, `r`, `A` may be numpy arrays (host) or
torch tensors on the handle's device (used in place, call is asynchronous on the stream).
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import ABI, check, fptr, ptr

TANGENT_ANALYTIC = ABI.TANGENT_ANALYTIC
TANGENT_REFERENCE_FD = ABI.TANGENT_REFERENCE_FD


class CSRPattern:
    """(rowptr int64[n_vdofs+1], col int32[nnz]) of PrepareSparsity (utils/precomputed.cpp:151-174)."""

    def __init__(self, rowptr, col, nnz):
        self.rowptr, self.col, self.nnz = rowptr, col, int(nnz)

    @classmethod
    def of_bspline_patch(cls, patch, device=0, on_device=False, node_box=None):
        """Structured pattern of a lexicographically numbered patch, built on the GPU.

        node_box = (begin[dim], end[dim]): the row slice of a rank that owns that box of nodes -- rowptr keeps its full
        length, rows of other nodes are empty, col and the value array hold only the slice (mimi_hip.h:
        mimi_hip_bspline_sparsity_rows)."""
        L = _capi.lib()
        n = (C.c_int32 * 3)(*(patch.n_ctrl + [1] * (3 - patch.dim)))
        p = (C.c_int32 * 3)(*(patch.degrees + [0] * (3 - patch.dim)))
        nnz = C.c_int64(0)
        nrows = patch.n_vdofs
        if node_box is None:
            def build(rowptr, col):
                check(L.mimi_hip_bspline_sparsity(patch.dim, n, p, device, ptr(rowptr), ptr(col) if col is not None else None,
                                                  C.byref(nnz)))
        else:
            lo = (C.c_int32 * 3)(*(list(node_box[0]) + [0] * (3 - patch.dim)))
            hi = (C.c_int32 * 3)(*(list(node_box[1]) + [1] * (3 - patch.dim)))

            def build(rowptr, col):
                check(L.mimi_hip_bspline_sparsity_rows(patch.dim, n, p, lo, hi, device, ptr(rowptr),
                                                       ptr(col) if col is not None else None, C.byref(nnz)))
        if on_device:
            import torch
            dev = torch.device("cuda", device)
            rowptr = torch.empty(nrows + 1, dtype=torch.int64, device=dev)
            build(rowptr, None)
            col = torch.empty(nnz.value, dtype=torch.int32, device=dev)
            build(rowptr, col)
        else:
            rowptr = np.empty(nrows + 1, dtype=np.int64)
            build(rowptr, None)
            col = np.empty(nnz.value, dtype=np.int32)
            build(rowptr, col)
        return cls(rowptr, col, nnz.value)


class NonlinearBase(_capi.Handle):
    """integrators/nonlinear_base.hpp:14-154"""
    dt_ = 0.0
    first_effective_dt_ = 0.0
    second_effective_dt_ = 0.0

    def __init__(self, name):
        self.name_ = name

    def Name(self):
        return self.name_


class NonlinearSolid(NonlinearBase):
    """integrators::NonlinearSolid (integrators/nonlinear_solid.hpp:15-128) on one MI355X.

    Either `patch` (a splines.BSplinePatch: tables are generated on the device and the
    tensor-product kernels are used) or `tables` (dict with the reference's flattened
    PrecomputedData: dim, n_nodes, dofs[e,a], dN_dX[e,q,J,a], weight_det[e,q]) must be given.
    """
    _prefix = "domain"

    def __init__(self, name, material, pattern, patch=None, tables=None, device=0, quadrature_order=-1,
                 element_box=None, node_ids=None):
        super().__init__(name)
        self.material_ = material
        self.pattern_ = pattern
        self.patch_, self.tables_ = patch, tables
        self.device_ = device
        self.quadrature_order_ = quadrature_order
        self.element_box_ = element_box
        self.node_ids_ = node_ids
        self._keep = []

    # -- NonlinearSolid::Prepare (nonlinear_solid.cpp:31-46) --------------------------
    def Prepare(self):
        L = _capi.lib()
        mat = self.material_._c_struct()
        h = C.c_void_p()
        if self.patch_ is not None:
            p = self.patch_
            d = _capi.BSplinePatch()
            d.dim = p.dim
            for i in range(p.dim):
                d.degree[i] = p.degrees[i]
                d.n_knots[i] = len(p.knots[i])
                d.knots[i] = p.knots[i].ctypes.data
            d.control_points = p.control_points.ctypes.data
            if getattr(p, "weights", None) is not None:
                d.weights = p.weights.ctypes.data
            if self.node_ids_ is not None:
                ids = np.ascontiguousarray(self.node_ids_, dtype=np.int64)
                self._keep.append(ids)
                d.node_ids = ids.ctypes.data
            d.quadrature_order = self.quadrature_order_
            if self.element_box_ is not None:
                b, e = self.element_box_
                for i in range(3):
                    d.element_begin[i] = b[i]
                    d.element_end[i] = e[i]
            d.csr_rowptr = ptr(self.pattern_.rowptr, "int64").value
            d.csr_col = ptr(self.pattern_.col, "int32").value
            check(L.mimi_hip_domain_create_bspline(C.byref(d), C.byref(mat), self.device_, C.byref(h)))
        else:
            t = self.tables_
            d = _capi.DomainTables()
            dofs = np.ascontiguousarray(t["dofs"], dtype=np.int32)
            g = np.ascontiguousarray(t["dN_dX"], dtype=np.float64)
            wd = np.ascontiguousarray(t["weight_det"], dtype=np.float64)
            self._keep += [dofs, g, wd]
            d.dim = t["dim"]
            d.n_elements, d.n_dof = dofs.shape
            d.n_quad = wd.shape[1]
            d.n_nodes = t["n_nodes"]
            assert g.shape == (d.n_elements, d.n_quad, d.dim, d.n_dof)
            d.dofs, d.dN_dX, d.weight_det = dofs.ctypes.data, g.ctypes.data, wd.ctypes.data
            d.csr_rowptr = ptr(self.pattern_.rowptr, "int64").value
            d.csr_col = ptr(self.pattern_.col, "int32").value
            check(L.mimi_hip_domain_create(C.byref(d), C.byref(mat), self.device_, C.byref(h)))
        self._h = h
        if self.patch_ is None and self.tables_.get("N") is not None:
            self.SetShapeValues(self.tables_["N"])
        self.n_elements_ = self._info(ABI.DOMAIN_INFO_N_ELEMENTS)
        self.n_quad_ = self._info(ABI.DOMAIN_INFO_N_QUAD)
        self.n_dof_ = self._info(ABI.DOMAIN_INFO_N_DOF)
        self.nnz_ = self._info(ABI.DOMAIN_INFO_NNZ)
        self.n_vdofs_ = self._info(ABI.DOMAIN_INFO_N_VDOFS)
        self.path_ = self._info(ABI.DOMAIN_INFO_PATH)
        self.has_states_ = self.material_._kind == ABI.MAT_J2
        return self

    def _info(self, what):
        return int(_capi.lib().mimi_hip_domain_info(self._handle(), what))

    def _push_dt(self):
        # forms::Nonlinear pushes these public members before each call (forms/nonlinear.hpp:63-65)
        check(_capi.lib().mimi_hip_domain_set_dt(self._handle(), self.dt_, self.first_effective_dt_,
                                                 self.second_effective_dt_))

    def SetTangentMode(self, mode):
        check(_capi.lib().mimi_hip_domain_set_tangent_mode(self._handle(), mode))

    def Integrate(self, current_u):
        """phase 1 of a tangent assembly on its own (mimi_hip.h: mimi_hip_domain_integrate): the element pieces stay in the
        handle's scratch until Gather() adds them into r / A.  Two-phase tensor paths, device tensors."""
        self._push_dt()
        self._follow_torch(current_u)
        check(_capi.lib().mimi_hip_domain_integrate(self._handle(), fptr(current_u)))

    def Gather(self, grad_factor, residual, grad, node_begin, node_end):
        """phase 2 over the nodes [node_begin, node_end) (global node indices per direction): r and A += the rows of those
        nodes.  Every node the handle's elements touch is to be gathered exactly once per Integrate()."""
        self._follow_torch(residual, grad)
        lo = (C.c_int32 * 3)(*[int(v) for v in node_begin])
        hi = (C.c_int32 * 3)(*[int(v) for v in node_end])
        check(_capi.lib().mimi_hip_domain_gather(self._handle(), float(grad_factor), fptr(residual), fptr(grad), lo, hi))

    # -- nonlinear_solid.cpp:151-160 ---------------------------------------------------
    def AddDomainResidual(self, current_u, residual):
        self._push_dt()
        self._follow_torch(current_u, residual)
        check(_capi.lib().mimi_hip_domain_add_residual(self._handle(), fptr(current_u), fptr(residual)))

    # -- nonlinear_solid.cpp:162-177 ---------------------------------------------------
    def AddDomainResidualAndGrad(self, current_u, grad_factor, residual, grad_values):
        self._push_dt()
        self._follow_torch(current_u, residual, grad_values)
        check(_capi.lib().mimi_hip_domain_add_residual_and_grad(self._handle(), fptr(current_u), float(grad_factor),
                                                                fptr(residual), fptr(grad_values)))

    def AddDomainResidualAndGradFrom(self, current_u, grad_factor, residual, base_values, grad_values):
        """r += R(u); grad_values = base_values + grad_factor K(u) on the rows of the handle's nodes: the operator's
        "jacobian <- mass values, then AddMultGrad" (operators/nonlinear_solid.cpp:257-258) as ONE pass -- the row gathers
        read base_values where "+=" would read grad_values (mimi_hip.h: mimi_hip_domain_add_residual_and_grad_from)."""
        self._push_dt()
        self._follow_torch(current_u, residual, grad_values, base_values)
        check(_capi.lib().mimi_hip_domain_add_residual_and_grad_from(self._handle(), fptr(current_u), float(grad_factor),
                                                                     fptr(residual), fptr(base_values), fptr(grad_values)))

    # -- nonlinear_solid.cpp:179-199 ---------------------------------------------------
    def DomainPostTimeAdvance(self, converged_u):
        # the reference's material keeps the dt_ of the latest Add* call (nonlinear_solid.cpp:154,167)
        self._push_dt()
        self._follow_torch(converged_u)
        check(_capi.lib().mimi_hip_domain_post_time_advance(self._handle(), fptr(converged_u)))

    def AddDomainGrad(self, current_u, grad):
        raise RuntimeError("Currently not implemented, use AddDomainResidualAndGrad")  # nonlinear_solid.hpp:108-113

    # -- material state (MaterialState, materials.hpp:278-286) --------------------------
    # mimi_hip_kernel_family by value: "none", "tensor_p2_two_phase", "tensor_p3_two_phase", "tensor_small", "general"
    KERNEL_FAMILIES = {v: k[len("FAMILY_"):].lower() for k, v in vars(ABI).items() if k.startswith("FAMILY_")}

    def LastKernelFamily(self):
        """which kernel family the last assembly on this handle ran on (tests assert it; see mimi_hip_domain_info)"""
        return self.KERNEL_FAMILIES[self._info(ABI.DOMAIN_INFO_LAST_FAMILY)]

    # mimi_hip_general_route by value: "none", "gather", "atomics"
    GENERAL_ROUTES = {v: k[len("GENERAL_ROUTE_"):].lower() for k, v in vars(ABI).items() if k.startswith("GENERAL_ROUTE_")}

    def LastGeneralRoute(self):
        """how the element pieces of the last assembly on this handle reached r and A (MIMI_HIP_DOMAIN_INFO_GENERAL_ROUTE):
        "gather" = stored, then the general row gather (families "general" and "tensor_small"); "atomics" = the general
        kernels adding in place; "none" = no assembly yet, or a two-phase tensor family"""
        return self.GENERAL_ROUTES[self._info(ABI.DOMAIN_INFO_GENERAL_ROUTE)]

    def LastWalkGeometry(self):
        """(seg_len, cols_per_wg) of the last launch of the symmetric-half degree-2 kernel on this handle: elements per unit
        (column or column segment) and units a workgroup walks back to back; (0, 0) before any (MIMI_HIP_DOMAIN_INFO_SEGMENT_LENGTH
        and _UNITS_PER_WORKGROUP; tests assert the walk they were written to reach)"""
        return self._info(ABI.DOMAIN_INFO_SEGMENT_LENGTH), self._info(ABI.DOMAIN_INFO_UNITS_PER_WORKGROUP)

    def State(self, what):
        # "plastic_strain" = the material's first state matrix (J2 / J2Linear: plastic strain, J2Simo: be_old, J2Log:
        # Fp_inv); "state2" = its second one (J2Linear: beta, J2Simo: F_old)
        ids = {"accumulated_plastic_strain": ABI.STATE_EQPS, "temperature": ABI.STATE_TEMPERATURE,
               "plastic_strain": ABI.STATE_MATRIX_1, "state2": ABI.STATE_MATRIX_2}
        n = self.n_elements_ * self.n_quad_
        dim = self.patch_.dim if self.patch_ is not None else self.tables_["dim"]
        matrix = what in ("plastic_strain", "state2")
        shape = (self.n_elements_, self.n_quad_, dim * dim) if matrix else (self.n_elements_, self.n_quad_)
        out = np.empty(shape)
        check(_capi.lib().mimi_hip_domain_get_state(self._handle(), ids[what], ptr(out), out.size))
        return out

    # -- field output (mimi_hip.h: "field output") ---------------------------------------------------
    FIELDS = {"cauchy_stress": ABI.FIELD_CAUCHY, "von_mises_stress": ABI.FIELD_VON_MISES, "det_F": ABI.FIELD_DET_F,
              "accumulated_plastic_strain": ABI.FIELD_EQPS, "temperature": ABI.FIELD_TEMPERATURE}

    def _dim(self):
        return self.patch_.dim if self.patch_ is not None else self.tables_["dim"]

    def _field(self, name):
        if name not in self.FIELDS:
            raise ValueError(f"unknown field {name!r} (known: {', '.join(self.FIELDS)})")
        return self.FIELDS[name]

    def FieldComponents(self, name):
        """components of a field: dim^2 for "cauchy_stress" (column-major, [i + j dim]), 1 for the others"""
        return int(_capi.lib().mimi_hip_field_components(self._field(name), self._dim()))

    def SetShapeValues(self, N):
        """flat-table handles: the shape values N[e, q, a] (QuadData::N) the nodal projection needs; taken from
        tables["N"] at Prepare() when the dict has it"""
        N = np.ascontiguousarray(N, dtype=np.float64)
        if N.ndim != 3:
            raise ValueError(f"shape values must be [n_elements, n_quad, n_dof], got {N.shape}")
        want = (self._info(ABI.DOMAIN_INFO_N_ELEMENTS), self._info(ABI.DOMAIN_INFO_N_QUAD), self._info(ABI.DOMAIN_INFO_N_DOF))
        if N.shape != want:
            raise ValueError(f"shape values must be {want}, got {N.shape}")
        check(_capi.lib().mimi_hip_domain_set_shape_values(self._handle(), ptr(N)))

    def PointField(self, name, u, out=None):
        """the field at the quadrature points, [n_el, n_q, ncomp] (overwritten; allocated on the host when out is None).
        "cauchy_stress": sigma = P F^T / det F with the P AddDomainResidual would integrate at u (committed state, the
        pushed dt; no state changes); "von_mises_stress": sqrt(3/2) |sigma - tr(sigma)/dim I|, the trace taken over dim as
        in the reference's Dev -- the q of its J2 yield function, in 3-D the usual von Mises stress; "det_F";
        "accumulated_plastic_strain" and "temperature": the committed state (u may be None).  numpy arrays or torch
        device tensors."""
        field = self._field(name)
        ncomp = self.FieldComponents(name)
        if out is None:
            out = np.empty((self.n_elements_, self.n_quad_, ncomp))
        self._push_dt()
        self._follow_torch(u, out)
        size = out.size if isinstance(out, np.ndarray) else out.numel()
        check(_capi.lib().mimi_hip_domain_point_field(self._handle(), fptr(u), field, fptr(out), size))
        return out

    def NodalField(self, name, u, sum, weight=None):
        """the lumped L2 projection in accumulate form: sum[A, c] += sum_e sum_q w det N_A f_c, weight[A] += sum_e sum_q
        w det N_A over this handle's elements (A: the caller's node ids); the caller divides.  sum [n_nodes, ncomp],
        weight [n_nodes] or None."""
        field = self._field(name)
        self._push_dt()
        self._follow_torch(u, sum, weight)
        check(_capi.lib().mimi_hip_domain_nodal_field(self._handle(), fptr(u), field, fptr(sum), fptr(weight)))
        return sum

    # -- mass, damping and body-force forms (mimi_hip.h) -------------------------------------------
    def AddMass(self, density, values):
        """values[(A,i),(B,i)] += density * sum_e sum_q w det N_a N_b over this handle's elements (VectorMassIntegrator);
        the i != j entries of a node block are not touched.  numpy array or torch device tensor of nnz doubles."""
        self._follow_torch(values)
        check(_capi.lib().mimi_hip_domain_add_mass(self._handle(), float(density), fptr(values)))
        return values

    def AddDiffusion(self, viscosity, values):
        """values[(A,i),(B,i)] += viscosity * sum_e sum_q w det dN_a/dX . dN_b/dX (VectorDiffusionIntegrator)"""
        self._follow_torch(values)
        check(_capi.lib().mimi_hip_domain_add_diffusion(self._handle(), float(viscosity), fptr(values)))
        return values

    def AddBodyForce(self, b, r):
        """r[(A,i)] += b[i] * sum_e sum_q w det N_a (VectorDomainLFIntegrator); b: dim numbers"""
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).ravel())
        if b.size != self._dim():
            raise ValueError(f"body force must have {self._dim()} components, got {b.size}")
        self._follow_torch(r)
        check(_capi.lib().mimi_hip_domain_add_body_force(self._handle(), ptr(b), fptr(r)))
        return r

    # -- matrix-free tangent action (mimi_hip.h: "tangent action") ------------------------------------
    def Linearize(self, u):
        """the snapshot of the tangent at u (committed state, the pushed dt; no state changes) that ApplyTangent's stiffness
        term reads: a device copy of u on neo-Hookean handles, the record w det dP/dF per point on every other material.
        Stands in, with ApplyTangent, for AddMultGrad followed by SparseMatrix::Mult inside the reference's GMRES."""
        self._push_dt()
        self._follow_torch(u)
        check(_capi.lib().mimi_hip_domain_linearize(self._handle(), fptr(u)))

    def ApplyTangent(self, x, y, stiffness=1.0, density=0.0, viscosity=0.0):
        """y += density M x + stiffness K(u of Linearize) x + viscosity C x over this handle's elements, without a matrix; M and
        C the forms of AddMass / AddDiffusion with coefficient 1.  No essential dofs.  numpy arrays or torch device tensors."""
        self._follow_torch(x, y)
        check(_capi.lib().mimi_hip_domain_apply_tangent(self._handle(), float(density), float(stiffness), float(viscosity),
                                                        fptr(x), fptr(y)))
        return y

    def TangentDiagonal(self, out, stiffness=1.0, density=0.0, viscosity=0.0, block=False):
        """out += the diagonal of density M + stiffness K(u of Linearize) + viscosity C, the operator ApplyTangent applies,
        without a matrix (mimi_hip.h: "tangent diagonal").  block=False: n_nodes * dim values in byVDIM order; block=True: the
        node blocks [A][i][j], n_nodes * dim * dim values, whose entries i == j are the diagonal to the bit.  No essential dofs.
        What mfem::DSmoother reads off the assembled matrix.  numpy array or torch device tensor."""
        self._follow_torch(out)
        check(_capi.lib().mimi_hip_domain_tangent_diagonal(self._handle(), float(density), float(stiffness), float(viscosity),
                                                           1 if block else 0, fptr(out)))
        return out

    def LastActionFamily(self):
        """which kernel family the last ApplyTangent on this handle ran on (MIMI_HIP_DOMAIN_INFO_APPLY_FAMILY)"""
        return self.KERNEL_FAMILIES[self._info(ABI.DOMAIN_INFO_APPLY_FAMILY)]

    def LinearizationBytes(self):
        """bytes of linearisation record the handle holds (MIMI_HIP_DOMAIN_INFO_LINEARIZATION_BYTES): 0 on neo-Hookean handles"""
        return self._info(ABI.DOMAIN_INFO_LINEARIZATION_BYTES)

    def HoldsGradientTables(self):
        """whether the handle holds per-point gradient tables (MIMI_HIP_DOMAIN_INFO_HAS_GRADIENT_TABLES)"""
        return bool(self._info(ABI.DOMAIN_INFO_HAS_GRADIENT_TABLES))

    def SetPhaseTiming(self, on=True):
        check(_capi.lib().mimi_hip_domain_set_phase_timing(self._handle(), 1 if on else 0))

    def PhaseMs(self):
        """(phase 1, phase 2) milliseconds of the last two-phase tangent assembly (events on the launch stream)"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        check(_capi.lib().mimi_hip_domain_phase_ms(self._handle(), C.byref(a), C.byref(b)))
        return a.value, b.value

    def PhaseMsDetail(self):
        """(material pre-pass, integration / contraction kernel, row gather) milliseconds of the last two-phase tangent assembly"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(_capi.lib().mimi_hip_domain_phase_ms_detail(self._handle(), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def ResetState(self):
        check(_capi.lib().mimi_hip_domain_reset_state(self._handle()))

    # snake_case aliases
    prepare = Prepare
    add_domain_residual = AddDomainResidual
    add_domain_residual_and_grad = AddDomainResidualAndGrad
    domain_post_time_advance = DomainPostTimeAdvance


class _Frictional:
    """Coulomb friction of a rigid body (include/mimi_hip.h: mimi_hip_contact_set_friction; the reference has none):
    friction = mu (0: none), tangential_coefficient = the tangential penalty (None: the body's coefficient),
    step_displacement = the body's displacement over the current step (None: zero).  A change reaches the MortarContact
    integrators built on the body, as a change of NearestDistanceToSplines.coefficient does."""

    def _init_friction(self, friction=0.0, tangential_coefficient=None, step_displacement=None):
        self._friction_handles = weakref.WeakSet()      # MortarContact integrators built on this body
        self._friction, self._tangential = float(friction), tangential_coefficient
        self._step = None if step_displacement is None else [float(v) for v in np.ravel(step_displacement)]

    def _push_friction(self):
        for c in list(self.__dict__.get("_friction_handles", ())):
            c._apply_friction()

    @property
    def friction(self):
        return self.__dict__.get("_friction", 0.0)

    @friction.setter
    def friction(self, value):
        self._friction = float(value)
        self._push_friction()

    @property
    def tangential_coefficient(self):
        t = self.__dict__.get("_tangential")
        return self.coefficient if t is None else float(t)

    @tangential_coefficient.setter
    def tangential_coefficient(self, value):
        self._tangential = value
        self._push_friction()

    @property
    def step_displacement(self):
        return self.__dict__.get("_step")

    @step_displacement.setter
    def step_displacement(self, value):
        self._step = None if value is None else [float(v) for v in np.ravel(value)]
        self._push_friction()


class RigidSphere(_Frictional):
    """Analytic rigid body standing in for NearestDistanceToSplines
    (coefficients/nearest_distance.hpp:215-288; splinepy's proximity query is not available)."""
    kind = ABI.BODY_SPHERE

    def __init__(self, center, radius, coefficient=1.0e4, friction=0.0, tangential_coefficient=None, step_displacement=None):
        self.center, self.radius = [float(c) for c in center], float(radius)
        self.coefficient = float(coefficient)   # NearestDistanceBase::coefficient_ (nearest_distance.hpp:18)
        self._init_friction(friction, tangential_coefficient, step_displacement)

    def params(self, dim):
        return self.center + [0.0] * (3 - dim) + [self.radius]


class RigidPlane(_Frictional):
    kind = ABI.BODY_PLANE

    def __init__(self, point, normal, coefficient=1.0e4, friction=0.0, tangential_coefficient=None, step_displacement=None):
        n = np.asarray(normal, dtype=np.float64)
        self.point, self.normal = [float(c) for c in point], list(n / np.linalg.norm(n))
        self.coefficient = float(coefficient)
        self._init_friction(friction, tangential_coefficient, step_displacement)

    def params(self, dim):
        return self.point + [0.0] * (3 - dim) + self.normal + [0.0] * (3 - dim)


class RigidSpline(_Frictional):
    """One rigid boundary spline (curve in 2-D, surface in 3-D): what NearestDistanceToSplines holds
    (coefficients/nearest_distance.hpp:215-288).  Orientation: the normal (t_y, -t_x) / S_u x S_v must point out of the
    rigid body (nearest_distance.hpp:139-184)."""
    kind = ABI.BODY_SPLINE

    def __init__(self, degrees, knots, control_points, weights=None, resolution=100, coefficient=1.0e4, max_iterations=-1,
                 friction=0.0, tangential_coefficient=None, step_displacement=None):
        self.degrees = [int(p) for p in degrees]
        self.knots = [np.ascontiguousarray(k, dtype=np.float64) for k in knots]
        n = int(np.prod([len(k) - p - 1 for k, p in zip(self.knots, self.degrees)]))
        self.control_points = np.ascontiguousarray(control_points, dtype=np.float64).reshape(n, -1)
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(n)
        self.resolution, self.max_iterations = int(resolution), int(max_iterations)
        self.coefficient = float(coefficient)
        self._init_friction(friction, tangential_coefficient, step_displacement)

    def params(self, dim):
        return []

    def c_struct(self):
        s = _capi.SplineBody()
        s.para_dim = len(self.degrees)
        for k in range(s.para_dim):
            s.degree[k], s.n_knots[k] = self.degrees[k], len(self.knots[k])
            s.knots[k] = self.knots[k].ctypes.data
        s.control_points = self.control_points.ctypes.data
        s.weights = self.weights.ctypes.data if self.weights is not None else None
        s.kdtree_resolution, s.max_iterations = self.resolution, self.max_iterations
        return s


class NearestDistanceToSplines(_Frictional):
    """coefficients::NearestDistanceToSplines as bound in py/py_nearest_distance.cpp: add_spline / plant_kd_tree /
    coefficient.  `spline` is anything with the attributes degrees, knot_vectors, control_points and (optionally)
    weights -- a splinepy spline has them."""
    kind = ABI.BODY_SPLINE

    def __init__(self):
        self._coefficient = 1.0e4       # nearest_distance.hpp:18
        self.tolerance = 1.0e-24        # nearest_distance.hpp:20 (the search here stops on the step size)
        self._splines, self._resolution = [], 100
        self._attached = []             # MortarContact integrators built on this scene
        self._init_friction()

    @property
    def coefficient(self):
        return self._coefficient

    @coefficient.setter
    def coefficient(self, value):
        """the reference reads coefficient_ at every evaluation: a change after setup reaches the device handles"""
        self._coefficient = float(value)
        for c in getattr(self, "_attached", []):
            c.UpdateBody(penalty=self._coefficient)
        self._push_friction()           # (the tangential penalty defaults to the coefficient)

    def add_spline(self, spline):
        self._splines.append(spline)
        return self

    def clear(self):
        self._splines.clear()

    def plant_kd_tree(self, resolution, nthreads=1):
        """PlantKdTree (nearest_distance.hpp:243-255).  examples/nl_contact.py moves the spline's control points and
        calls this before every step: the attached device handles get the moved body."""
        self._resolution = int(resolution)
        for c in self._attached:
            c.UpdateBody(spline=True)

    def size(self):
        return len(self._splines)

    def _body(self):
        if len(self._splines) != 1:
            raise RuntimeError("exactly one boundary spline is supported (nearest_distance.hpp:262-263)")
        sp = self._splines[0]
        w = getattr(sp, "weights", None)
        return RigidSpline(sp.degrees, sp.knot_vectors, sp.control_points, None if w is None else np.ravel(w),
                           resolution=self._resolution, coefficient=self.coefficient)

    def params(self, dim):
        return []

    def c_struct(self):
        self._rs = self._body()
        return self._rs.c_struct()


class _FaceTangentAction:
    """The matrix-free action of a face tangent (include/mimi_hip.h: mimi_hip_contact_linearize / mimi_hip_pressure_linearize
    and their apply_tangent), the boundary twin of NonlinearSolid.Linearize / ApplyTangent.  `_operator_kind` is the kind of
    mimi_hip_linear_add_boundary_operator, `_action_prefix` names the C entries (mimi_hip_<_action_prefix>_linearize ...)."""

    def _action_fn(self, name):
        return getattr(_capi.lib(), f"mimi_hip_{self._action_prefix}_{name}")

    def Linearize(self, u):
        """the snapshot of the face tangent at u (the handle's current body and penalty, or pressure) that ApplyTangent reads:
        per face point a coefficient and the surface tangents, per face the active flag.  It survives every later call on
        the handle.  Stands in, with ApplyTangent, for AddBoundaryResidualAndGrad followed by SparseMatrix::Mult."""
        self._follow_torch(u)
        check(self._action_fn("linearize")(self._handle(), fptr(u)))

    def ApplyTangent(self, x, y, factor=1.0):
        """y += factor K_face(u of Linearize) x, without a matrix.  numpy arrays or torch device tensors."""
        self._follow_torch(x, y)
        check(self._action_fn("apply_tangent")(self._handle(), float(factor), fptr(x), fptr(y)))
        return y

    def LinearizationBytes(self):
        """bytes of linearisation record the handle holds (0 before the first Linearize)"""
        return int(self._action_fn("action_info")(self._handle(), ABI.ACTION_INFO_BYTES))

    def HoldsTangentBlocks(self):
        """whether the per-face tangent blocks of an assembly are allocated"""
        return bool(self._action_fn("action_info")(self._handle(), ABI.ACTION_INFO_FACE_BLOCKS))


class MortarContact(_FaceTangentAction, NonlinearBase):
    """integrators::MortarContact (integrators/mortar_contact.hpp:23-172) against an analytic
    rigid body, on one face of a B-spline patch."""
    _prefix = "contact"
    _action_prefix, _operator_kind = "contact", ABI.BOUNDARY_CONTACT

    def __init__(self, nearest_distance_coeff, name, pattern, patch, axis, side, device=0, quadrature_order=-1,
                 element_box=None):
        super().__init__(name)
        self.element_box_ = element_box          # multi-GPU: only the faces of the elements of this slab
        self.nearest_distance_coeff_ = nearest_distance_coeff
        self.pattern_, self.patch_ = pattern, patch
        self.axis_, self.side_ = axis, side
        self.device_, self.quadrature_order_ = device, quadrature_order
        self.last_area_ = 0.0
        self.last_pressure_ = 0.0
        self.last_force_ = np.zeros(patch.dim)
        self.friction_, self._has_increment = 0.0, False
        self.consistent_tangent_ = False
        self.friction_action_ = False
        self.augmented_ = False
        self.last_friction_force_ = np.zeros(patch.dim)
        self.last_friction_traction_ = 0.0
        self.n_stick_ = self.n_slip_ = 0

    def Prepare(self):
        L = _capi.lib()
        p = self.patch_
        t = _capi.ContactTables()
        self._keep = _capi.fill_face_tables(t, p, self.axis_, self.side_, self.quadrature_order_, self.element_box_,
                                            "no marked boundary faces in this element box")
        body = self.nearest_distance_coeff_
        t.body_kind = body.kind
        for i, v in enumerate(body.params(p.dim)):
            t.body[i] = v
        t.penalty = body.coefficient
        if body.kind == ABI.BODY_SPLINE:
            self._spline_struct = body.c_struct()
            self._keep.append(body)
            t.spline = C.cast(C.pointer(self._spline_struct), C.c_void_p)
            if hasattr(body, "_attached"):
                body._attached.append(self)
        t.csr_rowptr = ptr(self.pattern_.rowptr, "int64").value
        t.csr_col = ptr(self.pattern_.col, "int32").value
        h = C.c_void_p()
        check(L.mimi_hip_contact_create(C.byref(t), self.device_, C.byref(h)))
        self._h = h
        self.n_marked_boundaries_ = int(t.n_faces)
        self.n_q_ = int(t.n_quad)
        if hasattr(body, "_friction_handles"):
            body._friction_handles.add(self)
        self._apply_friction()
        return self

    # -- Coulomb friction (include/mimi_hip.h: mimi_hip_contact_set_friction ...) ------------------------------------
    def _apply_friction(self):
        """the body's friction, tangential_coefficient and step_displacement onto the handle; a body that never had
        friction makes no call at all"""
        if getattr(self, "_h", None) is None:
            return
        body = self.nearest_distance_coeff_
        mu = float(getattr(body, "friction", 0.0))
        if mu > 0.0 and getattr(self, "sharded_", False):
            raise RuntimeError(f"friction (mu = {mu:g}) on the body of a ShardedContact is not supported")
        if mu > 0.0 or self.friction_ > 0.0:
            self.SetFriction(mu, float(getattr(body, "tangential_coefficient", body.coefficient)))
        d = getattr(body, "step_displacement", None)
        if d is not None or self._has_increment:
            self.SetBodyIncrement(d)

    def SetFriction(self, mu, tangential_coefficient=None):
        """mu >= 0 and the tangential penalty (None: the body's coefficient); mu = 0 switches friction off"""
        eps_t = self.nearest_distance_coeff_.coefficient if tangential_coefficient is None else tangential_coefficient
        check(_capi.lib().mimi_hip_contact_set_friction(self._handle(), float(mu), float(eps_t)))
        self.friction_ = float(mu)

    def SetBodyIncrement(self, d=None):
        """the rigid body's displacement over the current step (dim numbers; None: zero)"""
        dim = self.patch_.dim
        v = np.zeros(dim) if d is None else np.ascontiguousarray(np.asarray(d, dtype=np.float64).ravel())
        if v.size != dim:
            raise ValueError(f"step displacement must have {dim} components, got {v.size}")
        check(_capi.lib().mimi_hip_contact_set_body_increment(self._handle(), ptr(v)))
        self._has_increment = d is not None

    def ResetFriction(self):
        """elastic slip zero, no point in contact, no trial state"""
        check(_capi.lib().mimi_hip_contact_reset_friction(self._handle()))

    def CommitFriction(self):
        """commit the trial state of the latest evaluation, on the device: nothing is recomputed, nothing waits"""
        check(_capi.lib().mimi_hip_contact_post_time_advance(self._handle(), None))

    def FrictionState(self):
        """the committed state: (xi [n_faces, n_q, dim], xbar [n_faces, n_q, dim], c [n_faces, n_q] uint8)"""
        shape = (self.n_marked_boundaries_, self.n_q_, self.patch_.dim)
        xi, xbar, c = np.zeros(shape), np.zeros(shape), np.zeros(shape[:2], dtype=np.uint8)
        check(_capi.lib().mimi_hip_contact_friction_state(self._handle(), ptr(xi), ptr(xbar), c.ctypes.data_as(C.c_void_p)))
        return xi, xbar, c

    def _refuse_friction(self, what, lifted=False):
        """(lifted: what SetFrictionAction(True) makes available)"""
        if self.friction_ > 0.0 and not lifted:
            raise RuntimeError(f"{what} is not available on a contact with friction (mu = {self.friction_:g}): the friction "
                               "tangent is assembled only")

    def SetFrictionAction(self, on=True):
        """Friction on the matrix-free route (include/mimi_hip.h: mimi_hip_contact_set_friction_action): with it Linearize,
        ApplyTangent, a Krylov operator built on the handle and SetConsistentTangent accept a contact with friction.  A
        Linearize with mu > 0 then records, per face point, a = xi + x_q - xbar - d, the traction's coefficient and the
        branch, from the COMMITTED friction state -- a snapshot like the rest of the record, which no later SetFriction,
        SetBodyIncrement, CommitFriction, ResetFriction, UpdateBody or evaluation touches; it writes no trial state.
        ApplyTangent adds the assembled friction tangent's action and, on a consistent record, the derivative of the slip
        limit mu p_N by the nodal pressure.  Off (the default): every refusal stands.  The reference-FD tangent mode stays
        refused, and so do the handles of a ShardedContact."""
        if on and getattr(self, "sharded_", False):
            raise RuntimeError("the friction action on a ShardedContact is not supported: friction itself is refused there")
        check(_capi.lib().mimi_hip_contact_set_friction_action(self._handle(), 1 if on else 0))
        self.friction_action_ = bool(on)

    def HoldsFrictionRecord(self):
        """whether the record of the last Linearize carries friction"""
        return bool(self._action_fn("action_info")(self._handle(), ABI.ACTION_INFO_FRICTION))

    def Linearize(self, u):
        self._refuse_friction("the matrix-free tangent action (Linearize)", self.friction_action_)
        return super().Linearize(u)

    def ApplyTangent(self, x, y, factor=1.0):
        self._refuse_friction("the matrix-free tangent action (ApplyTangent)", self.friction_action_)
        return super().ApplyTangent(x, y, factor)

    def SetConsistentTangent(self, on=True):
        """The next Linearize records the consistent tangent (include/mimi_hip.h: mimi_hip_contact_set_consistent_tangent):
        ApplyTangent then adds the derivative of the nodal pressure p_i = eps G_i / A_i to the frozen-pressure action.  The
        term reaches past the CSR pattern, so it exists as an action only; AddBoundaryResidualAndGrad is unchanged.  An
        existing record is not touched.  On a handle built from an element box the nodal sums are those of its own faces,
        so the handles of a ShardedContact are refused."""
        if on and getattr(self, "sharded_", False):
            raise RuntimeError("the consistent tangent on a ShardedContact is not supported: the nodal sums of a handle run "
                               "over its own faces")
        if on:
            self._refuse_friction("the consistent tangent", self.friction_action_)
        check(_capi.lib().mimi_hip_contact_set_consistent_tangent(self._handle(), 1 if on else 0))
        self.consistent_tangent_ = bool(on)

    def HoldsConsistentRecord(self):
        """whether the record of the last Linearize is a consistent one"""
        return bool(self._action_fn("action_info")(self._handle(), ABI.ACTION_INFO_CONSISTENT))

    # -- augmented-Lagrangian mode (include/mimi_hip.h: mimi_hip_contact_set_augmented ...) ---------------------------
    def SetAugmented(self, on=True):
        """The augmented-Lagrangian law: a multiplier lambda_i <= 0 per marked node, the point gap unclamped in the nodal
        sum, p_i = min(0, lambda_i + eps G_i / A_i).  Switching from off to on zeroes the multipliers.  Off (the default):
        the penalty law on its launches and bytes.  It earns its place at a penalty of the order of the body's stiffness
        (the Uzawa loop contracts like k / (k + eps): DESIGN.md).  Refused on the handles of a ShardedContact (the nodal
        sums of a handle run over its own faces) and in the reference-FD tangent mode."""
        if on and getattr(self, "sharded_", False):
            raise RuntimeError("the augmented mode on a ShardedContact is not supported: the multipliers of a handle belong "
                               "to its own faces' nodal sums")
        check(_capi.lib().mimi_hip_contact_set_augmented(self._handle(), 1 if on else 0))
        self.augmented_ = bool(on)

    def Lagrange(self):
        """the multipliers at MarkedNodes(), a host array"""
        out = np.zeros(self.MarkedNodes().size)
        check(_capi.lib().mimi_hip_contact_lagrange(self._handle(), 0, ptr(out)))
        return out

    def SetLagrange(self, values):
        """multipliers at MarkedNodes() (host array or device tensor); projected onto lambda <= 0 on the device"""
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):
            values = np.ascontiguousarray(values, dtype=np.float64)
        else:
            self._follow_torch(values)
        n = self.MarkedNodes().size
        if values.ndim != 1 or values.shape[0] != n:
            raise ValueError(f"expected {n} multipliers (one per marked node), got shape {tuple(values.shape)}")
        check(_capi.lib().mimi_hip_contact_lagrange(self._handle(), 1, fptr(values)))

    def FillLagrange(self, value=0.0):
        self.SetLagrange(np.full(self.MarkedNodes().size, float(value)))

    def UpdateLagrange(self, u, apply=True):
        """The Uzawa step at u: dlambda_i = p_i - lambda_i, and with `apply` lambda_i <- p_i.  Returns a dict:
        violation = max |dlambda_i| / eps (a length), norm = sqrt(sum A_i dlambda_i^2), n_active = nodes with p_i < 0,
        max_lagrange = max |lambda_i| after the call.  The history of the last Add* call is left alone."""
        self._follow_torch(u)
        out = np.zeros(4)
        check(_capi.lib().mimi_hip_contact_update_lagrange(self._handle(), fptr(u), 1 if apply else 0, ptr(out)))
        return {"violation": float(out[0]), "norm": float(out[1]), "n_active": int(out[2]), "max_lagrange": float(out[3])}

    def HoldsAugmentedRecord(self):
        """whether the record of the last Linearize was made in the augmented mode"""
        return bool(self._action_fn("action_info")(self._handle(), ABI.ACTION_INFO_AUGMENTED))

    def UpdateBody(self, spline=False, penalty=-1.0):
        """the rigid body moved (spline=True: re-read it from nearest_distance_coeff_) and / or the penalty changed"""
        sp = None
        if spline:
            self._spline_struct = self.nearest_distance_coeff_.c_struct()
            sp = C.cast(C.pointer(self._spline_struct), C.c_void_p)
        check(_capi.lib().mimi_hip_contact_update_body(self._handle(), sp, float(penalty)))

    # -- the two halves of an evaluation, for element slabs on several GPUs (mimi_amd/parallel.py ShardedContact) -----
    def GapArea(self, current_u):
        """pass 1 only: nodal area / gap of this handle's faces"""
        self._follow_torch(current_u)
        check(_capi.lib().mimi_hip_contact_gap_area(self._handle(), fptr(current_u)))

    def MarkedNodes(self):
        return self._sized_query("marked_nodes", np.int32)

    def GetNodal(self, area, gap):
        self._follow_torch(area, gap)
        check(_capi.lib().mimi_hip_contact_nodal(self._handle(), 0, fptr(area), fptr(gap)))

    def SetNodal(self, area, gap):
        self._follow_torch(area, gap)
        check(_capi.lib().mimi_hip_contact_nodal(self._handle(), 1, fptr(area), fptr(gap)))

    def AddBoundaryResidualFromNodal(self, current_u, grad_factor, residual, grad=None):
        """pressure from the (summed) nodal area / gap, then pass 2"""
        self._follow_torch(current_u, residual, grad)
        check(_capi.lib().mimi_hip_contact_add_residual_from_nodal(self._handle(), fptr(current_u), float(grad_factor),
                                                                   fptr(residual), fptr(grad)))

    def SetTangentMode(self, mode):
        if mode == TANGENT_REFERENCE_FD:
            self._refuse_friction("the reference-FD tangent mode")
        check(_capi.lib().mimi_hip_contact_set_tangent_mode(self._handle(), mode))

    def _history(self):
        out = np.zeros(5)
        check(_capi.lib().mimi_hip_contact_last_history(self._handle(), ptr(out)))
        self.last_area_, self.last_pressure_ = out[0], out[1]
        self.last_force_ = out[2:2 + self.patch_.dim].copy()
        if self.friction_ > 0.0:
            out = np.zeros(6)
            check(_capi.lib().mimi_hip_contact_friction_history(self._handle(), ptr(out)))
            self.last_friction_force_ = out[:self.patch_.dim].copy()
            self.last_friction_traction_ = float(out[3])
            self.n_stick_, self.n_slip_ = int(out[4]), int(out[5])

    # mortar_contact.cpp:297-351
    def AddBoundaryResidual(self, current_u, residual):
        self._follow_torch(current_u, residual)
        check(_capi.lib().mimi_hip_contact_add_residual(self._handle(), fptr(current_u), fptr(residual)))

    # mortar_contact.cpp:353-421
    def AddBoundaryResidualAndGrad(self, current_u, grad_factor, residual, grad_values):
        self._follow_torch(current_u, residual, grad_values)
        check(_capi.lib().mimi_hip_contact_add_residual_and_grad(self._handle(), fptr(current_u), float(grad_factor),
                                                                 fptr(residual), fptr(grad_values)))

    # mortar_contact.cpp:423-467
    def GapNorm(self, test_u, nthreads=-1):
        out = C.c_double(0.0)
        check(_capi.lib().mimi_hip_contact_gap_norm(self._handle(), ptr(test_u), C.byref(out)))
        return out.value

    # mortar_contact.cpp:469-488: record last_area_, last_force_, last_pressure_.  With friction: first the evaluation at
    # converged_u and the commit of its state (the history is then that of converged_u)
    def BoundaryPostTimeAdvance(self, converged_u):
        if self.friction_ > 0.0:
            self._follow_torch(converged_u)
            check(_capi.lib().mimi_hip_contact_post_time_advance(self._handle(), fptr(converged_u)))
        self._history()

    def AveragePressure(self):
        return self._sized_query("get_pressure", np.float64)

    def AddBoundaryGrad(self, current_u, grad):
        raise RuntimeError("Currently not implemented, use AddDomainResidualAndGrad")  # mortar_contact.hpp:142-149


class FollowerPressure(_FaceTangentAction, NonlinearBase):
    """Follower pressure t = -p n da on the CURRENT surface of one face of a B-spline patch (include/mimi_hip.h:
    mimi_hip_pressure_*).  The reference's BCMarker::Pressure (utils/boundary_conditions.cpp:43-50) stores the value and
    never applies it; the boundary-integrator surface is MortarContact's (integrators/mortar_contact.hpp:23-172).

    Residual r(a,i) += sum_q w p_q N_a m_i (m: the non-normalised outward normal of the deformed face), tangent with
    dm/dx -- exact, not symmetric.  element_box = (begin, end): only the faces of the elements in that box (element slabs:
    every contribution lands in rows of the slab's own elements, no exchange of nodal values is needed)."""
    _prefix = "pressure"
    _action_prefix, _operator_kind = "follower", ABI.BOUNDARY_PRESSURE

    def __init__(self, name, pattern, patch, axis, side, device=0, quadrature_order=-1, element_box=None):
        super().__init__(name)
        self.pattern_, self.patch_ = pattern, patch
        self.axis_, self.side_ = axis, side
        self.device_, self.quadrature_order_ = device, quadrature_order
        self.element_box_ = element_box
        self.last_area_ = 0.0
        self.last_force_ = np.zeros(patch.dim)

    def Prepare(self):
        L = _capi.lib()
        t = _capi.PressureTables()
        self._keep = _capi.fill_face_tables(t, self.patch_, self.axis_, self.side_, self.quadrature_order_, self.element_box_,
                                            "no loaded boundary faces in this element box")
        t.csr_rowptr = ptr(self.pattern_.rowptr, "int64").value
        t.csr_col = ptr(self.pattern_.col, "int32").value
        h = C.c_void_p()
        check(L.mimi_hip_pressure_create(C.byref(t), self.device_, C.byref(h)))
        self._h = h
        self.n_faces_ = int(t.n_faces)
        return self

    def FaceNodes(self):
        """sorted global node ids of the loaded faces: the order of a nodal pressure array"""
        return self._sized_query("face_nodes", np.int32)

    def SetPressure(self, value):
        """a float (uniform pressure) or an array of values at FaceNodes() (host array or device tensor); applies from the
        next assembly on"""
        if np.isscalar(value):
            check(_capi.lib().mimi_hip_pressure_set_value(self._handle(), float(value)))
            return
        if isinstance(value, np.ndarray) or not hasattr(value, "data_ptr"):
            value = np.ascontiguousarray(value, dtype=np.float64)
        else:
            self._follow_torch(value)
        n = value.shape[0] if value.ndim == 1 else -1
        check(_capi.lib().mimi_hip_pressure_set_nodal(self._handle(), fptr(value), n))

    def AddBoundaryResidual(self, current_u, residual):
        self._follow_torch(current_u, residual)
        check(_capi.lib().mimi_hip_pressure_add_residual(self._handle(), fptr(current_u), fptr(residual)))

    def AddBoundaryResidualAndGrad(self, current_u, grad_factor, residual, grad_values):
        self._follow_torch(current_u, residual, grad_values)
        check(_capi.lib().mimi_hip_pressure_add_residual_and_grad(self._handle(), fptr(current_u), float(grad_factor),
                                                                  fptr(residual), fptr(grad_values)))

    def _history(self):
        out = np.zeros(4)
        check(_capi.lib().mimi_hip_pressure_last_history(self._handle(), ptr(out)))
        self.last_area_ = float(out[0])
        self.last_force_ = out[1:1 + self.patch_.dim].copy()

    # as MortarContact::BoundaryPostTimeAdvance (mortar_contact.cpp:469-488): area and force of the latest Add* call
    def BoundaryPostTimeAdvance(self, converged_u):
        self._history()

    def AddBoundaryGrad(self, current_u, grad):
        raise RuntimeError("Currently not implemented, use AddBoundaryResidualAndGrad")


class CouplingSurface(_capi.Handle):
    """The coupling surface of one face of a B-spline patch (include/mimi_hip.h: mimi_hip_surface_*): what a fluid partner
    exchanges with the solid every iteration of the reference's fixed-point loop (fixed_point_solve2 / fixed_point_advance2
    / advance_time2, py/py_solid.cpp:443-511), on the face tables, rule and outward normal of FollowerPressure
    (splines.face_tables).  Points are face-major, point-minor: n_points_ = n_faces_ * n_q_.

      points(u=None)          -> device tensors x [n_points, dim], unit outward normal [n_points, dim], area weight
                                 w_q |m_q| [n_points] of the configuration X + u
      set_traction(t, u=None) -> load_ = f(a,i) = sum_q w_q |m_q(X+u)| N_a t(q,i): the consistent nodal forces of t
                                 [n_points, dim], a traction per unit area of X + u (Cauchy for the current or advanced
                                 configuration, nominal for u = None); None removes the load

    u and load_ are in the solver's numbering: with `fold` (a PeriodicFold) u is expanded by fold.Expand and the load folded
    by fold.Add.  The load is dead within a solve and has no tangent: the coupling iteration carries its dependence on the
    geometry (the follower load with an exact tangent is FollowerPressure's).  Points / AddLoad are the C ABI as it stands
    (u in the patch's numbering, host arrays or device tensors, AddLoad adds into f)."""
    _prefix = "surface"

    def __init__(self, patch, axis, side, device=0, quadrature_order=-1, fold=None):
        self.patch_, self.axis_, self.side_ = patch, axis, side
        self.device_, self.quadrature_order_, self.fold_ = device, quadrature_order, fold
        self.load_ = None

    def Prepare(self):
        L = _capi.lib()
        t = _capi.PressureTables()
        keep = _capi.fill_face_tables(t, self.patch_, self.axis_, self.side_, self.quadrature_order_)   # (copied at create)
        h = C.c_void_p()
        check(L.mimi_hip_surface_create(C.byref(t), self.device_, C.byref(h)))
        self._h = h
        self.n_faces_, self.n_q_ = int(t.n_faces), int(t.n_quad)
        self.n_points_ = int(L.mimi_hip_surface_n_points(h))
        return self

    def Points(self, u, x, normal, weight):
        self._follow_torch(u, x, normal, weight)
        check(_capi.lib().mimi_hip_surface_points(self._handle(), fptr(u), fptr(x), fptr(normal), fptr(weight)))

    def AddLoad(self, u, t, f):
        self._follow_torch(u, t, f)
        check(_capi.lib().mimi_hip_surface_add_load(self._handle(), fptr(u), fptr(t), fptr(f)))

    def _on_device(self, a):
        import torch
        if not hasattr(a, "data_ptr"):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        return a.to(device=torch.device("cuda", self.device_), dtype=torch.float64).contiguous()

    def _unwrapped(self, u):
        """u in the solver's numbering -> the device vector of the patch's nodes the kernels read (None stays None)"""
        if u is None:
            return None
        import torch
        u = self._on_device(u).reshape(-1)
        n = self.fold_.n_f_ if self.fold_ is not None else self.patch_.n_vdofs
        if u.numel() != n:
            raise ValueError(f"displacement of {u.numel()} entries, the solver has {n}")
        if self.fold_ is None:
            return u
        return self.fold_.Expand(u, torch.empty(self.fold_.n_u_, dtype=torch.float64, device=u.device))

    def points(self, u=None):
        """device tensors (x [n_points, dim], unit outward normal [n_points, dim], area weight w_q |m_q| [n_points]) of
        the configuration X + u (u = None: the reference configuration)"""
        import torch
        uu = self._unwrapped(u)
        dev = torch.device("cuda", self.device_)
        x = torch.empty((self.n_points_, self.patch_.dim), dtype=torch.float64, device=dev)
        n = torch.empty_like(x)
        w = torch.empty(self.n_points_, dtype=torch.float64, device=dev)
        self.Points(uu, x, n, w)
        return x, n, w

    def set_traction(self, t, u=None):
        """load_ = the consistent nodal forces f(a,i) = sum_q w_q |m_q(X+u)| N_a t(q,i) of t [n_points, dim] (or flat),
        a traction per unit area of X + u: Cauchy traction for the current or advanced displacement, nominal traction for
        u = None.  t = None removes the load.  The load is dead within a solve and has no tangent: the coupling iteration
        carries its dependence on the geometry (a follower load with an exact tangent is FollowerPressure's)."""
        if t is None:
            self.load_ = None
            return
        import torch
        t = self._on_device(t)
        shape = (self.n_points_, self.patch_.dim)
        if tuple(t.shape) not in (shape, (shape[0] * shape[1],)):
            raise ValueError(f"traction of shape {tuple(t.shape)}: expected {shape} (points by components) or that many "
                             "values flat")
        uu = self._unwrapped(u)
        f = torch.zeros(self.patch_.n_vdofs, dtype=torch.float64, device=t.device)
        self.AddLoad(uu, t, f)
        if self.fold_ is not None:
            f_f = torch.zeros(self.fold_.n_f_, dtype=torch.float64, device=t.device)
            self.fold_.Add(f, f_f)
            f = f_f
        self.load_ = f


def periodic_node_map(n_ctrl, axes):
    """Node map of a lexicographically numbered patch (n_ctrl nodes per direction, direction 0 fastest) made periodic along
    `axes`: the last node plane along a periodic axis is the first one.  Folded nodes are numbered lexicographically on the
    grid without those last planes, so a merged node has the index of its lowest copy (what the reference's DofMap returns
    for a space whose boundaries were joined by NURBSExtension::ConnectBoundaries, py/py_nonlinear_solid.cpp:34-62).
    Returns node_map[n_nodes] (int64)."""
    dim = len(n_ctrl)
    axes = sorted(set(int(a) for a in axes))
    if any(a < 0 or a >= dim for a in axes):
        raise RuntimeError(f"periodic axes {axes} out of range for a {dim}-D patch")
    idx = np.indices(tuple(reversed([int(n) for n in n_ctrl])))[::-1]         # idx[d][z, y, x] = coordinate along d
    out = np.zeros(idx[0].shape, dtype=np.int64)
    stride = 1
    for d in range(dim):
        n_d = int(n_ctrl[d])
        if d in axes:
            if n_d < 2:
                raise RuntimeError(f"a periodic direction needs at least two nodes (direction {d} has {n_d})")
            out += (idx[d] % (n_d - 1)) * stride
            stride *= n_d - 1
        else:
            out += idx[d] * stride
            stride *= n_d
    return out.reshape(-1)


class PeriodicFold(_capi.Handle):
    """The periodic fold of include/mimi_hip.h (mimi_hip_fold_*) on one device: P is the 0/1 map from the folded dofs to
    the unwrapped dofs of `pattern` (an integrator's structured pattern), given per node by node_map.
    Expand(u_f, u_u): u_u = P u_f.  Add(r_u, r_f, A_u, A_base, A_f): r_f += P^T r_u, A_f = A_base + P^T A_u P (A_base is
    A_f: "+="; None: A_f = P^T A_u P; A_u None: residual only; r_u / r_f None: matrix only).  Host arrays or device
    tensors."""
    _prefix = "fold"

    def __init__(self, pattern, node_map, dim, device=0):
        self.pattern_u_ = pattern
        self.node_map_ = np.ascontiguousarray(node_map, dtype=np.int64)
        self.dim_, self.device_ = int(dim), device

    def Prepare(self):
        L = _capi.lib()
        h = C.c_void_p()
        check(L.mimi_hip_fold_create(self.dim_, len(self.node_map_), ptr(self.node_map_, "int64"),
                                     ptr(self.pattern_u_.rowptr, "int64"), ptr(self.pattern_u_.col, "int32"), self.device_,
                                     C.byref(h)))
        self._h = h
        self.n_nodes_f_ = int(L.mimi_hip_fold_info(h, ABI.FOLD_INFO_N_NODES_F))
        self.nnz_f_ = int(L.mimi_hip_fold_info(h, ABI.FOLD_INFO_NNZ_F))
        self.nnz_u_ = int(L.mimi_hip_fold_info(h, ABI.FOLD_INFO_NNZ_U))
        self.n_f_ = self.n_nodes_f_ * self.dim_
        self.n_u_ = len(self.node_map_) * self.dim_
        return self

    def Info(self, what):
        return int(_capi.lib().mimi_hip_fold_info(self._handle(), what))

    def Pattern(self, on_device=False):
        """the folded CSRPattern (the pattern of P^T A P, columns sorted)"""
        if on_device:
            import torch
            dev = torch.device("cuda", self.device_)
            rowptr = torch.empty(self.n_f_ + 1, dtype=torch.int64, device=dev)
            col = torch.empty(self.nnz_f_, dtype=torch.int32, device=dev)
        else:
            rowptr = np.empty(self.n_f_ + 1, dtype=np.int64)
            col = np.empty(self.nnz_f_, dtype=np.int32)
        check(_capi.lib().mimi_hip_fold_pattern(self._handle(), ptr(rowptr), ptr(col)))
        return CSRPattern(rowptr, col, self.nnz_f_)

    def Expand(self, u_f, u_u):
        self._follow_torch(u_f, u_u)
        check(_capi.lib().mimi_hip_fold_expand(self._handle(), fptr(u_f), fptr(u_u)))
        return u_u

    def Add(self, r_u, r_f, A_u=None, A_base=None, A_f=None):
        self._follow_torch(r_u, r_f, A_u, A_base, A_f)
        check(_capi.lib().mimi_hip_fold_add(self._handle(), fptr(r_u), fptr(r_f), fptr(A_u), fptr(A_base), fptr(A_f)))
