"""Host-side callers of the hot path with the reference's Python surface, so that the solver
calls of the reference's tests / examples run against the HIP integrators:

    nl = mimi_amd.NonlinearSolid(); nl.read_mesh(...); nl.elevate_degrees(2); nl.subdivide(1)
    nl.set_material(mat); nl.boundary_condition = bc; nl.runtime_communication = rc
    nl.setup(1); nl.configure_newton("nonlinear_solid", 1e-12, 1e-8, 10, False)
    nl.time_step_size = 0.05; u = nl.solution_view("displacement", "x"); nl.step_time2()

These layers are CALLERS of the path (out of scope for acceleration); they are
restated in plain numpy / scipy only as far as the path's tests need them:
  PySolid / PyNonlinearSolid::Setup        src/mimi/py/py_solid.cpp:9-68, py_nonlinear_solid.cpp:15-387
  operators::NonlinearSolid                src/mimi/operators/nonlinear_solid.cpp:124-292
  forms::Nonlinear::AddMult[Grad]          src/mimi/forms/nonlinear.hpp:53-116
  solvers::LineSearchNewton::Mult          src/mimi/solvers/newton.cpp:10-218
  solvers::GeneralizedAlpha2               src/mimi/solvers/ode.cpp:5-79
The linear solves (UMFPack / CG in the reference) use scipy's sparse LU.  The element
integration itself always goes through libmimi_hip (no CPU fallback).

Differences a user must know: dofs are numbered lexicographically (the reference exposes MFEM's
NURBS numbering); meshes must be single-cell degree-1 descriptions with unit weights (any quadrilateral / hexahedron:
the refined control net is the cell's multilinear map at the Greville abscissae), which
covers every mesh the reference's solver tests use.
"""
import contextlib
import os
import re
import typing

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import nurbs_mesh, splines
from .explicit import ExplicitDynamics
from .integrators import (CouplingSurface, CSRPattern, FollowerPressure, MortarContact,
                          NonlinearSolid as NonlinearSolidIntegrator, PeriodicFold, TANGENT_ANALYTIC, periodic_node_map)
from .kronecker import KroneckerOperator, stiffness_coefficients
from .linear import LinearSolver
from .splines import BSplinePatch


# ---- utils/runtime_communication.hpp:48-198 (the keys that reach the path) -----------------
class RuntimeCommunication:
    """utils/runtime_communication.hpp:48-200 with the pybind11 names of py_runtime_communication.cpp:14-31: runtime
    switches, the save cadence of solution vectors and their .npz output (cnpy::npz_save(..., "a"): one array per call
    appended to the archive `fname`)."""

    def __init__(self):
        self.reals, self.ints = {}, {}
        self.fname = ""
        self._save_every, self._real_history, self._latest = {}, {}, {}
        self.i_timestep_, self.t_ = 0, 0.0

    def set_fname(self, fname):
        self.fname = str(fname)

    def set_real(self, key, value):
        self.reals[key] = float(value)

    def set_int(self, key, value):
        self.ints[key] = int(value)

    def get_real(self, key, default):
        return self.reals.get(key, default)

    def get_int(self, key, default):
        return self.ints.get(key, default)

    # -- time step counter (InitializeTimeStep / NextTimeStep, :71-80) ---------------------------
    def initialize_time_step(self):
        self.i_timestep_, self.t_ = 0, 0.0

    def next_time_step(self, dt):
        self.i_timestep_ += 1
        self.t_ += dt

    # -- save cadence (:115-130) -----------------------------------------------------------------
    def append_should_save(self, name, every):
        self._save_every[str(name)] = int(every)

    def should_save(self, name):
        every = self._save_every.get(name)
        return every is not None and self.i_timestep_ % every == 0

    # -- histories (:132-161) ----------------------------------------------------------------------
    def setup_real_history(self, name, n_reserve):
        self._real_history[name] = []

    def record_real_history(self, name, value):
        self._real_history[name].append(float(value))

    def get_real_history(self, name):
        return self._real_history[name]

    def get_real_history_at(self, name, at):
        return self._real_history[name][at]

    def save_real_history(self, name):
        self.save_vector(name + "_history", np.asarray(self._real_history[name]))

    # -- npz output (:163-197) -------------------------------------------------------------------------
    def save_vector(self, vector_name, vector):
        """append the array `vector_name` to the archive (an .npz is a zip of .npy members)"""
        import zipfile
        if not self.fname:
            raise RuntimeError("Save requested, but fname not set in RuntimeCommunication")
        with zipfile.ZipFile(self.fname, "a", allowZip64=True) as z:
            with z.open(vector_name + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(vector, dtype=np.float64), allow_pickle=False)

    def save_dynamic_vector(self, vector_name, vector):
        self.save_vector(vector_name + str(self.i_timestep_), vector)
        self._latest[vector_name] = np.array(vector, dtype=np.float64)

    def latest_vector(self, vector_name):
        return self._latest[vector_name]


# ---- utils/boundary_conditions.hpp: BCMarker / BoundaryConditions ----------------------------
class BoundaryMarker:
    def __init__(self, initial_config=True):
        self.dirichlet_, self.body_force_, self.contact_ = [], {}, {}
        self.traction_, self.pressure_ = {}, {}
        self.constant_velocity_, self.periodic_boundaries_ = {}, {}
        self.initial_config_ = bool(initial_config)

    def _only_for_initial_config(self, b_name):        # BCMarker::OnlyForInitialConfig (boundary_conditions.cpp:5-11)
        if not self.initial_config_:
            raise RuntimeError(f"{b_name} boundary condition is currently only available for initial config.")

    def dirichlet(self, bid, dim):
        self.dirichlet_.append((int(bid), int(dim)))
        return self

    def body_force(self, dim, value):
        self.body_force_[int(dim)] = float(value)
        return self

    def contact(self, bid, nearest_distance_coeff):
        self.contact_[int(bid)] = nearest_distance_coeff
        return self

    def pressure(self, bid, value):
        """boundary_conditions.cpp:43-50.  The reference stores it and never applies it; here it is a follower load,
        t = -p n da on the current surface (integrators.FollowerPressure)."""
        self._only_for_initial_config("Pressure")
        self.pressure_[int(bid)] = float(value)
        return self

    def traction(self, bid, dim, value):
        """boundary_conditions.cpp:61-69: a dead load on the reference surface, f_a = int t N_a dA0 on the right-hand side
        (py_nonlinear_solid.cpp:243-283)"""
        self._only_for_initial_config("Traction")
        self.traction_.setdefault(int(bid), {})[int(dim)] = float(value)
        return self

    def constant_velocity(self, bid, dim, value):
        """boundary_conditions.cpp:127-138: component `dim` of boundary `bid` moves with velocity `value` (the dofs are
        essential through the implied dirichlet(bid, dim)); applied around every generalized-alpha solve as
        TimeDependentDirichletBoundaryCondition::Apply / Restore (boundary_conditions.cpp:209-291)"""
        self._only_for_initial_config("ConstantVelocity")
        self.dirichlet(bid, dim)
        self.constant_velocity_.setdefault(int(bid), {})[int(dim)] = float(value)
        return self

    def periodic(self, bid0, bid1):
        """boundary_conditions.cpp:150-159: join the faces of boundary ATTRIBUTES bid0 and bid1 -- 1-based ("fortran
        numbering", unlike every other marker's bid, which is attribute bid + 1).  The two faces must be the opposite faces
        of one parametric axis; the joined faces become interior (no load or contact marker may name them)."""
        self._only_for_initial_config("PeriodicBoundary")
        self.periodic_boundaries_[int(bid0)] = int(bid1)
        return self


class BoundaryConditions:
    def __init__(self):
        self.initial = BoundaryMarker(initial_config=True)
        self.current = BoundaryMarker(initial_config=False)


# ---- mesh: MFEM NURBS mesh v1.0, one patch (mimi_amd/nurbs_mesh.py) ------------------------------
class Solid:
    """PySolid (src/mimi/py/py_solid.cpp:9-68): mesh handling."""

    def __init__(self):
        self._dim = None
        self.runtime_communication = None
        self.boundary_condition = None
        self.time_step_size = 0.0
        self.current_time = 0.0

    def read_mesh(self, fname):
        self._nurbs = nurbs_mesh.read_mfem_nurbs(fname)                               # py_solid.cpp:70-95
        self._dim = self._nurbs.dim
        self._faces = self._nurbs.faces

    def elevate_degrees(self, degrees, max_degrees=50):
        if int(degrees) > 0:                                                          # py_solid.cpp:148-168
            self._nurbs = self._nurbs.elevate(int(degrees), int(max_degrees))

    def subdivide(self, n_subdivision):
        for _ in range(int(n_subdivision)):                                           # py_solid.cpp:170-183
            self._nurbs = self._nurbs.refine()

    def mesh_dim(self):
        return self._dim

    def mesh_degrees(self):
        return list(self._nurbs.degrees)

    # counts as py_solid.hpp:130-157
    def n_elements(self):
        return self._nurbs.n_elements()

    def n_vertices(self):
        return self._nurbs.n_vertices()

    def n_boundary_elements(self):
        return self._nurbs.n_boundary_elements()

    def n_subelements(self):
        return self._nurbs.n_subelements()

    def mfem_node_order(self):
        """lexicographic node index of every dof of the reference's (MFEM's) numbering: vectors of the reference, such as
        its golden files, are `v_lexicographic.reshape(-1, dim)[order] = v_reference.reshape(-1, dim)`"""
        return self._nurbs.mfem_order()

    def patch(self):
        nb = self._nurbs
        return BSplinePatch(nb.degrees, nb.knots, nb.ctrl, nb.weights if nb.is_rational() else None)

    def _periodic_axes(self, bc):
        """the parametric axes joined by bc.initial.periodic_boundaries_ (attributes, 1-based), checked"""
        pairs = bc.initial.periodic_boundaries_ if bc is not None else {}
        axes, seen = [], {}
        for b0, b1 in sorted(pairs.items()):
            for b in (b0, b1):
                if b not in self._faces:
                    raise RuntimeError(f"periodic boundary: the mesh has no boundary attribute {b} (attributes: "
                                       f"{sorted(self._faces)}; periodic(bid0, bid1) takes 1-based attributes)")
                if b in seen:
                    raise RuntimeError(f"periodic boundary: attribute {b} appears in two pairs ({seen[b]} and {(b0, b1)})")
                seen[b] = (b0, b1)
            (a0, s0), (a1, s1) = self._faces[b0], self._faces[b1]
            if a0 != a1 or s0 == s1:
                raise RuntimeError(f"periodic boundary: attributes {b0} and {b1} are not the two opposite faces of one "
                                   f"parametric axis (axis {a0} side {s0}, axis {a1} side {s1})")
            axes.append(a0)
        # a joined face is interior: a load or contact on it has no surface to act on (bid -> attribute bid + 1)
        for what, marks in (("pressure", bc.initial.pressure_ if pairs else {}), ("traction", bc.initial.traction_ if pairs else {}),
                            ("contact", {**bc.initial.contact_, **bc.current.contact_} if pairs else {})):
            for bid in marks:
                if bid + 1 in seen:
                    raise RuntimeError(f"periodic boundary: {what} marker on boundary {bid} (attribute {bid + 1}), "
                                       "which the periodic pair makes interior")
        return sorted(axes)

    def dof_map(self, key):
        """PySolid::DofMap (py_solid.cpp:320-331): the (folded) node of every node of the patch, in this facade's
        lexicographic numbering -- the identity without periodic boundaries"""
        if key != "displacement":
            raise KeyError(key)
        patch = self.patch()
        nm = getattr(self, "node_map_", None)
        if nm is None:
            axes = self._periodic_axes(self.boundary_condition)
            nm = periodic_node_map(patch.n_ctrl, axes) if axes else np.arange(patch.n_nodes, dtype=np.int64)
        return np.asarray(nm, dtype=np.int32).copy()


def _element_tables(patch, quadrature_order=-1, with_gradients=False, elements=None):
    """N[e,q,a], w*det[e,q], conn[e,a] (and dN/dX[e,q,i,a]) for the mass matrix / damping / body force; elements: a slice
    of the element range (setup walks large meshes in chunks)."""
    dim = patch.dim
    pmax = max(patch.degrees)
    order = 2 * pmax + 3 if quadrature_order < 0 else quadrature_order
    nq = order // 2 + 1
    tabs = [splines._tables_1d(patch.knots[d], patch.degrees[d], nq) for d in range(dim)]
    m = [len(t[0]) for t in tabs]
    e = np.arange(int(np.prod(m)))
    if elements is not None:
        e = e[elements]
    em = []
    for s in m:
        em.append(e % s)
        e = e // s
    def outer(f):
        """[e, (z,) y, x, (c,) b, a] = product of the 1-D tables f[d][e, a_d, q_d] (plain broadcasting: the three-operand
        einsum of this takes ten times as long)"""
        t = [np.ascontiguousarray(g.transpose(0, 2, 1)) for g in f]            # [e, q_d, a_d]
        r = t[1][:, :, None, :, None] * t[0][:, None, :, None, :]               # [e, y, x, b, a]
        if dim == 3:
            r = t[2][:, :, None, None, :, None, None] * r[:, None, :, :, None, :, :]   # [e, z, y, x, c, b, a]
        return r

    if dim == 2:
        w = np.einsum("y,x->yx", tabs[1][3], tabs[0][3]).ravel()
    else:
        w = np.einsum("z,y,x->zyx", tabs[2][3], tabs[1][3], tabs[0][3]).ravel()
    N = outer([tabs[d][1][em[d]] for d in range(dim)])
    ne = len(em[0])
    N = N.reshape(ne, w.size, -1)
    # connectivity
    conn = np.zeros((ne, N.shape[2]), dtype=np.int64)
    a = np.arange(N.shape[2])
    stride = 1
    for d in range(dim):
        ad = (a // int(np.prod([pp + 1 for pp in patch.degrees[:d]]))) % (patch.degrees[d] + 1)
        conn += ((tabs[d][0][em[d]] - patch.degrees[d])[:, None] + ad[None, :]) * stride
        stride *= patch.n_ctrl[d]
    # geometry Jacobian per point from the control net (derivatives wrt the element's reference coordinates)
    B = [t[1] for t in tabs]
    D = [t[2] for t in tabs]
    dN = []
    for k in range(dim):
        f = [D[d] if d == k else B[d] for d in range(dim)]
        dN.append(outer([f[d][em[d]] for d in range(dim)]).reshape(ne, w.size, -1))
    if getattr(patch, "weights", None) is not None:
        # rational basis: N = B w / sum(B w), with the quotient rule for the derivatives (precomputed.cpp:295-321 via MFEM)
        wa = patch.weights[conn]                                        # [e, a]
        Ws = np.einsum("eqa,ea->eq", N, wa)
        dWs = [np.einsum("eqa,ea->eq", g, wa) for g in dN]
        dN = [(g * wa[:, None, :] * Ws[:, :, None] - (N * wa[:, None, :]) * dW[:, :, None]) / (Ws ** 2)[:, :, None]
              for g, dW in zip(dN, dWs)]
        N = N * wa[:, None, :] / Ws[:, :, None]
    X = patch.control_points[conn]                                      # [e, a, i]
    J = np.stack([np.matmul(g, X) for g in dN], axis=-1)                # [e, q, i, k]
    det = np.linalg.det(J)
    if not np.all(det > 0):
        raise RuntimeError("geometry map has a non-positive Jacobian determinant")
    if with_gradients:
        Jinv = np.linalg.inv(J)                                             # dxi_k / dX_i  [e, q, k, i]
        dN_dX = np.einsum("keqa,eqki->eqia", np.stack(dN), Jinv)            # [e, q, i, a]
        return N, w[None, :] * det, conn, dN_dX
    return N, w[None, :] * det, conn


class Route(typing.NamedTuple):
    """what setup() builds and the steps run, resolved once from the runtime flags (resolve_route)"""
    explicit: bool = False              # explicit_steps in place of step_time2, no matrix of any kind (mimi_amd/explicit.py)
    explicit_consistent: bool = False   # ... with the reference's consistent-mass solve in place of the lumped division
    iterative: bool = False             # GMRES / CG on the device in place of the host's sparse direct solve
    kronecker: bool = False             # ... with the fast-diagonalisation preconditioner in place of Jacobi
    matrix_free: bool = False           # the domain integrator's tangent action in place of the assembled Jacobian
    boundary_actions: bool = False      # ... with the contact and pressure tangents as actions beside it
    periodic_iterative: bool = False    # a periodic pair on the Kronecker, matrix-free and consistent-mass routes
    host_setup: bool = False            # mass, damping and right-hand side in numpy on the host
    consistent_contact: bool = False    # the contact actions carry the derivative of the nodal pressure as well
    friction_actions: bool = False      # ... and Coulomb friction, which is assembled only without it
    operator_jacobi: bool = False       # matrix-free: the reference's Jacobi from the diagonal of the operator itself
    block_jacobi: bool = False          # node-block (dim x dim per control point) Jacobi, assembled or matrix-free
    augmented_contact: bool = False     # the contacts carry nodal multipliers (MortarContact.SetAugmented)


def resolve_route(rc, bc, axes):
    """The Route of the flags of `rc` (a RuntimeCommunication or None), the markers of `bc` and the periodic `axes`, or the
    RuntimeError of the first rule the combination breaks.  No device work; the only place that reads these flags."""
    flag = lambda key: bool(rc is not None and rc.get_int(key, 0))
    # "periodic_iterative": the preconditioner from the folded 1-D matrices (KroneckerOperator(periodic_axes=...)), the solver's
    # product through the fold (LinearSolver.SetOperatorFold).  Without the flag those routes refuse the pair as they always did.
    periodic_iterative = bool(axes) and flag("periodic_iterative")
    # (the first rule asks for its flags itself, ahead of the others: tests/test_periodic_kronecker_cpu.py steps past it by
    # answering that question alone)
    if axes and not periodic_iterative and flag("use_iterative_solver") and flag("use_kronecker_preconditioner"):
        raise RuntimeError("use_kronecker_preconditioner cannot be combined with a periodic boundary "
                           "(boundary_condition.initial.periodic): the folded numbering needs periodic 1-D matrices, "
                           "which the Kronecker preconditioner does not build -- unset one of the two")
    explicit, consistent = flag("explicit_dynamics"), flag("explicit_consistent_mass")
    iterative, kronecker = flag("use_iterative_solver"), flag("use_kronecker_preconditioner")
    matrix_free, boundary_actions = flag("matrix_free"), flag("matrix_free_boundary")
    host_setup = flag("host_setup")
    # "matrix_free_jacobi": mfem::DSmoother without the matrix, 1 / diag from the domain integrator (TangentDiagonal);
    # "use_block_jacobi_preconditioner": the inverted node blocks, out of the CSR values or from the domain integrator
    operator_jacobi, block_jacobi = flag("matrix_free_jacobi"), flag("use_block_jacobi_preconditioner")
    if operator_jacobi and block_jacobi:
        raise RuntimeError("matrix_free_jacobi cannot be combined with use_block_jacobi_preconditioner: a solve has one "
                           "preconditioner -- unset one of the two")
    for name, on in (("matrix_free_jacobi", operator_jacobi), ("use_block_jacobi_preconditioner", block_jacobi)):
        if on and kronecker:
            raise RuntimeError(f"{name} cannot be combined with use_kronecker_preconditioner: a solve has one "
                               "preconditioner -- unset one of the two")
        if on and explicit:
            raise RuntimeError(f"{name} cannot be combined with explicit_dynamics: an explicit step has no linear solve for "
                               "it to act on -- unset one of the two")
    if operator_jacobi and not matrix_free:
        raise RuntimeError("matrix_free_jacobi needs matrix_free: with matrix values the Jacobi preconditioner reads the "
                           "diagonal off them (use_iterative_solver alone)")
    if block_jacobi and not iterative:
        raise RuntimeError("use_block_jacobi_preconditioner needs use_iterative_solver: it preconditions the device GMRES")
    consistent_contact = flag("contact_consistent_tangent")
    if consistent_contact and explicit:
        raise RuntimeError("contact_consistent_tangent cannot be combined with explicit_dynamics: an explicit step has no "
                           "tangent for it to act on -- unset one of the two")
    if consistent_contact and not boundary_actions:
        raise RuntimeError("contact_consistent_tangent needs matrix_free_boundary: the derivative of the nodal pressure "
                           "couples nodes up to 2 p basis functions apart, which leaves the CSR pattern -- it exists as a "
                           "matrix-free action only")
    # "friction_matrix_free": the friction tangent as a part of the contact action (MortarContact.SetFrictionAction).  Without
    # the flag matrix_free_boundary refuses a body with friction as it always did.
    friction_actions = flag("friction_matrix_free")
    if friction_actions and explicit:
        raise RuntimeError("friction_matrix_free cannot be combined with explicit_dynamics: an explicit step has no "
                           "tangent for it to act on -- unset one of the two")
    if friction_actions and not boundary_actions:
        raise RuntimeError("friction_matrix_free needs matrix_free_boundary: it adds the friction tangent to the contact "
                           "action of the matrix-free product")
    # "contact_augmented_lagrange": nodal multipliers on every contact, on every implicit route (assembled or matrix-free,
    # frozen or consistent, with or without friction): whatever reads the nodal pressure reads the augmented one
    augmented_contact = flag("contact_augmented_lagrange")
    if augmented_contact and explicit:
        raise RuntimeError("contact_augmented_lagrange cannot be combined with explicit_dynamics: an explicit step has no "
                           "solve to repeat after a multiplier update -- unset one of the two")
    if explicit:
        for other, on in (("matrix_free", matrix_free), ("use_iterative_solver", iterative)):
            if on:
                raise RuntimeError(f"explicit_dynamics cannot be combined with {other}: an explicit step has no linear solve "
                                   "for it to act on -- unset one of the two")
        if host_setup:
            raise RuntimeError("explicit_dynamics cannot be combined with host_setup: the lumped mass is assembled on the device")
    if consistent:
        if not explicit:
            raise RuntimeError("explicit_consistent_mass needs explicit_dynamics: it is an option of the explicit route")
        if axes and not periodic_iterative:
            raise RuntimeError("explicit_consistent_mass cannot be combined with a periodic boundary: the operator's action and "
                               "the Kronecker preconditioner run in the unwrapped numbering")
    if boundary_actions and not matrix_free:
        raise RuntimeError("matrix_free_boundary needs matrix_free: it adds the contact and pressure tangents to the "
                           "matrix-free product")
    if matrix_free:                                                  # only what the action covers
        if not (iterative and (kronecker or operator_jacobi or block_jacobi)):
            raise RuntimeError("matrix_free needs use_iterative_solver and use_kronecker_preconditioner (or matrix_free_jacobi, "
                               "or use_block_jacobi_preconditioner): without matrix values there is neither a direct solve nor "
                               "a diagonal to read off them")
        if (bc.initial.contact_ or bc.current.contact_) and not boundary_actions:
            raise RuntimeError("matrix_free cannot be combined with a contact marker: the contact tangent has no matrix-free action")
        if bc.initial.pressure_ and not boundary_actions:
            raise RuntimeError("matrix_free cannot be combined with a follower pressure marker: the pressure tangent has no "
                               "matrix-free action")
        rough = [b for b in bc.current.contact_.values() if float(getattr(b, "friction", 0.0)) > 0.0]
        if rough and not friction_actions:
            raise RuntimeError(f"matrix_free_boundary cannot be combined with a contact body with friction (mu = "
                               f"{rough[0].friction:g}): the friction tangent has no matrix-free action")
        if axes and not periodic_iterative:
            raise RuntimeError("matrix_free cannot be combined with a periodic boundary: the action runs in the unwrapped numbering")
    host_setup = host_setup or os.environ.get("MIMI_HIP_HOST_SETUP", "") == "1"
    if explicit and host_setup:
        raise RuntimeError("explicit_dynamics cannot be combined with the host set-up: the lumped mass is assembled on the device")
    return Route(explicit, consistent, iterative, iterative and kronecker, matrix_free, boundary_actions, periodic_iterative, host_setup,
                 consistent_contact, friction_actions, operator_jacobi, block_jacobi, augmented_contact)


class NonlinearSolid(Solid, ExplicitDynamics):
    """PyNonlinearSolid (src/mimi/py/py_nonlinear_solid.cpp:15-387) on top of the HIP integrators; with
    rc.set_int("explicit_dynamics", 1) the explicit central-difference route of mimi_amd/explicit.py."""

    def __init__(self, device=0):
        super().__init__()
        self.material = None
        self.device = device
        self._newton = dict(rel_tol=1e-8, abs_tol=1e-12, max_iter=None, iterative_mode=False)
        self.tangent_mode = TANGENT_ANALYTIC
        self.newton_history = []
        self.augmentation_history = []      # one entry per update_contact_lagrange
        self.augmentation_loops = []        # one entry per step of the automatic loop (contact_augmentations > 0)

    def set_material(self, material):
        self.material = material

    # -- Setup (py_nonlinear_solid.cpp:15-387) -------------------------------------------------
    def setup(self, nthreads=-1):
        dim = self._dim
        bc = self.boundary_condition or BoundaryConditions()
        axes = self._periodic_axes(bc)                               # refusals come before any device work
        # the route and its refusals (resolve_route) come before any device work too
        self.route_ = route = resolve_route(self.runtime_communication, bc, axes)
        self.explicit_, self.explicit_consistent_ = route.explicit, route.explicit_consistent
        self.periodic_axes_ = axes
        self.patch_ = patch = self.patch()
        n = patch.n_vdofs
        # the integrators' pattern: the patch's unwrapped structured one (the tensor kernels' own) -- with periodic
        # boundaries the solver's vectors and matrices live on the folded pattern, and one device pass (PeriodicFold) folds
        # what the integrators assemble
        self.pattern_u_ = CSRPattern.of_bspline_patch(patch, device=self.device)
        self.fold_, self.node_map_ = None, None
        if axes:
            self.node_map_ = periodic_node_map(patch.n_ctrl, axes)
            self.fold_ = PeriodicFold(self.pattern_u_, self.node_map_, dim, device=self.device).Prepare()
            self.pattern_ = self.fold_.Pattern()
            n = self.fold_.n_f_
        else:
            self.pattern_ = self.pattern_u_
        rowptr, col = self.pattern_.rowptr, self.pattern_.col
        self.x = np.zeros(n)        # displacement (py_nonlinear_solid.cpp:119)
        self.x_dot = np.zeros(n)
        # the fixed-point entries' state: a step predicted and not yet advanced, the arrays fixed_point_advance2 fills
        self._fp_open = False
        self._fp_x_, self._fp_v_ = np.zeros((n // dim, dim)), np.zeros((n // dim, dim))
        self.bc_ = bc
        self.surfaces_ = {}
        self._rhs_view_ = None
        # the reference makes the "rhs" linear form only for a body force or a traction (py_nonlinear_solid.cpp:221-283)
        self.has_rhs_ = bool(bc.initial.body_force_) or bool(bc.initial.traction_)
        if self.runtime_communication is None:                       # PySolid::RuntimeCommunication(): created on demand
            self.runtime_communication = RuntimeCommunication()
        rc = self.runtime_communication
        rc.initialize_time_step()                                    # py_solid.cpp:360
        # Dirichlet dofs (FindBoundaryDofIds, py_solid.cpp:185-235): bid -> attribute bid+1
        dofs = []
        for bid, comp in bc.initial.dirichlet_:
            axis, side = self._faces[bid + 1]
            dofs.append(self._folded_dofs(patch.boundary_nodes(axis, side), comp))
        self.dirichlet_ = np.unique(np.concatenate(dofs)) if dofs else np.zeros(0, dtype=np.int64)
        # constant velocity (py_nonlinear_solid.cpp:372-380): dof -> value, later markers over earlier ones (std::map order)
        cv = {}
        for bid, dim_value in sorted(bc.initial.constant_velocity_.items()):
            axis, side = self._faces[bid + 1]
            for comp, value in sorted(dim_value.items()):
                for d in self._folded_dofs(patch.boundary_nodes(axis, side), comp):
                    cv[int(d)] = value
        self.constant_velocity_dofs_ = np.array(sorted(cv), dtype=np.int64)
        self.constant_velocity_values_ = np.array([cv[d] for d in sorted(cv)], dtype=np.float64)
        # mass (VectorMassIntegrator(rho), FormSystemMatrix(zero_dofs); :155-173), damping (:176-192:
        # VectorDiffusionIntegrator(viscosity): C_(a,i),(b,j) = d_ij nu int grad N_a . grad N_b, integrated with the same
        # rule as the mass matrix -- exact on affine patches; mfem's own default rule for this integrator cannot be read
        # here and no reference fixture sets a viscosity: parity unpinned) and rhs (:221-283): on the device
        # (_device_setup, once the integrator and the eliminations exist) unless the host pass is asked for with
        # MIMI_HIP_HOST_SETUP=1 or rc.set_int("host_setup", 1)
        self.host_setup_ = route.host_setup
        self._mass_host, self._visc_host = None, None
        self.d_mass_, self.d_visc_ = None, None
        self.host_nnz_arrays_ = 0                                    # host arrays of nnz doubles made since setup began
        if self.host_setup_:
            self._host_setup(patch, bc, rowptr, col)
        # integrators (py_nonlinear_solid.cpp:197-218, 286-326)
        q_order = rc.get_int("nonlinear_solid_quadrature_order", -1)
        self.domain_ = self._make_domain(q_order)
        self.domain_.SetTangentMode(self.tangent_mode)
        self._finish_setup(patch, bc, rc, q_order)

    def _host_setup(self, patch, bc, rowptr, col):
        """mass, damping and right-hand side in numpy on the host"""
        viscosity = getattr(self.material, "viscosity", -1.0)
        mass, visc, rhs = _assemble_mass_viscosity_rhs(patch, self.pattern_u_.rowptr, self.material.density, viscosity,
                                                       bc.initial.body_force_)
        rhs = self._load_vector_folded(rhs)
        if self.fold_ is not None:
            # assembled on the unwrapped pattern as without periodicity, folded once by the device pass
            mass_f = np.empty(self.pattern_.nnz)
            self.fold_.Add(None, None, mass, None, mass_f)
            mass = mass_f
            if visc is not None:
                visc_f = np.empty(self.pattern_.nnz)
                self.fold_.Add(None, None, visc, None, visc_f)
                visc = visc_f
        self.mass_ = mass
        self.host_nnz_arrays_ += 1 + (visc is not None)
        _eliminate_row_col(rowptr, col, self.mass_, self.dirichlet_)
        self.visc_ = visc
        if visc is not None:
            _eliminate_row_col(rowptr, col, self.visc_, self.dirichlet_)
        self.rhs_ = rhs

    def _make_domain(self, q_order):
        """the domain integrator of the patch with the rule of `q_order`"""
        patch, dim = self.patch_, self._dim
        try:
            return NonlinearSolidIntegrator("nonlinear_solid", self.material, self.pattern_u_, patch=patch,
                                            device=self.device, quadrature_order=q_order).Prepare()
        except RuntimeError as exc:
            if "not a tensor product" not in str(exc):
                raise
        # NURBS weights that do not factorise: the reference's flat per-point tables (general kernels), with the shape
        # values the mass and body-force forms need
        N_t, wd_t, conn_t, dN_dX = _element_tables(patch, q_order, with_gradients=True)
        tables = dict(dim=dim, n_nodes=patch.n_nodes, dofs=conn_t.astype(np.int32), dN_dX=np.ascontiguousarray(dN_dX),
                      weight_det=np.ascontiguousarray(wd_t), N=np.ascontiguousarray(N_t))
        return NonlinearSolidIntegrator("nonlinear_solid", self.material, self.pattern_u_, tables=tables,
                                        device=self.device).Prepare()

    @contextlib.contextmanager
    def _forms_domain(self):
        """the integrator the mass, damping and body-force forms are assembled with: they use the default rule, which is the
        domain integrator's unless nonlinear_solid_quadrature_order is set -- then a handle of its own, dropped on exit"""
        if self.runtime_communication.get_int("nonlinear_solid_quadrature_order", -1) < 0:
            yield self.domain_
            return
        forms = self._make_domain(-1)
        yield forms
        forms.Synchronize()
        del forms

    def _body_force_vector(self, forms):
        """the body-force vector of the unwrapped patch, assembled on the device: n_vdofs doubles on the host"""
        import torch
        r_u = torch.zeros(self.patch_.n_vdofs, dtype=torch.float64, device=torch.device("cuda", self.device))
        b = np.zeros(self._dim)
        for comp, value in self.bc_.initial.body_force_.items():
            b[comp] += value
        if np.any(b != 0.0):
            forms.AddBodyForce(b, r_u)
        return r_u.cpu().numpy()

    def _load_vector_folded(self, rhs):
        """body force `rhs` (unwrapped, modified) + traction, folded, zero on the Dirichlet dofs"""
        patch, bc = self.patch_, self.bc_
        if self.fold_ is None:
            return _load_vector(patch, self._faces, bc.initial.traction_, rhs, self.dirichlet_)
        rhs = _load_vector(patch, self._faces, bc.initial.traction_, rhs, np.zeros(0, dtype=np.int64))
        rhs_f = np.zeros(self.fold_.n_f_)
        self.fold_.Add(rhs, rhs_f)
        return _load_vector(patch, self._faces, {}, rhs_f, self.dirichlet_)

    def _device_setup(self):
        """mass, damping and body force assembled by the domain integrator's forms into zeroed device arrays on the unwrapped
        pattern, folded (PeriodicFold.Add) and eliminated (LinearSolver.Eliminate: EliminateRowCol(DIAG_ONE)) there: no
        array of nnz doubles exists on the host or crosses PCIe.  The traction stays on the host (face work)."""
        import torch
        dev = torch.device("cuda", self.device)

        def assembled(add, factor):
            a = torch.zeros(self.pattern_u_.nnz, dtype=torch.float64, device=dev)
            add(factor, a)
            if self.fold_ is not None:
                a_f = torch.empty(self.pattern_.nnz, dtype=torch.float64, device=dev)
                self.fold_.Add(None, None, a, None, a_f)
                a = a_f
            self.linear_.Eliminate(None, a)
            return a

        with self._forms_domain() as forms:
            self.d_mass_ = assembled(forms.AddMass, self.material.density)
            viscosity = getattr(self.material, "viscosity", -1.0)
            self.d_visc_ = assembled(forms.AddDiffusion, viscosity) if viscosity > 0.0 else None
            self.rhs_ = self._load_vector_folded(self._body_force_vector(forms))

    # mass_ / visc_: the host copies of d_mass_ / d_visc_, downloaded on first read (the direct-solve route and _csr read
    # them; the iterative route never does)
    @property
    def mass_(self):
        if self._mass_host is None and self.d_mass_ is not None:
            self._mass_host = self.d_mass_.cpu().numpy()
            self.host_nnz_arrays_ += 1
        return self._mass_host

    @mass_.setter
    def mass_(self, values):
        self._mass_host = values

    @property
    def visc_(self):
        if self._visc_host is None and self.d_visc_ is not None:
            self._visc_host = self.d_visc_.cpu().numpy()
            self.host_nnz_arrays_ += 1
        return self._visc_host

    @visc_.setter
    def visc_(self, values):
        self._visc_host = values

    def set_body_force(self, dim, value):
        """new body force in direction `dim` (after setup(); the counterpart of set_pressure): the body-force vector is
        assembled again on the device and rhs_ rebuilt IN PLACE -- body force + traction, zero on the Dirichlet dofs --
        so the array linear_form_view2("rhs") handed out stays the one in use; takes effect from the next solve"""
        self.bc_.initial.body_force_[dim] = value
        with self._forms_domain() as forms:
            self.rhs_[:] = self._load_vector_folded(self._body_force_vector(forms))
        del forms                                    # (a temporary handle goes here, not at the return)
        self.has_rhs_ = True
        self.d_rhs_.copy_(self._torch.from_numpy(self.rhs_))

    def _finish_setup(self, patch, bc, rc, q_order):
        dim = self._dim
        self.contacts_ = []
        for bid, body in bc.current.contact_.items():
            axis, side = self._faces[bid + 1]
            self.contacts_.append(MortarContact(body, "contact", self.pattern_u_, patch, axis, side, device=self.device,
                                                quadrature_order=rc.get_int("contact_quadrature_order", -1)).Prepare())
            if self.route_.friction_actions:
                self.contacts_[-1].SetFrictionAction(True)
            if self.route_.consistent_contact:
                self.contacts_[-1].SetConsistentTangent(True)
            if self.route_.augmented_contact:
                self.contacts_[-1].SetAugmented(True)
        # the automatic augmentation loop of step_time2 (off without the mode or with contact_augmentations = 0)
        self._augmentations = max(rc.get_int("contact_augmentations", 0), 0) if self.route_.augmented_contact else 0
        self._gap_tolerance = rc.get_real("contact_gap_tolerance", 0.0)
        # follower pressure (the reference stores BCMarker::pressure_ and never applies it): one device integrator per bid
        self.pressures_, self._pressure_by_bid = [], {}
        for bid, value in bc.initial.pressure_.items():
            axis, side = self._faces[bid + 1]
            fp = FollowerPressure("pressure", self.pattern_u_, patch, axis, side, device=self.device).Prepare()
            fp.SetPressure(value)
            self.pressures_.append(fp)
            self._pressure_by_bid[bid] = fp
        if self._newton["max_iter"] is None:
            self._newton["max_iter"] = 10 * dim                                       # :346-361
        rho_inf = min(max(rc.get_real("ode_coefficient", 0.25), 0.0), 1.0)            # :367-370
        am = (2.0 - rho_inf) / (1.0 + rho_inf)
        af = 1.0 / (1.0 + rho_inf)
        beta = 0.25 * (1.0 + am - af) ** 2
        gamma = 0.5 + am - af
        self._fac = (0.5 - beta / am, af, af * (1.0 - gamma / am), beta * af / am, gamma * af / am, am)  # ode.cpp:5-14
        self._nstate = 0
        # linear solver (py_nonlinear_solid.cpp:327-343): "use_iterative_solver" -> GMRES + Jacobi on the device
        # (mimi_amd/linear.py); else a sparse direct solve on the host (UMFPack in the reference, SuperLU here)
        self.linear_ = LinearSolver(self.pattern_, self.dirichlet_, device=self.device)
        route = self.route_
        self.use_iterative_solver_, self.matrix_free_ = route.iterative, route.matrix_free
        # "use_kronecker_preconditioner" (with the iterative solver only): the fast-diagonalisation operator of
        # mimi_amd/kronecker.py in place of Jacobi, for the Newton solves and the explicit mass solve
        self.use_kronecker_, self._kronecker_pushed = False, None
        if route.kronecker:
            self._set_kronecker()
        if route.block_jacobi:
            self.linear_.SetNodeBlock(dim)
            self.linear_.preconditioner = "block_jacobi"
        if route.operator_jacobi:
            self.linear_.SetOperatorDiagonal(True)    # ("jacobi" stays the solver's preconditioner)
        if self.fold_ is not None and (self.matrix_free_ or self.explicit_consistent_):
            # the operator handles stay in the unwrapped numbering: the solver's product expands and folds around them
            # (set once: it survives every SetOperator)
            self.linear_.SetOperatorFold(self.fold_)
        if self.explicit_:
            self._explicit_setup()
        elif not self.host_setup_:
            self._device_setup()
        self._to_device()
        if self.explicit_:
            self._explicit_make_stepper()

    def _set_kronecker(self):
        """the Kronecker preconditioner of the patch on the solver: the implicit routes and the consistent-mass solve"""
        self.linear_.SetKronecker(KroneckerOperator(self.patch_, self.dirichlet_, self._dim, periodic_axes=self.periodic_axes_))
        self.linear_.preconditioner = "kronecker"
        self.use_kronecker_, self._kronecker_pushed = True, None

    def _folded_dofs(self, nodes, comp):
        """dofs (node, comp) of unwrapped nodes in the solver's numbering (through the periodic node map), unique"""
        nodes = np.asarray(nodes, dtype=np.int64)
        if self.node_map_ is not None:
            nodes = np.unique(self.node_map_[nodes])
        return nodes * self._dim + comp

    def configure_newton(self, name, rel_tol, abs_tol, max_iter, iterative_mode):   # py_solid.cpp:334-346
        self._newton = dict(rel_tol=rel_tol, abs_tol=abs_tol, max_iter=int(max_iter), iterative_mode=bool(iterative_mode))

    def set_pressure(self, bid, value):
        """new pressure on boundary `bid` (marked with boundary_condition.initial.pressure before setup): a float, or values
        at the face's nodes (FollowerPressure.FaceNodes order); used from the next assembly on (load ramps between steps)"""
        if bid not in getattr(self, "_pressure_by_bid", {}):
            raise KeyError(f"boundary {bid} has no pressure marker: mark it with boundary_condition.initial.pressure "
                           "before setup()")
        self._pressure_by_bid[bid].SetPressure(value)

    def solution_view(self, fe_space, component):
        """"x" (the displacement), "x_dot", "x_ref" (the nodes' reference positions, py_nonlinear_solid.cpp:91-114): host
        arrays in this facade's node order, the solver's own storage for the first two (write prescribed values in place)"""
        if component == "x_ref":
            x_ref = np.ascontiguousarray(self.patch_.control_points, dtype=np.float64)
            if self.node_map_ is not None:
                # the lowest copy of every folded node (the node map is ascending in it)
                _, first = np.unique(self.node_map_, return_index=True)
                x_ref = x_ref.reshape(-1, self._dim)[first]
            return x_ref.reshape(-1).copy()
        return {"x": self.x, "x_dot": self.x_dot}[component]

    # -- operators::NonlinearSolid ----------------------------------------------------------------
    # ---- device-resident state ---------------------------------------------------------------------
    # x, v, a, the residual, the mass / viscosity / Jacobian values and the right-hand side live in HBM (torch tensors
    # as the memory container); the integrators, the eliminations, the matrix-vector products and -- on the iterative
    # route -- the linear solves use them in place.  The host sees: norms (scalars), the solution after a step
    # (n_vdofs doubles into the arrays `solution_view` hands out) and, on the reference's default direct-solve route
    # only, the Jacobian values for the host factorisation.
    def _to_device(self):
        import torch
        self._torch = torch
        dev = torch.device("cuda", self.device)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        if self.host_setup_:
            self.d_mass_ = f(self.mass_)
            self.d_visc_ = f(self.visc_) if self.visc_ is not None else None
        self.d_rhs_ = f(self.rhs_)
        self._rhs = self.d_rhs_           # what the residual subtracts (_update_rhs)
        if not self.matrix_free_ and not self.explicit_:
            self.d_jac_ = torch.zeros_like(self.d_mass_)
        self.d_dirichlet_ = torch.from_numpy(np.asarray(self.dirichlet_, dtype=np.int64)).to(dev)
        self.d_x_, self.d_v_ = f(self.x), f(self.x_dot)
        if self.fold_ is not None:
            # the integrators' side of the fold: expanded x, unwrapped residual and values
            self.d_xu_ = torch.zeros(self.fold_.n_u_, dtype=torch.float64, device=dev)
            self.d_ru_ = torch.zeros_like(self.d_xu_)
            if not self.explicit_ and not self.matrix_free_:
                self.d_Au_ = torch.zeros(self.fold_.nnz_u_, dtype=torch.float64, device=dev)
        if len(self.constant_velocity_dofs_):
            self.d_cv_dofs_ = torch.from_numpy(self.constant_velocity_dofs_).to(dev)
            self.d_cv_values_ = f(self.constant_velocity_values_)
        self.pcie_csr_bytes_ = 0          # CSR values that crossed PCIe since setup (direct-solve route only)

    def _csr(self, vals):
        n = len(self.x)
        return sp.csr_matrix((vals, self.pattern_.col, self.pattern_.rowptr), shape=(n, n))

    def _push(self, integ):
        integ.dt_, integ.first_effective_dt_, integ.second_effective_dt_ = self.time_step_size, self._fac0, self._fac1

    # ---- the seam: what the integrators see -------------------------------------------------------------
    # The integrators work in the patch's unwrapped numbering, the solver in the folded one.  Every assembly and every step
    # goes through these entries, the only ones that ask whether there is a fold and the only ones that walk the integrators.
    @property
    def boundaries_(self):
        """the boundary integrators in assembly order: contacts, then pressures (the domain comes before them)"""
        return self.contacts_ + self.pressures_

    @property
    def integrators_(self):
        """every integrator in assembly order: the domain, then the boundaries"""
        return [self.domain_] + self.boundaries_

    def _expand(self, x):
        """the vector the integrators read for the solver's x: x through the fold, x itself without one"""
        return x if self.fold_ is None else self.fold_.Expand(x, self.d_xu_)

    def _open(self, x, y):
        """(xu, target): the expanded x and the zeroed unwrapped residual the integrators add into -- x and y themselves
        without a fold; _close(target, y) finishes"""
        if self.fold_ is None:
            return x, y
        xu = self._expand(x)
        self.d_ru_.zero_()
        return xu, self.d_ru_

    def _close(self, target, y):
        """y += the fold of target (nothing without a fold: the integrators wrote into y)"""
        if self.fold_ is not None:
            self.fold_.Add(target, y)

    def _add_residual(self, x, y, linearize=False):
        """y += the residual of every integrator at x; linearize: each one also takes the snapshot of its tangent action there"""
        xu, target = self._open(x, y)
        self.domain_.AddDomainResidual(xu, target)
        if linearize:
            self.domain_.Linearize(xu)
        for c in self.boundaries_:
            c.AddBoundaryResidual(xu, target)
            if linearize:
                c.Linearize(xu)
        self._close(target, y)

    def _add_residual_and_grad(self, x, y):
        """y += the residual, d_jac_ = d_mass_ + fac0 K of every integrator at x.  Without a fold the domain integrator writes
        J = M + fac0 K in one pass where "+=" would read J (std::copy_n(mass_A_, ...) followed by AddMultGrad:
        mimi_hip_domain_add_residual_and_grad_from -- no 2 x nnz copy, and the domain integrator of a single-patch solid
        touches every row); with one everything goes into the zeroed unwrapped r_u / A_u and ONE fold forms
        y += P^T r_u, J = M + P^T A_u P"""
        xu, r = self._open(x, y)
        if self.fold_ is None:
            A = self.d_jac_
            self.domain_.AddDomainResidualAndGradFrom(xu, self._fac0, r, self.d_mass_, A)
        else:
            A = self.d_Au_
            A.zero_()
            self.domain_.AddDomainResidualAndGrad(xu, self._fac0, r, A)
        for c in self.boundaries_:
            c.AddBoundaryResidualAndGrad(xu, self._fac0, r, A)
        if self.fold_ is not None:
            self.fold_.Add(r, y, A, self.d_mass_, self.d_jac_)

    def _post_time_advance(self, x, domain=True, boundaries=True, commit=True):
        """PostTimeAdvance at the solver's x of the chosen integrators (the boundary ones read the scalars of the latest
        residual evaluation back: an explicit step leaves them to the next download; a contact with friction first evaluates
        and commits its state at x).  commit=False: the scalars only -- the explicit loop has committed on the device"""
        xp = self._expand(x)
        if domain:
            self.domain_.DomainPostTimeAdvance(xp)
        for c in self.boundaries_ if boundaries else ():
            if commit:
                c.BoundaryPostTimeAdvance(xp)
            else:
                c._history()

    def _raise_device_errors(self):
        """The integrators get device tensors, so their calls only enqueue and an error raised by a kernel -- a return map
        that cannot solve its scalar equation, where the reference throws out of the evaluation -- waits in the handle's status
        word (include/mimi_hip.h: "kernel-raised errors").  Read the words: called where the host has just waited for the
        stream anyway, so it costs one 4-byte copy per integrator.  Raises the reference's RuntimeError; the words are cleared
        and the integrators stay usable."""
        for integ in self.integrators_:
            integ.Synchronize()

    def _displacement(self, u):
        """the current displacement (u None) or the host vector u in this facade's numbering, as a device vector"""
        if u is None:
            return self.d_x_
        x = self._torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64).reshape(-1)).to(self.d_x_.device)
        if x.numel() != self.d_x_.numel():
            raise ValueError(f"u has {x.numel()} entries, the displacement has {self.d_x_.numel()}")
        return x

    def _add_mult(self, xt, y):                       # forms/nonlinear.hpp:53-81
        self._push(self.domain_)
        self._add_residual(xt, y)
        self.linear_.Eliminate(y, None)               # y[ess] = 0

    def _linear_part(self, a, y):
        """y = M a [+ C (v_alpha + fac1 a)]   (operators/nonlinear_solid.cpp:177-187,249-255)"""
        y.zero_()
        self.linear_.AddMult(self.d_mass_, a, y)
        if self.d_visc_ is not None:
            self.linear_.AddMult(self.d_visc_, self._va + self._fac1 * a, y)

    def _mult(self, a):                               # operators/nonlinear_solid.cpp:172-205
        xt = self._xa + self._fac0 * a
        y = self._torch.empty_like(a)
        self._linear_part(a, y)
        self._add_mult(xt, y)
        y -= self._rhs
        self.linear_.Eliminate(y, None)
        return y

    def _residual_and_grad(self, a):                  # operators/nonlinear_solid.cpp:240-283
        xt = self._xa + self._fac0 * a
        y = self._torch.empty_like(a)
        self._linear_part(a, y)
        self._push(self.domain_)
        if self.matrix_free_:
            # no Jacobian: the residual-only assembly, the snapshot of the tangent at x_t, and the solver's product becomes
            # rho M + fac0 K(x_t) + fac1 eta C of the domain integrator; with "matrix_free_boundary"
            # every contact and pressure integrator adds its residual, is linearised at x_t too and joins the product.
            # With a periodic pair ("periodic_iterative") the product goes through the fold set in setup
            self._add_residual(xt, y, linearize=True)
            eta = getattr(self.material, "viscosity", -1.0)
            self.linear_.SetOperator(self.domain_, self.material.density, self._fac0,
                                     self._fac1 * eta if self.d_visc_ is not None else 0.0)
            for c in self.boundaries_:
                self.linear_.AddBoundaryOperator(c, self._fac0)
            self.linear_.Eliminate(y, None)
            y -= self._rhs
            self.linear_.Eliminate(y, None)
            return y, None
        self._add_residual_and_grad(xt, y)
        self.linear_.Eliminate(y, self.d_jac_)        # forms/nonlinear.hpp:76-80,112-115
        if self.d_visc_ is not None:
            self.d_jac_.add_(self.d_visc_, alpha=self._fac1)     # jacobian_->Add(fac1_, viscosity_->SpMat())
        y -= self._rhs
        self.linear_.Eliminate(y, None)
        return y, self.d_jac_

    def _push_kronecker(self, fac0, fac1):
        """the coefficients of the Kronecker operator for J = M + fac0 K + fac1 C, pushed when they change"""
        if not self.use_kronecker_ or self._kronecker_pushed == (fac0, fac1):
            return
        m = self.material
        self.linear_.SetKroneckerCoefficients(m.density, stiffness_coefficients(m.lambda_, m.mu, fac0, fac1,
                                                                                  getattr(m, "viscosity", -1.0), self._dim))
        self._kronecker_pushed = (fac0, fac1)

    def _solve(self, J, r):
        """the linear solve of a Newton iteration (py_nonlinear_solid.cpp:327-343)"""
        if self.use_iterative_solver_:
            self._push_kronecker(self._fac0, self._fac1)
            return self.linear_.Mult(J, r, self._torch.zeros_like(r))        # GMRES + Jacobi, all in HBM
        # the reference's default: a sparse direct solve (UMFPack there, SuperLU here) -- on the host
        Jh = J.cpu().numpy()
        self.pcie_csr_bytes_ += Jh.nbytes
        c = spla.splu(self._csr(Jh).tocsc()).solve(r.cpu().numpy())
        return self._torch.from_numpy(c).to(r.device)

    def _newton_solve(self, x0):                      # solvers/newton.cpp:10-218
        torch = self._torch
        o = self._newton

        def nrm(t):
            """the norm of a residual on the host, and with it whether the evaluation behind it failed on the device: a step
            whose return map fails raises here, before anything is committed, as the reference throws out of StepTime2"""
            value = float(torch.linalg.vector_norm(t))
            self._raise_device_errors()
            return value

        x = x0.clone() if o["iterative_mode"] else torch.zeros_like(x0)
        improved, i_improved = [True] * 5, 0
        best_res, best_x = np.finfo(float).max, x.clone()
        r, J = self._residual_and_grad(x)
        norm0 = norm = nrm(r)
        goal = max(o["rel_tol"] * norm, o["abs_tol"])
        it, converged = 0, False
        while True:
            if norm <= goal:
                converged = True
                break
            if it >= o["max_iter"]:
                if it != 0:
                    x = best_x.clone()
                break
            if not any(improved):
                x = best_x.clone()
                break
            c = self._solve(J, r)
            q1 = norm
            q3 = nrm(self._mult(x - c))
            q2 = nrm(self._mult(x - 0.5 * c))
            den = q1 - 2.0 * q2 + q3
            eps = (3.0 * q1 - 4.0 * q2 + q3) / (4.0 * den) if den != 0 else np.inf
            scale = eps if (den > 0 and 0 < eps < 1) else (1.0 if q3 < q1 else 0.05)
            if abs(scale) < 1e-12:
                break
            x = x - scale * c
            if it == o["max_iter"] - 1:
                r = self._mult(x)
            else:
                r, J = self._residual_and_grad(x)
            norm = nrm(r)
            if norm < best_res:
                best_x, best_res = x.clone(), norm
                improved[i_improved % 5] = True
            else:
                improved[i_improved % 5] = False
            i_improved += 1
            it += 1
        self.newton_history.append(dict(converged=converged, iterations=it, norm=norm, norm0=norm0))
        return x

    # -- GeneralizedAlpha2::StepTime2 / FixedPointSolve2 / FixedPointAdvance2 / AdvanceTime2 (solvers/ode.cpp:16-187) ----
    # A step is: predict (once per step), the Newton solve of aa, commit.  step_time2 runs the three in a row; the
    # fixed-point entries run them apart, so `fixed_point_solve2(); advance_time2()` performs the same operations in the same
    # order as `step_time2()` and gives the same bits.
    def _update_rhs(self):
        """the right-hand side of the next solve, pushed before every solve: the host view linear_form_view2 handed out (if
        one was requested) into d_rhs_, plus the loads of the coupling surfaces with the Dirichlet rows zeroed -- one
        vector, so still one subtraction per residual evaluation.  A solid with neither subtracts d_rhs_ as it is."""
        torch = self._torch
        if self._rhs_view_ is not None:
            self.d_rhs_.copy_(torch.from_numpy(self._rhs_view_))
        loads = [s.load_ for _, s in sorted(self.surfaces_.items()) if s.load_ is not None]
        if not loads:
            self._rhs = self.d_rhs_
            return
        rhs = self.d_rhs_.clone()
        for f in loads:
            rhs += f
        self.linear_.Eliminate(rhs, None)
        self._rhs = rhs

    def _predict(self):
        """StepTime2 up to the solve (ode.cpp:38-58; FixedPointSolve2's predictor, :87-103)"""
        torch = self._torch
        dt = self.time_step_size
        f0, f1, f2, f3, f4, f5 = self._fac
        # what the caller may have written through solution_view since the last step (n_vdofs doubles)
        self.d_x_.copy_(torch.from_numpy(self.x))
        self.d_v_.copy_(torch.from_numpy(self.x_dot))
        x, v = self.d_x_, self.d_v_
        self._fac0, self._fac1 = f3 * dt * dt, f4 * dt
        self._update_rhs()
        if self._nstate == 0:
            z = torch.zeros_like(x)                    # operators/nonlinear_solid.cpp:124-156
            self._add_mult(x, z)
            if self.d_visc_ is not None:
                self.linear_.AddMult(self.d_visc_, v, z)
            z = self._rhs - z
            if self.use_iterative_solver_:
                # mass_inv_: mfem::CGSolver + DSmoother (operators/nonlinear_solid.cpp:39-50,155)
                self._push_kronecker(0.0, 0.0)
                self._a = self.linear_.MultCG(self.d_mass_, z, torch.zeros_like(z))
            else:
                self._a = torch.from_numpy(spla.splu(self._csr(self.mass_).tocsc()).solve(z.cpu().numpy())).to(x.device)
            self._raise_device_errors()                # (the evaluation at the initial x)
            self._aa = torch.zeros_like(x)
            self._nstate = 1
        a = self._a
        self._xa = x + (v + f0 * dt * a) * (f1 * dt)
        self._va = v + f2 * dt * a
        self._saved_x = None
        if len(self.constant_velocity_dofs_):
            # TimeDependentDirichletBoundaryCondition::Apply (boundary_conditions.cpp:209-259, ode.cpp:56-58)
            idx, val = self.d_cv_dofs_, self.d_cv_values_
            self._aa[idx] = 0.0
            self._va[idx] = val
            self._xa[idx] = x[idx] + val * dt
            self._saved_x = self._xa[idx].clone()

    def _extrapolate(self, x, v):
        """x, v <- the end-of-step vectors of the current aa, in place (ode.cpp:61-68, and the Restore of x and v, :73-75)"""
        aa = self._aa
        f1 = self._fac[1]
        xa = self._xa + self._fac0 * aa
        va = self._va + self._fac1 * aa
        prev = 1.0 - 1.0 / f1
        x.mul_(prev).add_(xa, alpha=1.0 / f1)
        v.mul_(prev).add_(va, alpha=1.0 / f1)
        if self._saved_x is not None:
            # ... Restore (boundary_conditions.cpp:261-291)
            x[self.d_cv_dofs_] = self._saved_x
            v[self.d_cv_dofs_] = self.d_cv_values_

    def _commit(self):
        """AdvanceTime2 (ode.cpp:148-187) and PySolid's save cadence (py_solid.cpp:494-510)"""
        dt = self.time_step_size
        f1, f5 = self._fac[1], self._fac[5]
        x, v = self.d_x_, self.d_v_
        self._extrapolate(x, v)
        self._a = self._a * (1.0 - 1.0 / f1) + self._aa / f5
        if self._saved_x is not None:
            self._a[self.d_cv_dofs_] = 0.0
        # PostTimeAdvance (operators/nonlinear_solid.cpp:285-292)
        self._push(self.domain_)
        self._post_time_advance(x)
        self._raise_device_errors()                    # (the commit runs the return map once more: before the time moves on)
        self.current_time += dt
        # the arrays solution_view handed out (zero-copy views of the reference: py_solid.cpp:379-388)
        self.x[:] = x.cpu().numpy()
        self.x_dot[:] = v.cpu().numpy()
        rc = self.runtime_communication
        if rc is not None:
            self._save_cadence()
            rc.next_time_step(dt)

    def _save_cadence(self, before=None):
        """PySolid::StepTime2 (py_solid.cpp:433-440): x_<step> and v_<step> from the host arrays where the save cadence asks,
        in the reference's (MFEM's) dof numbering; beyond the reference the nodal fields, <field name>_<step>, in its node
        order.  before(): runs once if anything is due, ahead of the first write.  Returns the number of fields saved."""
        rc = self.runtime_communication
        names = [k for k in ("x", "v") + tuple(NonlinearSolidIntegrator.FIELDS) if rc.should_save(k)]
        if names and before is not None:
            before()
        for k in names:
            if k == "x":
                rc.save_dynamic_vector("x_", self.in_reference_numbering(self.x))
            elif k == "v":
                rc.save_dynamic_vector("v_", self.in_reference_numbering(self.x_dot))
            else:
                f = self.field(k)
                rc.save_dynamic_vector(k + "_", self.in_reference_numbering(f, ncomp=f.shape[1]))
        return len([k for k in names if k not in ("x", "v")])

    def step_time2(self):
        """PySolid::StepTime2 (py_solid.cpp:425-441).

        Difference from the reference: refused (RuntimeError) while a fixed-point step is open, i.e. after a
        fixed_point_solve2() that no advance_time2() has committed yet; the reference would silently commit that step's
        stale alpha levels."""
        self._explicit_refuse("step_time2")
        if self._fp_open:
            raise RuntimeError("step_time2() while a fixed-point step is open: finish it with advance_time2() first")
        self._predict()
        self._aa = self._newton_solve(self._aa)
        self._augment()
        self._commit()

    # -- augmented-Lagrangian contact (rc.set_int("contact_augmented_lagrange", 1)) ---------------------------------------
    def _require_augmented(self, what):
        if not getattr(self, "route_", None) or not self.route_.augmented_contact:
            raise RuntimeError(f"{what} needs contact_augmented_lagrange: the contacts carry no multipliers")

    def update_contact_lagrange(self, apply=True):
        """The Uzawa step of every contact at the configuration of the latest converged residual, x_a + fac0 aa:
        dlambda_i = p_i - lambda_i and, with `apply`, lambda_i <- p_i.  Returns the largest violation max |dlambda_i| / eps (a
        length) over the contacts and appends dict(time, apply, violation, contacts=[MortarContact.UpdateLagrange's dict per
        contact]) to augmentation_history.  The multipliers are an iterate, not history: they survive the step as a warm
        start and no trial copy is kept.  Expect the violation to shrink like k / (k + eps) per update, k the effective
        stiffness under the contact: useful at a penalty of the order of the body's stiffness, not at a soft one."""
        self._require_augmented("update_contact_lagrange()")
        if getattr(self, "_xa", None) is None or getattr(self, "_aa", None) is None:
            raise RuntimeError("update_contact_lagrange() before any solve: there is no converged configuration to measure")
        xu = self._expand(self._xa + self._fac0 * self._aa)
        per = [c.UpdateLagrange(xu, apply) for c in self.contacts_]
        violation = max([d["violation"] for d in per], default=0.0)
        self.augmentation_history.append(dict(time=self.current_time, apply=bool(apply), violation=violation, contacts=per))
        return violation

    def fill_contact_lagrange(self, value=0.0):
        """every multiplier of every contact <- value (projected onto lambda <= 0); the way to drop multipliers a node kept
        because all its points slid past the rim of a spline body"""
        self._require_augmented("fill_contact_lagrange()")
        for c in self.contacts_:
            c.FillLagrange(value)

    def _augment(self):
        """the automatic loop behind the first Newton solve of step_time2: measure; stop at the tolerance or after
        contact_augmentations updates (converged=False, nothing raised, as Newton's own limit); else update and solve again
        from the current aa"""
        if not self._augmentations or not self.contacts_:
            return
        applied, violations = 0, []
        while True:
            violations.append(self.update_contact_lagrange(apply=False))
            if violations[-1] <= self._gap_tolerance or applied >= self._augmentations:
                break
            self.update_contact_lagrange(apply=True)
            applied += 1
            self._aa = self._newton_solve(self._aa)
        self.augmentation_loops.append(dict(converged=violations[-1] <= self._gap_tolerance, augmentations=applied,
                                            violations=violations))

    # -- partitioned coupling: PySolid::FixedPointSolve2 / FixedPointAdvance2 / AdvanceTime2 (py_solid.cpp:443-511) -----
    def fixed_point_solve2(self):
        """Solve the current step with the current loads and commit nothing (GeneralizedAlpha2::FixedPointSolve2,
        ode.cpp:81-111): the first call of a step takes x / x_dot from the host arrays, forms the initial acceleration on the
        first step, predicts the alpha levels and applies constant velocity; every call then runs the Newton solve of aa.
        x, x_dot, the acceleration, the material state and the contact history stay untouched, so calling it again (after
        set_traction / a write to linear_form_view2) re-solves the same step.  `fixed_point_solve2(); advance_time2()` gives
        the same bits as `step_time2()`.

        Differences from the reference, both RuntimeError where the reference silently commits stale alpha levels:
        advance_time2() without a fixed_point_solve2() in the step, and step_time2() while a fixed-point step is open."""
        self._explicit_refuse("fixed_point_solve2")
        if not self._fp_open:
            self._predict()
            self._fp_open = True
        else:
            self._update_rhs()
        self._aa = self._newton_solve(self._aa)

    def fixed_point_advance2(self):
        """(x, v), each (n // dim, dim): the end-of-step vectors the current aa gives, after the constant-velocity Restore
        (GeneralizedAlpha2::FixedPointAdvance2, ode.cpp:113-146).  The same two host arrays on every call, updated in place;
        no solver state changes."""
        self._explicit_refuse("fixed_point_advance2")
        if not self._fp_open:
            raise RuntimeError("FixedPointAdvance2() should be called after FixedPointSolve2()")
        x, v = self.d_x_.clone(), self.d_v_.clone()
        self._extrapolate(x, v)
        self._fp_x_.reshape(-1)[:] = x.cpu().numpy()
        self._fp_v_.reshape(-1)[:] = v.cpu().numpy()
        return self.fixed_point_advanced_vector_views()

    def fixed_point_advanced_vector_views(self):
        """the arrays of the latest fixed_point_advance2, not recomputed (py_solid.cpp:482-492)"""
        return self._fp_x_, self._fp_v_

    def advance_time2(self):
        """Commit the step of the latest fixed_point_solve2 (GeneralizedAlpha2::AdvanceTime2, ode.cpp:148-187): x / v / a,
        the constant-velocity Restore, DomainPostTimeAdvance and the boundary integrators' post-advance, current_time, the
        host arrays, the RuntimeCommunication save cadence and next_time_step; the predictor is re-armed.

        Difference from the reference: refused (RuntimeError) without a fixed_point_solve2() in the step; the reference
        would silently commit stale alpha levels."""
        self._explicit_refuse("advance_time2")
        if not self._fp_open:
            raise RuntimeError("advance_time2() without a fixed_point_solve2() in this step: there is no solved step to "
                               "commit")
        self._commit()
        self._fp_open = False

    # -- the accessors a coupling reads (py_solid.cpp:363-407, py_solid.hpp:213-218) ------------------------------------
    def linear_form_view2(self, lf_name):
        """PySolid::LinearFormView2: the writable host view of the right-hand side "rhs" (body force plus traction,
        Dirichlet rows zero).  What the caller writes there is used from the next step_time2 / fixed_point_solve2 on (pushed
        to the device before every solve).  As in the reference it exists only when a body force or traction marker made
        it (py_nonlinear_solid.cpp:221-283); otherwise, and for any other name, KeyError."""
        if lf_name != "rhs" or not getattr(self, "has_rhs_", False):
            raise KeyError(f"Requested linear form -{lf_name}- does not exist.")
        self._rhs_view_ = self.rhs_
        return self.rhs_

    def boundary_dof_ids(self, fe_space, bid, dim):
        """PySolid::BoundaryDofIds: the dofs of component `dim` on boundary `bid` (attribute bid + 1, as the markers), in
        this facade's numbering (folded on periodic solids), sorted"""
        if fe_space != "displacement":
            raise KeyError(fe_space)
        axis, side = self._faces[int(bid) + 1]
        return np.sort(self._folded_dofs(self.patch_.boundary_nodes(axis, side), int(dim))).astype(np.int32)

    def zero_dof_ids(self, fe_space):
        """PySolid::ZeroDofIds: the sorted unique Dirichlet dofs (constant-velocity dofs included: that marker implies
        dirichlet)"""
        if fe_space != "displacement":
            raise KeyError(fe_space)
        return np.asarray(self.dirichlet_, dtype=np.int32).copy()

    def newton_final_norms(self, name):
        """PySolid::NewtonFinalNorms: (final / initial, final) residual norm of the latest Newton solve, of step_time2 or
        fixed_point_solve2"""
        if name != "nonlinear_solid":
            raise KeyError(name)
        if not self.newton_history:
            return 0.0, 0.0
        h = self.newton_history[-1]
        return (h["norm"] / h["norm0"] if h["norm0"] else 0.0), h["norm"]

    def coupling_surface(self, bid, quadrature_order=-1):
        """integrators.CouplingSurface of boundary `bid` (attribute bid + 1, as the markers), in this facade's numbering:
        points(u) hands a fluid partner the wet surface, set_traction(t, u) takes its traction back as nodal forces that are
        subtracted with the right-hand side from the next solve on (step_time2 and fixed_point_solve2).  The load is dead
        within a solve and has no tangent: the coupling iteration carries its dependence on the geometry (a follower load
        with an exact tangent is bc.initial.pressure's).  One object per bid (a second call with another quadrature_order is
        refused); call after setup()."""
        if getattr(self, "surfaces_", None) is None:
            raise RuntimeError("coupling_surface() needs setup() first")
        bid = int(bid)
        if bid in self.surfaces_:
            s = self.surfaces_[bid]
            if s.quadrature_order_ != quadrature_order:
                raise RuntimeError(f"coupling surface of boundary {bid} exists with quadrature_order "
                                   f"{s.quadrature_order_}, not {quadrature_order}")
            return s
        if bid + 1 not in self._faces:
            raise RuntimeError(f"coupling surface: the mesh has no boundary {bid} (attribute {bid + 1}; attributes: "
                               f"{sorted(self._faces)})")
        joined = {b for pair in self.bc_.initial.periodic_boundaries_.items() for b in pair}
        if bid + 1 in joined:
            raise RuntimeError(f"coupling surface on boundary {bid} (attribute {bid + 1}), which the periodic pair makes "
                               "interior")
        axis, side = self._faces[bid + 1]
        s = CouplingSurface(self.patch_, axis, side, device=self.device, quadrature_order=quadrature_order,
                            fold=self.fold_).Prepare()
        self.surfaces_[bid] = s
        return s

    def field(self, name, where="nodes", u=None):
        """A stress / state field as a host array: "cauchy_stress" ([i + j dim], sigma = P F^T / det F),
        "von_mises_stress" (sqrt(3/2) |sigma - tr(sigma)/dim I|: the trace over dim as in the reference's Dev, so the q of
        its J2 yield function; in 3-D the usual von Mises stress), "det_F", "accumulated_plastic_strain", "temperature".

        where = "points": [n_el, n_q, ncomp] at the quadrature points; "nodes": [n_nodes, ncomp], the lumped L2 projection
        sum_q w det N_A f / sum_q w det N_A (reproduces constants, stays within the point values around a node).  u: a
        displacement in this facade's numbering (default: the committed one).  With periodic boundaries sum and weight are
        computed on the unwrapped nodes and folded before the division: the result is in the folded numbering, like
        solution_view."""
        if name not in NonlinearSolidIntegrator.FIELDS:
            raise ValueError(f"unknown field {name!r} (known: {', '.join(NonlinearSolidIntegrator.FIELDS)})")
        if where not in ("nodes", "points"):
            raise ValueError(f"where must be 'nodes' or 'points', got {where!r}")
        if getattr(self, "domain_", None) is None:
            raise RuntimeError("field() needs setup()")
        torch = self._torch
        x = self._displacement(u)
        xu = self._expand(x)
        self.domain_.dt_ = self.time_step_size      # (the effective dts do not reach the material)
        ncomp = self.domain_.FieldComponents(name)
        if where == "points":
            return self.domain_.PointField(name, xu)
        n_u = self.patch_.n_nodes
        s = torch.zeros((n_u, ncomp), dtype=torch.float64, device=x.device)
        w = torch.zeros(n_u, dtype=torch.float64, device=x.device)
        self.domain_.NodalField(name, xu, s, w)
        s, w = s.cpu().numpy(), w.cpu().numpy()
        if self.node_map_ is not None:
            n_f = int(self.node_map_.max()) + 1
            sf, wf = np.zeros((n_f, ncomp)), np.zeros(n_f)
            np.add.at(sf, self.node_map_, s)
            np.add.at(wf, self.node_map_, w)
            s, w = sf, wf
        return s / w[:, None]

    def in_reference_numbering(self, vec, ncomp=None):
        """byVDIM vector of this facade (lexicographic nodes) -> the reference's dof order (MFEM's NURBS numbering).
        ncomp: components per node (default: dim, a displacement-like vector; 1 for a scalar nodal field).

        With periodic boundaries the vector is expanded first (every copy of a joined node gets its value) and written
        in the NON-periodic reference numbering: MFEM's numbering of a periodic space cannot be restated without MFEM."""
        order = self._nurbs.mfem_order()
        v = np.asarray(vec).reshape(-1, self._dim if ncomp is None else int(ncomp))
        if getattr(self, "node_map_", None) is not None and len(v) != len(order):
            v = v[self.node_map_]
        return np.ascontiguousarray(v[order]).reshape(-1)

    def from_reference_numbering(self, vec):
        """inverse of in_reference_numbering (periodic: the value of a joined node is its lowest copy's)"""
        order = self._nurbs.mfem_order()
        out = np.zeros(len(order) * self._dim)
        out.reshape(-1, self._dim)[order] = np.asarray(vec).reshape(-1, self._dim)
        if getattr(self, "node_map_", None) is not None:
            _, first = np.unique(self.node_map_, return_index=True)
            out = np.ascontiguousarray(out.reshape(-1, self._dim)[first]).reshape(-1)
        return out


def _structured_positions(patch, rowptr, conn):
    """Position in the CSR value array of (row = node conn[e, a] component 0, column = node conn[e, b] component 0) in the
    structured pattern of a lexicographically numbered patch (CSRPattern.of_bspline_patch): the columns of a node's row are
    the nodes of its window [A_d - p_d, A_d + p_d] (clipped), lexicographic, times the components -- so the position is
    arithmetic, no search through the 10^8 column indices of a large mesh.  Returns pos0[e, a, b] and the row lengths."""
    dim = patch.dim
    row0 = conn * dim
    n_e, n_a = conn.shape
    rank = np.zeros((n_e, n_a, n_a), dtype=np.int64)
    width = np.ones((n_e, n_a), dtype=np.int64)
    rem = conn.copy()
    for d in range(dim):
        n_d, p_d = patch.n_ctrl[d], patch.degrees[d]
        x = rem % n_d                       # coordinate of every node of the element in direction d
        rem = rem // n_d
        lo = np.maximum(x - p_d, 0)         # the window of a ROW node
        w = np.minimum(x + p_d, n_d - 1) - lo + 1
        rank += (x[:, None, :] - lo[:, :, None]) * width[:, :, None]
        width = width * w
    return rowptr[row0][:, :, None] + dim * rank, rowptr[row0 + 1] - rowptr[row0]


def _assemble_mass_viscosity_rhs(patch, rowptr, density, viscosity, body_force, chunk=8192):
    """mass (VectorMassIntegrator(rho), py_nonlinear_solid.cpp:155-173), damping (:176-192: VectorDiffusionIntegrator(
    viscosity): C_(a,i),(b,j) = d_ij nu int grad N_a . grad N_b, integrated with the rule of the mass matrix -- exact on
    affine patches; mfem's own default rule for this integrator cannot be read here and no reference fixture sets a
    viscosity: parity unpinned) and the body-force vector (:221-283) of the whole patch, on the host.
    Elements are taken COLOUR by colour (element index modulo p + 1 per direction): two elements of a colour share no
    node, so their entries go to distinct positions and one vectorised `+=` adds them -- in a fixed order of the colours,
    the same bits every run."""
    dim = patch.dim
    n = patch.n_vdofs
    nnz = int(rowptr[-1])
    mass = np.zeros(nnz)
    visc = np.zeros(nnz) if viscosity > 0.0 else None
    rhs = np.zeros(n)
    spans = list(patch.n_spans)
    e_all = np.arange(patch.n_elements)
    em, rem = [], e_all
    for d in range(dim):
        em.append(rem % spans[d])
        rem = rem // spans[d]
    colour = np.zeros(patch.n_elements, dtype=np.int64)
    mult = 1
    for d in range(dim):
        colour += (em[d] % (patch.degrees[d] + 1)) * mult
        mult *= patch.degrees[d] + 1
    order = np.argsort(colour, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=mult))])
    for cidx in range(mult):
        els_c = order[bounds[cidx]:bounds[cidx + 1]]
        for s0 in range(0, len(els_c), chunk):
            els = els_c[s0:s0 + chunk]
            if visc is not None:
                N, wd, conn, dN_dX = _element_tables(patch, with_gradients=True, elements=els)
                G = dN_dX.reshape(dN_dX.shape[0], -1, dN_dX.shape[3])                    # [e, (q, i), a]
                Ce = viscosity * np.matmul((G * np.repeat(wd, dim, axis=1)[:, :, None]).transpose(0, 2, 1), G)
            else:
                N, wd, conn = _element_tables(patch, elements=els)
            Me = density * np.matmul((N * wd[:, :, None]).transpose(0, 2, 1), N)           # [e, a, b]
            pos0, row_len = _structured_positions(patch, rowptr, conn)
            # the rows of a node's other components follow with the same column pattern: + c (row length) for the row,
            # + c for the column
            for c in range(dim):
                pos = (pos0 + c * row_len[:, :, None] + c).ravel()
                mass[pos] += Me.ravel()
                if visc is not None:
                    visc[pos] += Ce.ravel()
            fe = np.einsum("eq,eqa->ea", wd, N)
            for comp, value in body_force.items():
                rhs[(conn * dim + comp).ravel()] += (fe * value).ravel()
    return mass, visc, rhs


def _load_vector(patch, faces, traction, rhs, dirichlet):
    """the right-hand side of py_nonlinear_solid.cpp:221-283: the body-force vector `rhs` (modified in place) plus the
    traction of every marked boundary (VectorBoundaryLFIntegrator with a PWConstCoefficient per attribute: bid -> attribute
    bid + 1, as for Dirichlet), then zero on the Dirichlet dofs (rhs->SetSubVector(zero_dofs, 0.0))"""
    for bid, dim_value in traction.items():
        axis, side = faces[bid + 1]
        rhs += traction_vector(patch, axis, side, dim_value)
    rhs[dirichlet] = 0.0
    return rhs


def traction_vector(patch, axis, side, dim_value, quadrature_order=-1):
    """Dead-load traction on the face {xi_axis = side} of the patch in the reference configuration (mfem's
    VectorBoundaryLFIntegrator, py_nonlinear_solid.cpp:243-283): f_(a,i) = t_i int N_a dA0 for dim_value = {i: t_i}, with
    the rule of the body force (2 p + 3 unless given).  Faces of rational patches are refused (splines.face_tables)."""
    dim = patch.dim
    dofs, N, dN, weight = splines.face_tables(patch, axis, side, quadrature_order)
    X = np.asarray(patch.control_points, dtype=np.float64)[dofs]          # [f, a, i]
    T = np.einsum("fqka,fai->fqki", dN, X)                                # tangents [f, q, k, i]
    if dim == 2:
        dA = np.hypot(T[:, :, 0, 0], T[:, :, 0, 1])
    else:
        dA = np.linalg.norm(np.cross(T[:, :, 0, :], T[:, :, 1, :]), axis=-1)
    fe = np.einsum("fq,fqa->fa", weight * dA, N)                          # int N_a dA0 per face node
    nodal = np.bincount(dofs.ravel(), weights=fe.ravel(), minlength=patch.n_nodes)
    out = np.zeros(patch.n_vdofs)
    for comp, value in dim_value.items():
        out[comp::dim] += value * nodal
    return out


def _eliminate_row_col(rowptr, col, vals, dofs):
    """SparseMatrix::EliminateRowCol(rc, DIAG_ONE) for each rc (forms/nonlinear.hpp:112-115)."""
    n = len(rowptr) - 1
    mask = np.zeros(n, dtype=bool)
    mask[dofs] = True
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    kill = mask[rows] | mask[col]
    vals[kill] = 0.0
    vals[kill & (rows == col) & mask[rows]] = 1.0
