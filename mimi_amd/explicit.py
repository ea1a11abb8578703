"""The explicit central-difference step with a lumped mass (include/mimi_hip.h: mimi_hip_explicit_*): the reference's
CentralDifference = Newmark(beta = 0, gamma = 1/2) (solvers/ode.hpp:257, ode.cpp:229-250) with the consistent-mass solve
replaced by a division, and an energy ledger beside it.  Device tensors only.

    s = ExplicitStepper(n, fixed, prescribed, prescribed_velocity).Prepare(); s.SetMass(m)
    s.Start(v, f, r0, d0)                                    # a_0; the works are zeroed
    s.Predict(dt, x, v); <r1 = forces(x), d1 = damping(v)>; s.Correct(dt, f, r1, d1, v)
    s.Energies(dt) -> {"KE", "W_int", "W_ext", "W_damp", "Q", "E_star"}

E* = KE - Q + W_int + W_damp - W_ext is conserved by the scheme in exact arithmetic (for any internal force, with the
lagged damping and with prescribed dofs, while f stays put): the step's built-in self-check.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ABI, check, fptr

# The shape of the ledger's sums (mimi_amd/csrc/explicit.hip; mimi_hip_explicit_info(NULL, MIMI_HIP_EXPLICIT_INFO_SUM_*) returns the
# same numbers):
# a launch has min(ceil(n / SUM_BLOCK), SUM_GRID_CAP) workgroups of SUM_BLOCK threads; a thread adds its dofs i, i + stride,
# ... in ascending order, the workgroup adds by a tree of log2(SUM_BLOCK) levels, and the last workgroup adds the partials,
# SUM_FINAL_RUN consecutive ones per thread and the same tree again.
SUM_BLOCK = 256
SUM_GRID_CAP = 1024
SUM_FINAL_RUN = SUM_GRID_CAP // SUM_BLOCK
SUM_TREE_DEPTH = 16

ENERGY_NAMES = ("KE", "W_int", "W_ext", "W_damp", "Q", "E_star")


def sum_grid(n):
    """workgroups of a launch over n dofs"""
    return min(-(-int(n) // SUM_BLOCK), SUM_GRID_CAP)


def sum_run_length(n):
    """the most values any thread adds one after the other on the way of a term into a sum over n dofs: its own dofs, then
    the partials.  A sum of the ledger is within (sum_run_length(n) + SUM_TREE_DEPTH + 2) 2^-53 sum|terms| of the exact
    one: a run of k values makes k - 1 rounded additions and there are two runs, the trees add SUM_TREE_DEPTH, a term
    itself is rounded twice, and the factor (dt, dt / 2, dt^2 / 8) and the sum of the two parts of W_ext once each."""
    return -(-int(n) // (sum_grid(n) * SUM_BLOCK)) + SUM_FINAL_RUN


class ExplicitStepper(_capi.Handle):
    _prefix = "explicit"

    def __init__(self, n, fixed=None, prescribed=None, prescribed_velocity=None, device=0):
        """fixed / prescribed: byte masks of n entries (numpy or torch, None: none set); prescribed_velocity: n doubles,
        read where `prescribed` is set"""
        self.n_, self.device_ = int(n), device
        as_mask = lambda a: None if a is None else (np.ascontiguousarray(a, dtype=np.uint8) if isinstance(a, np.ndarray) else a)
        self.fixed_, self.prescribed_ = as_mask(fixed), as_mask(prescribed)
        self.prescribed_velocity_ = (np.ascontiguousarray(prescribed_velocity, dtype=np.float64)
                                     if isinstance(prescribed_velocity, np.ndarray) else prescribed_velocity)
        for a in (self.fixed_, self.prescribed_, self.prescribed_velocity_):
            if a is not None and (a.size if isinstance(a, np.ndarray) else a.numel()) != self.n_:
                raise ValueError(f"masks and prescribed velocities must have {self.n_} entries")

    def Prepare(self):
        h = C.c_void_p()
        check(_capi.lib().mimi_hip_explicit_create(self.n_, _capi.ptr(self.fixed_, "uint8"), _capi.ptr(self.prescribed_, "uint8"),
                                                   fptr(self.prescribed_velocity_), self.device_, C.byref(h)))
        self._h = h
        return self

    def Info(self, what):
        return int(_capi.lib().mimi_hip_explicit_info(self._handle(), what))

    def PreviousForcePointers(self):
        """(r, d) addresses of the force vectors of the previous step the handle keeps (by pointer: no copy)"""
        return self.Info(ABI.EXPLICIT_INFO_R_PREV), self.Info(ABI.EXPLICIT_INFO_D_PREV)

    def SetMass(self, m):
        self._follow_torch(m)
        check(self._fn("set_mass")(self._handle(), fptr(m)))

    def Start(self, v, f, r, d=None):
        self._follow_torch(v, f, r, d)
        check(self._fn("start")(self._handle(), fptr(v), fptr(f), fptr(r), fptr(d)))

    def Predict(self, dt, x, v):
        self._follow_torch(x, v)
        check(self._fn("predict")(self._handle(), float(dt), fptr(x), fptr(v)))

    def Correct(self, dt, f, r, d, v):
        self._follow_torch(v, f, r, d)
        check(self._fn("correct")(self._handle(), float(dt), fptr(f), fptr(r), fptr(d), fptr(v)))

    def Acceleration(self, out):
        self._follow_torch(out)
        check(self._fn("acceleration")(self._handle(), fptr(out)))
        return out

    def Energies(self, dt):
        """the six numbers as a dict; the only call that waits for the device"""
        out = np.zeros(6)
        check(self._fn("energies")(self._handle(), float(dt), _capi.ptr(out)))
        return dict(zip(ENERGY_NAMES, (float(v) for v in out)))


def power_start(n):
    """the start vector of the power iterations: the same numbers every run, with a share of every mode"""
    return np.random.default_rng(0).standard_normal(int(n))


def power_lambda_max(apply, m, free, z, rel_tol, max_iter):
    """(lambda, iterations): the largest eigenvalue of K z = lambda diag(m) z on the dofs where `free` is 1, by the power
    iteration z <- M^-1 K z with the Rayleigh quotient z.Kz / z.Mz, which approaches lambda_max from below (K symmetric
    positive semi-definite); stops when two successive quotients differ by at most rel_tol of the last.  apply(z) -> K z;
    numpy arrays or torch tensors (only *, /, sum are used)."""
    z = z * free
    lam = 0.0
    for it in range(1, int(max_iter) + 1):
        y = apply(z) * free
        new = float((z * y).sum()) / float((z * m * z).sum())
        z = y / m * free
        z = z / float((z * z).sum()) ** 0.5
        if abs(new - lam) <= rel_tol * abs(new):
            return new, it
        lam = new
    return lam, int(max_iter)


def stable_step_from(lam_k, lam_c, safety):
    """safety (2 / omega) (sqrt(1 + xi^2) - xi) with omega = sqrt(lam_k), xi = lam_c / (2 omega): the central-difference limit
    with the damping force lagged by half a step"""
    omega = lam_k ** 0.5
    xi = lam_c / (2.0 * omega)
    return safety * (2.0 / omega) * ((1.0 + xi * xi) ** 0.5 - xi)


class ExplicitDynamics:
    """What NonlinearSolid adds under rc.set_int("explicit_dynamics", 1) (before setup()): explicit_steps(n) in place of
    step_time2().  No Jacobian and no mass or viscosity matrix is allocated; the mass is the lumped one (the row sums of the
    consistent mass, assembled as the body-force form with b = rho), a step is predict, one residual-only assembly of every
    integrator (and the damping force eta C v through the tangent action, without a linearisation), correct, and the state
    commit.  x, v, a and the force vectors stay on the device; the host arrays of solution_view are refreshed when
    explicit_steps returns and where the save cadence asks for output.  With rc.set_int("explicit_consistent_mass", 1) beside the
    flag the division by the lumped mass becomes the reference's solve (rho M + dt/2 eta C) a = f - r - eta C v_{n+1/2}, by the
    operator CG with the Kronecker preconditioner, still without a matrix; that route keeps no ledger.  It takes a periodic pair
    under rc.set_int("periodic_iterative", 1): the CG then runs on the folded dofs, its product through the fold."""

    explicit_ = False
    explicit_consistent_ = False

    def _explicit_require(self):
        if not self.explicit_:
            raise RuntimeError('explicit dynamics is off: call runtime_communication.set_int("explicit_dynamics", 1) before setup()')

    def _explicit_refuse(self, entry):
        if self.explicit_:
            raise RuntimeError(f"{entry}() under explicit_dynamics: there is no Jacobian and no Newton loop -- advance with "
                               "explicit_steps(n)")

    def _explicit_setup(self):
        """the lumped mass and the load vector on the device; no matrix"""
        import torch
        dev = torch.device("cuda", self.device)
        dim = self._dim
        with self._forms_domain() as forms:
            m_u = torch.zeros(self.patch_.n_vdofs, dtype=torch.float64, device=dev)
            forms.AddBodyForce(self.material.density * np.ones(dim), m_u)
            if self.fold_ is not None:
                m = torch.zeros(self.fold_.n_f_, dtype=torch.float64, device=dev)
                self.fold_.Add(m_u, m)
            else:
                m = m_u
            self.d_lumped_mass_ = m
            self.rhs_ = self._load_vector_folded(self._body_force_vector(forms))

    def _explicit_make_stepper(self):
        import torch
        n = len(self.x)
        fixed, pres, vbar = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n)
        fixed[self.dirichlet_] = 1
        pres[self.constant_velocity_dofs_] = 1
        vbar[self.constant_velocity_dofs_] = self.constant_velocity_values_
        self.explicit_stepper_ = ExplicitStepper(n, fixed, pres, vbar, device=self.device).Prepare()
        self.explicit_stepper_.SetMass(self.d_lumped_mass_)
        self.d_free_ = torch.from_numpy(1.0 - np.maximum(fixed, pres)).to(self.d_x_.device)
        self._fac0 = self._fac1 = 0.0                # (the integrators' effective dts: an explicit step has none)
        eta = getattr(self.material, "viscosity", -1.0)
        self._ex_eta = eta if eta > 0.0 else 0.0
        # two force vectors each, alternated: the stepper reads the previous one again, by pointer
        self._ex_r = [torch.zeros_like(self.d_x_), torch.zeros_like(self.d_x_)]
        self._ex_d = [torch.zeros_like(self.d_x_), torch.zeros_like(self.d_x_)] if self._ex_eta else None
        self._ex_i, self._ex_started = 0, False
        self.explicit_d2h_copies_ = 0                # solution-sized device-to-host copies since setup
        if self.explicit_consistent_:
            # the mass solve's preconditioner, built here: the caller sets no solver flag on this route
            self._set_kronecker()
            self.d_vbar_ = torch.from_numpy(vbar).to(self.d_x_.device)
            self._cm_a, self._cm_rhs = torch.zeros_like(self.d_x_), torch.zeros_like(self.d_x_)
            self.explicit_cg_iterations_ = []        # of every mass solve since setup

    def _explicit_forces(self, x, out):
        """out = the RAW internal force of the domain, contact and pressure integrators at x: no elimination, the ledger
        needs the reactions"""
        out.zero_()
        self._push(self.domain_)
        self._add_residual(x, out)

    def _explicit_action(self, z, out, stiffness, viscosity):
        """out = (stiffness K(linearised u) + viscosity C) z of the domain integrator, through the fold when there is one"""
        out.zero_()
        zu, target = self._open(z, out)
        self.domain_.ApplyTangent(zu, target, stiffness=stiffness, density=0.0, viscosity=viscosity)
        self._close(target, out)
        return out

    def _consistent_solve(self, fac1):
        """a <- (rho M + fac1 eta C)^-1 (f - r - eta C v) at the current x and v, the essential dofs eliminated (a = 0 there):
        the operator CG of the implicit route's mass solve, with the tangent action in place of a matrix"""
        r, rhs, eta = self._ex_r[0], self._cm_rhs, self._ex_eta
        self._explicit_forces(self.d_x_, r)
        self._torch.sub(self._rhs, r, out=rhs)
        if eta:
            rhs.sub_(self._explicit_action(self.d_v_, self._ex_d[0], 0.0, eta))
        self.linear_.Eliminate(rhs, None)
        self._push_kronecker(0.0, fac1)
        self.linear_.SetOperator(self.domain_, self.material.density, 0.0, fac1 * eta)
        self.linear_.MultCG(None, rhs, self._cm_a)
        self.explicit_cg_iterations_.append(self.linear_.final_iter_)
        if not self.linear_.converged_:
            raise RuntimeError(f"explicit_consistent_mass: the mass solve did not converge in {self.linear_.final_iter_} iterations")

    def explicit_restart(self):
        """take up the host arrays of solution_view ("x", "x_dot") and form the acceleration from them; the works of the
        ledger restart at zero"""
        self._explicit_require()
        torch = self._torch
        self.d_x_.copy_(torch.from_numpy(self.x))
        self.d_v_.copy_(torch.from_numpy(self.x_dot))
        self._update_rhs()
        self._ex_i = 0
        if self.explicit_consistent_:
            self.d_v_.mul_(self.d_free_).add_(self.d_vbar_)          # v = 0 on fixed dofs, the prescribed value on the others
            self._consistent_solve(0.0)                              # rho M a_0 = f - r_0 - eta C v_0
        else:
            r, d = self._ex_r[0], None
            self._explicit_forces(self.d_x_, r)
            if self._ex_d is not None:
                d = self._explicit_action(self.d_v_, self._ex_d[0], 0.0, self._ex_eta)
            self.explicit_stepper_.Start(self.d_v_, self._rhs, r, d)
        # outside the step loop a wait costs nothing: a return map that fails at the start displacement raises here, before a
        # step is taken or anything is committed (inside the loop the words are read once per explicit_steps call)
        self._raise_device_errors()
        self._ex_started = True

    def _explicit_download(self):
        """x and x_dot into the host arrays, and the boundary integrators' post-advance, which reads the scalars of the latest
        residual evaluation back: only where the host looks"""
        self.x[:] = self.d_x_.cpu().numpy()
        self.x_dot[:] = self.d_v_.cpu().numpy()
        self.explicit_d2h_copies_ += 2
        self._post_time_advance(self.d_x_, domain=False, commit=False)

    def _lumped_step(self, dt):
        st, x, v = self.explicit_stepper_, self.d_x_, self.d_v_
        st.Predict(dt, x, v)
        k = 1 - self._ex_i
        r, d = self._ex_r[k], None
        self._explicit_forces(x, r)
        if self._ex_d is not None:
            d = self._explicit_action(v, self._ex_d[k], 0.0, self._ex_eta)
        st.Correct(dt, self._rhs, r, d, v)
        self._ex_i = k

    def _consistent_step(self, dt):
        # the essential dofs have a = 0 and keep their v, so the masks hold without a kernel of their own
        x, v = self.d_x_, self.d_v_
        v.add_(self._cm_a, alpha=0.5 * dt)
        x.add_(v, alpha=dt)
        self._consistent_solve(0.5 * dt)
        v.add_(self._cm_a, alpha=0.5 * dt)

    def explicit_steps(self, n):
        """n central-difference steps of time_step_size.  Inside the loop nothing is copied to the host and nothing waits
        for the device, except at the steps where runtime_communication.should_save asks for output (after step k the
        counter is k: append_should_save("x", 2) writes x_2, x_4, ..., as step_time2 writes them).  Afterwards x and x_dot are
        downloaded once and the status words of the handles are read once: a failed return map raises here.  The state
        continues on the device, so n steps and n more give the bytes of 2 n steps; explicit_restart() takes up host edits."""
        self._explicit_require()
        if not self.time_step_size > 0.0:
            raise RuntimeError(f"explicit_steps needs a positive time_step_size, got {self.time_step_size}")
        if not self._ex_started:
            self.explicit_restart()
        else:
            self._update_rhs()
        step = self._consistent_step if self.explicit_consistent_ else self._lumped_step
        for _ in range(int(n)):
            dt = self.time_step_size
            step(dt)
            self._post_time_advance(self.d_x_, boundaries=False)
            for c in self.contacts_:                 # friction: the state of the step's force evaluation, on the device
                if c.friction_ > 0.0:
                    c.CommitFriction()
            self.current_time += dt
            self.runtime_communication.next_time_step(dt)
            fields = self._save_cadence(before=self._explicit_download)      # (the download counts its own two copies)
            self.explicit_d2h_copies_ += fields
        self._explicit_download()
        for handle in self.integrators_ + [self.explicit_stepper_]:
            handle.Synchronize()

    def explicit_energies(self):
        """{"KE", "W_int", "W_ext", "W_damp", "Q", "E_star"} of the ledger since the last (re)start, Q with the current
        time_step_size.  E_star is conserved by the scheme up to rounding: a drift is the sign of an unstable step."""
        self._explicit_require()
        if self.explicit_consistent_:
            raise RuntimeError("explicit_energies() under explicit_consistent_mass: the ledger belongs to the lumped-mass step")
        if not self._ex_started:
            self.explicit_restart()
        return self.explicit_stepper_.Energies(self.time_step_size)

    def explicit_acceleration(self):
        """the current acceleration as a host array"""
        self._explicit_require()
        if not self._ex_started:
            self.explicit_restart()
        if self.explicit_consistent_:
            return self._cm_a.cpu().numpy()
        a = self.explicit_stepper_.Acceleration(self._torch.empty_like(self.d_x_))
        return a.cpu().numpy()

    def stable_time_step(self, u=None, safety=0.9, rel_tol=1e-3, max_iter=500):
        """safety x the central-difference limit of the BODY at the displacement u (default: the current one):
        (2 / omega) (sqrt(1 + xi^2) - xi), omega^2 = lambda_max(M_l^-1 K(u)) and xi = lambda_max(M_l^-1 eta C) / (2 omega)
        (0 without viscosity), each by a power iteration with the tangent action (Linearize / ApplyTangent), the prescribed
        dofs masked, from a fixed start vector.  The Rayleigh quotient approaches lambda_max from below, so the estimate
        errs long: the safety factor covers that.  The contact penalty and a follower pressure are NOT in it -- a stiff
        contact lowers the limit further; watch E_star of explicit_energies(), which drifts as soon as a step is too long."""
        self._explicit_require()
        torch = self._torch
        x = self._displacement(u)
        self._push(self.domain_)
        self.domain_.Linearize(self._expand(x))
        z0 = torch.from_numpy(power_start(x.numel())).to(x.device)
        m, free = self.d_lumped_mass_, self.d_free_
        out = torch.empty_like(x)
        lam_k, self.stable_iterations_ = power_lambda_max(lambda z: self._explicit_action(z, out, 1.0, 0.0), m, free, z0, rel_tol, max_iter)
        lam_c = 0.0
        if self._ex_eta:
            lam_c, it = power_lambda_max(lambda z: self._explicit_action(z, out, 0.0, self._ex_eta), m, free, z0, rel_tol, max_iter)
            self.stable_iterations_ = max(self.stable_iterations_, it)
        self.stable_lambda_ = (lam_k, lam_c)
        return stable_step_from(lam_k, lam_c, safety)
