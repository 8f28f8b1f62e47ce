"""Host-side mirror of the reference's contact-implicit MPC policy over the device solver.

  ci_mpc_policy(traj, s, obj; H_mpc, N_sample, κ_mpc, mode, n_opts, ip_opts)     src/controller/policy.jl:42-96
  policy(p::CIMPC, traj, t)                                                       src/controller/policy.jl:98-146

The reference policy owns a rotating copy of the reference trajectory (`p.traj`), a window of knot indices and a
Newton workspace; every `N_sample` simulator steps it solves `newton_solve!(p.newton, p.s, p.q0, q1, p.window,
p.im_traj, p.traj, warm_start = t > 1)`, rotates the reference (`rot_n_stride!`), advances the window and returns
`newton.traj.u[1] / N_sample` until the next solve.  Here the trajectory, the window and the workspace live on the
GPU (`cimpc_set_gait`, `cimpc_newton_solve`, `cimpc_mpc_advance`); per step the host sends `q0, q1` (2 nq doubles per
robot) and reads `u1` back.  B robots / Monte-Carlo rollouts run in lock step (same cadence, independent states).
"""
from __future__ import annotations

import numpy as np

from .solver import CIMPCSolver, InteriorPointOptions, NewtonOptions


def update_altitude(model, alt, gamma_hist, q_hist, threshold=1.0):
    """`update_altitude!(alt, ϕ, s, traj, t, nc, N_sample; threshold)` (mpc_utils.jl:109-136) on the window of simulator
    steps the caller hands over (the reference looks at steps max(0, t-1-N_sample)+1 .. t-1): per contact point, the step
    with the largest normal impulse decides - if it exceeds `threshold`, the altitude becomes ϕ_i at the configuration
    that step ended in.  gamma_hist: (n, nc); q_hist: (n, nq) with q_hist[j] = traj.q[j+2]; alt: (nc,) updated in place."""
    import torch
    gamma_hist = np.asarray(gamma_hist, dtype=np.float64).reshape(-1, model.nc)
    q_hist = np.asarray(q_hist, dtype=np.float64).reshape(gamma_hist.shape[0], model.nq)
    for i in range(model.nc):
        g_max, idx = 0.0, -1
        for j in range(gamma_hist.shape[0]):
            if gamma_hist[j, i] > g_max:
                g_max, idx = gamma_hist[j, i], j
        if g_max > threshold:
            alt[i] = float(model.phi(torch.as_tensor(q_hist[idx]))[i])
    return alt


class CIMPCPolicy:
    def __init__(self, problem, obj_q, obj_u, H_mpc=None, N_sample=1, kappa_mpc=None, B=1, mode=0,
                 n_opts: NewtonOptions | None = None, ip_opts: InteriorPointOptions | None = None, device=0,
                 phase=None, obj_gamma=None, obj_b=None, obj_v=None, v_target=None, altitude_update=False,
                 altitude_impact_threshold=1.0, device_tables=False, gains=False, control_gain_scaling=100.0,
                 velocity_gain_scaling=100.0, gains_N=10):
        """problem: a `lcp_models.ReferenceProblem` (reference trajectory + per-knot linearization at κ_mpc);
        obj_q, obj_u: (H_mpc, nq, nq), (H_mpc, nu, nu) TrackingObjective weights; obj_gamma / obj_b: contact-force
        weights of `:configurationforce` mode (mode = 1, the default of ci_mpc_policy); obj_v (+ v_target): the
        velocity weights of a TrackingVelocityObjective.  altitude_update / altitude_impact_threshold: CIMPCOptions
        (policy.jl:5-14): before every solve after the first, `update_altitude!` over the simulator steps since the last solve
        (handed over through `observe`, which `plant.simulate` calls), then `set_altitude!` (policy.jl:110-117).
        device_tables: the knots are linearized and their tables built on the device in one call (`CIMPCSolver.linearize_knots`,
        from problem.z, problem.theta and the device plant model of problem.model's name) instead of one `set_linearization` per
        knot from the problem's (r0, rz0, rθ0); a problem made with `tables=False` has none and needs it.
        gains (CIMPCOptions.gains, policy.jl:11-13; needs obj_v): the time-varying LQR gains of the reference trajectory
        (`gains.reference_gains` on problem.z, problem.theta with obj_q[0], obj_v[0], obj_u[0], gains_N repeats and the two scalings:
        `reference_gains(s, traj, obj; N, U_scaling, V_scaling)`, gains.jl:17-51), computed once on the device; every call then returns
        (u1 + K[window[1]] ([q_ref[1]; q_ref[2]] - [q0; q1])) / N_sample with q0 = q1 - N_sample (q1 - q_prev), q_prev the configuration of
        the previous call: the feedback line of examples/centroidal_quadruped/continuous_policy_v3.jl:74-85 in the discrete policy -
        a placement of this build, the reference's own policy() never applies its gains."""
        if gains and obj_v is None:
            raise ValueError("gains=True needs obj_v: reference_gains takes a TrackingVelocityObjective")
        m = problem.model
        self.problem = problem
        self.H = H_mpc or problem.H
        self.N_sample = int(N_sample)
        self.B = B
        kappa = problem.kappa if kappa_mpc is None else kappa_mpc
        if abs(kappa - problem.kappa) > 0:
            raise ValueError("the linearization table was built at κ = %g, policy asks for κ_mpc = %g" % (problem.kappa, kappa))
        if not device_tables and (problem.r0 is None or problem.rz0 is None or problem.rth0 is None):
            raise ValueError("the problem was made with tables=False: it has no (r0, rz0, rθ0); pass device_tables=True")
        self.kappa = kappa
        self.solver = CIMPCSolver(m.nq, m.nu, m.nw, m.nc, m.nb, problem.H, self.H, B=B, mode=mode,
                                  ip_opts=ip_opts or InteriorPointOptions(kappa_tol=kappa),       # policy.jl:54-61
                                  newton_opts=n_opts or NewtonOptions(kappa=kappa, r_tol=3e-4, max_iter=5), device=device)
        if device_tables:
            self.solver.linearize_knots(m.name, problem.z, problem.theta, kappa)
        else:
            for t in range(problem.H):
                self.solver.set_linearization(t + 1, problem.z[t], problem.theta[t], problem.r0[t], problem.rz0[t], problem.rth0[t])
        self.solver.set_objective(obj_q, obj_u, obj_gamma, obj_b, V=obj_v, v_target=v_target)
        from .lcp_models import get_stride
        self.stride = get_stride(m, problem.q)
        self.phase0 = None if phase is None else np.asarray(phase, dtype=np.int32).reshape(B)
        self.newton_iters = []
        self.altitude_update = bool(altitude_update)
        self.altitude_impact_threshold = float(altitude_impact_threshold)
        self.gains = bool(gains)
        if self.gains:
            from .gains import reference_gains
            self.K = reference_gains(m.name, problem.z, problem.theta, np.asarray(obj_q)[0], np.asarray(obj_v)[0], np.asarray(obj_u)[0],
                                     N=gains_N, U_scaling=control_gain_scaling, V_scaling=velocity_gain_scaling)
            self.solver.set_gains(self.K)
        self.reset()

    def reset(self):
        """policy(p, traj, t = 1): set_trajectory!(p.traj, p.ref_traj), reset_window!, p.q0 = ref_traj.q[1], cnt = N_sample."""
        P = self.problem
        self.solver.set_gait(P.q, P.u, P.theta, self.stride, w=P.w, gamma=P.gamma, b=P.b, phase=self.phase0)
        ph = np.zeros(self.B, dtype=np.int64) if self.phase0 is None else self.phase0.astype(np.int64)
        self.q0 = np.stack([P.q[0] if p == 0 else P.q[(p - 1) % P.H + 1] + ((p - 1) // P.H) * self.stride for p in ph])
        self.cnt = self.N_sample
        self.solves = 0
        self.u = np.zeros((self.B, P.model.nu))
        self.altitude = np.zeros((self.B, P.model.nc))          # p.altitude .= 0.0 (policy.jl:102)
        self.gamma_hist, self.q_hist = [], []
        self.q_prev = self.q0.copy()

    def observe(self, q2, gamma):
        """The outcome of one simulator step, (B, nq) and (B, nc): the part of `traj` the altitude update reads."""
        if self.altitude_update:
            self.q_hist = (self.q_hist + [np.array(q2, dtype=np.float64).reshape(self.B, -1)])[-self.N_sample:]
            self.gamma_hist = (self.gamma_hist + [np.array(gamma, dtype=np.float64).reshape(self.B, -1)])[-self.N_sample:]

    def __call__(self, q1):
        """One simulator step: q1 = current configurations (B, nq) (`traj.q[t+1]`).  Returns the controls (B, nu)."""
        q1 = np.asarray(q1, dtype=np.float64).reshape(self.B, -1)
        if self.cnt == self.N_sample:
            if self.altitude_update:
                if self.solves > 0 and self.gamma_hist:               # steps max(0, t-1-N_sample)+1 .. t-1 (mpc_utils.jl:112)
                    g, qh = np.stack(self.gamma_hist, axis=1), np.stack(self.q_hist, axis=1)
                    for r in range(self.B):
                        update_altitude(self.problem.model, self.altitude[r], g[r], qh[r], self.altitude_impact_threshold)
                self.set_altitude(self.altitude)
            u1, it, rn = self.solver.newton_solve(self.q0, q1, warm_start=self.solves > 0)
            self.newton_iters.append(it.copy())
            if self.gains:
                self.solver.gain_latch()                    # before the reference rotates: K[window[1]], p.traj.q[1], p.traj.q[2]
            self.solver.mpc_advance(self.stride)            # rot_n_stride! + update_window!
            self.q0 = q1.copy()
            self.cnt = 0
            self.solves += 1
            self.u = u1 / self.N_sample                      # policy.jl:142-144 (:direct)
        self.cnt += 1
        if self.gains:
            u = self.solver.gain_feedback(self.q_prev, q1, self.N_sample)
            self.q_prev = q1.copy()
            return u
        return self.u

    def relinearize(self, z=None, theta=None, t0=1, terrain=None):
        """Knots t0 .. t0+N-1 linearized again in flight, at the policy's κ, on the device: the `update!` of the reference's
        RLin / RZLin / RθLin.  z (N, nz), theta (N, nθ); the defaults are the problem's own."""
        z = self.problem.z if z is None else z
        theta = self.problem.theta if theta is None else theta
        self.solver.linearize_knots(self.problem.model.name, z, theta, self.kappa, t0=t0, terrain=terrain)

    def set_altitude(self, alt):
        """`set_altitude!(p.im_traj, p.altitude)` (policy.jl:116, implicit_dynamics.jl:141-154): (B, nc) or (nc,)."""
        alt = np.broadcast_to(np.asarray(alt, dtype=np.float64), (self.B, self.problem.model.nc))
        self.solver.set_altitude(np.ascontiguousarray(alt))

    def close(self):
        self.solver.close()
