#!/usr/bin/env python3
"""examples/centroidal_quadruped/continuous_wall.jl with BOTH sides on the device: the MPC policy on the wall model
(:configuration mode, H_mpc = 5, N_sample = 5, κ_mpc 2e-4, TrackingVelocityObjective of :41-51, IP r_tol 1e-4 / undercut 5,
Newton r_tol 3e-5 / max_iter 5) and the device wall plant (CIMPC_PLANT_CENTROIDAL_WALL), for B robots that carry different
payloads (a constant body force the controller does not know about).  The example's `gains = true` is off by default - the discrete
CIMPCPolicy acts alone; `--gains` adds the time-varying LQR feedback of `reference_gains` to every control (CIMPCPolicy(gains=True):
the feedback line of the example's continuous-time policy placed in the discrete one).  Prints per robot: body height / orientation drift against the
gait, the front-left foot's x and wall force over the stand, Newton iterations per solve.
usage: python scripts/closed_loop_wall.py [--steps 250] [--payload 0 -5 -10 -20] [--gains]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, gait_io, lcp_models, plant  # noqa: E402
from contactimplicitmpc.jl_amd.policy import CIMPCPolicy  # noqa: E402


def run(steps=250, payload=(0.0, -5.0, -10.0, -20.0), H_mpc=5, N_sample=5, verbose=True, gains=False):
    kappa = 2e-4
    m = lcp_models.CentroidalQuadrupedWall()
    gait = gait_io.load_gait(os.path.join(ROOT, "tests", "golden", "gaits", "wall_stand_FL_4.jld2"))
    P = lcp_models.reference_problem(m, gait, kappa)
    B = len(payload)
    tile = lambda M: np.tile(np.asarray(M, dtype=float)[None], (H_mpc, 1, 1))
    obj_q = tile(lcp_models.relative_state_cost(1.0 * np.array([1e-2, 1e-2, 1.0]), 0.3 * np.ones(3), 1.0 * np.array([0.1, 0.1, 1.0])))
    obj_u = tile(np.diag(3e-3 * np.ones(12)))
    obj_v = tile(np.diag(1e-3 * np.concatenate([np.ones(3), 1e3 * np.ones(3), np.ones(12)])))
    pol = CIMPCPolicy(P, obj_q, obj_u, H_mpc=H_mpc, N_sample=N_sample, B=B, mode=0, obj_v=obj_v, v_target=np.zeros((H_mpc, 18)),
                      n_opts=NewtonOptions(kappa=kappa, r_tol=3e-5, max_iter=5),
                      ip_opts=InteriorPointOptions(kappa_tol=kappa, r_tol=1e-4, undercut=5.0), gains=gains)
    rnorm = []                                                                          # each solve's final Newton residual norm
    solve = pol.solver.newton_solve
    def recording(*a, **k):
        u1, it, rn = solve(*a, **k)
        rnorm.append(np.array(rn, dtype=float))
        return u1, it, rn
    pol.solver.newton_solve = recording
    h_sim = P.h / N_sample
    w = np.zeros((B, 3)); w[:, 2] = np.asarray(payload) * h_sim                      # impulse per simulator step
    q1 = np.tile(P.q[1], (B, 1)); v1 = np.tile((P.q[1] - P.q[0]) / P.h, (B, 1))
    t0 = time.perf_counter()
    ok, q, u, g, b = plant.simulate("centroidal_quadruped_wall", pol, q1, v1, steps, h_sim, mu=m.mu_world, disturbances=lambda t: w)
    dt = time.perf_counter() - t0
    iters, rnorm = np.stack(pol.newton_iters), np.stack(rnorm)
    solves = pol.solves
    pol.close()
    # simulator step t (0-based) applies gait knot t // N_sample; the gait has the front-left foot at the wall (x = 0.25) from
    # knot 31 on
    on_wall = np.arange(steps) // N_sample >= 31
    out = []
    for r in range(B):
        dz = q[2:, r, 2] - P.q[np.minimum(np.arange(steps) // N_sample + 2, gait.H + 1), 2]
        out.append(dict(payload_N=float(payload[r]), controls_finite=bool(np.isfinite(u[:, r]).all()), height_drift_max=float(np.abs(dz).max()),
                        orientation_max=float(np.abs(q[:, r, 3:6]).max()), fl_x_max=float(q[:, r, 6].max()),
                        fl_wall_gamma_min_on_wall=float(g[on_wall, r, 4].min()) if on_wall.any() else float("nan"),
                        fl_wall_gamma_max=float(g[:, r, 4].max()), fl_wall_gamma_max_on_wall=float(g[on_wall, r, 4].max()) if on_wall.any() else float("nan"), newton_iters_mean=float(iters[:, r].mean()),
                        newton_iters_max=int(iters[:, r].max()), newton_rnorm_max=float(rnorm[:, r].max())))
        if verbose:
            o = out[-1]
            print("robot %d payload %+6.1f N: height drift max %.4f m, |orientation| max %.4f rad, FL foot x max %.4f, FL wall gamma "
                  "min / max on wall %.3e / %.3e, max %.3e, Newton iterations per solve %.2f (max %d), residual norm max %.2e"
                  % (r, payload[r], o["height_drift_max"], o["orientation_max"], o["fl_x_max"], o["fl_wall_gamma_min_on_wall"],
                     o["fl_wall_gamma_max_on_wall"], o["fl_wall_gamma_max"], o["newton_iters_mean"], o["newton_iters_max"], o["newton_rnorm_max"]))
    if verbose:
        print("all plant steps converged: %s; %d plant steps, %d MPC solves of %d robots in %.2f s" % (ok, steps, solves, B, dt))
    return ok, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--payload", type=float, nargs="*", default=[0.0, -5.0, -10.0, -20.0])
    ap.add_argument("--gains", action="store_true", help="add the reference_gains feedback to every control")
    a = ap.parse_args()
    run(a.steps, tuple(a.payload), gains=a.gains)
