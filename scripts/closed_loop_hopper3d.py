#!/usr/bin/env python3
"""examples/hopper/3D_flat.jl and 3D_sine.jl (:32-81) with BOTH sides on the device: the MPC policy on the flat hopper_3D model
(gait_forward.jld2, :configuration mode, H_mpc 20, N_sample 10, κ_mpc 1e-4, Q = 0.1 diag(3, 3, 0.1, 50, 50, 50, 10),
R = diag(0.1, 0.1, 10), Newton r_tol 3e-4 / 5 iterations, interior point 1e-4 / 1e-4, altitude update with impact threshold 0.05)
and the device plant (CIMPC_PLANT_HOPPER_3D) on flat ground or on sine2_3D_lc, for B robots whose start is offset in (x, y) by
U(-perturb, perturb) (robot 0: none).  Prints per robot: plant convergence, Newton iterations and residual norm, the tracking
error of q (trajectory.jl:186-220), the lowest ϕ, the largest |p| and the lowest height of the body above its foot.
usage: python scripts/closed_loop_hopper3d.py [--terrain flat|sine2] [--robots 4] [--steps 300] [--perturb 0.01]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, gait_io, lcp_models, plant, terrain  # noqa: E402
from contactimplicitmpc.jl_amd.policy import CIMPCPolicy  # noqa: E402

TERRAINS = {"flat": "flat_3D_lc", "sine2": "sine2_3D_lc"}
H_MPC, N_SAMPLE, KAPPA = 20, 10, 1e-4


def foot(q):
    """k = pos - R(p) e_3 r (hopper_3D/model.jl:33-37), q (..., 7) -> (..., 3)."""
    p, r = q[..., 3:6], q[..., 6:7]
    n = np.sum(p * p, axis=-1, keepdims=True)
    N = np.stack([8.0 * p[..., 0] * p[..., 2] + 4.0 * (1.0 - n[..., 0]) * p[..., 1],
                  8.0 * p[..., 1] * p[..., 2] - 4.0 * (1.0 - n[..., 0]) * p[..., 0],
                  -8.0 * (p[..., 0] ** 2 + p[..., 1] ** 2)], axis=-1)
    a = N / (1.0 + n) ** 2
    a[..., 2] += 1.0
    return q[..., 0:3] - a * r


def run(terrain_name="flat", robots=4, steps=300, perturb=0.01, verbose=True):
    m = lcp_models.Hopper3D()
    traj = gait_io.load_joint_traj(os.path.join(ROOT, "tests", "golden", "gaits", "hopper_3D_gait_forward.jld2"))
    P = lcp_models.reference_problem_from_traj(m, traj, KAPPA)
    ter = terrain.get(TERRAINS[terrain_name])
    B = robots
    tile = lambda M: np.tile(np.asarray(M, dtype=float)[None], (H_MPC, 1, 1))
    obj_q = tile(np.diag(0.1 * np.array([3.0, 3.0, 0.1, 50.0, 50.0, 50.0, 10.0])))
    obj_u = tile(np.diag([0.1, 0.1, 10.0]))
    pol = CIMPCPolicy(P, obj_q, obj_u, H_mpc=H_MPC, N_sample=N_SAMPLE, kappa_mpc=KAPPA, B=B, mode=0,
                      n_opts=NewtonOptions(kappa=KAPPA, r_tol=3e-4, max_iter=5),
                      ip_opts=InteriorPointOptions(kappa_tol=KAPPA, r_tol=1e-4),
                      altitude_update=True, altitude_impact_threshold=0.05)
    rnorm = []                                                                          # each solve's final Newton residual norm
    solve = pol.solver.newton_solve
    def recording(*a, **k):
        u1, it, rn = solve(*a, **k)
        rnorm.append(np.array(rn, dtype=float))
        return u1, it, rn
    pol.solver.newton_solve = recording
    h_sim = P.h / N_SAMPLE
    rng = np.random.default_rng(100)
    q1 = np.tile(P.q[1], (B, 1)); v1 = np.tile((P.q[1] - P.q[0]) / P.h, (B, 1))
    q1[1:, 0:2] += rng.uniform(-perturb, perturb, (B - 1, 2))
    k1 = foot(q1)
    q1[:, 2] += ter.surface(k1[:, 0], k1[:, 1])                                        # start on the terrain under the foot
    # the loop of plant.simulate, keeping every step's status per robot
    status = []
    t0 = time.perf_counter()
    q = [q1 - h_sim * v1, q1.copy()]
    for t in range(steps):
        q2, g, b, st, it = plant.plant_step("hopper_3D", q[t], q[t + 1], pol(q[t + 1]), m.mu_world, h_sim, terrain=ter)
        status.append(st.astype(bool))
        pol.observe(q2, g)                                                              # the altitude update reads (q2, gamma)
        q.append(q2)
    dt = time.perf_counter() - t0
    q, status = np.array(q), np.array(status)
    iters, rnorm = np.stack(pol.newton_iters), np.stack(rnorm)
    solves = pol.solves
    pol.close()
    k = foot(q)
    phi = k[..., 2] - ter.surface(k[..., 0], k[..., 1])
    stride = lcp_models.get_stride(m, P.q)
    out = []
    for r in range(B):
        # tracking_error of q (trajectory.jl:186-220) against the repeated gait, the robot's own start offset taken out
        err, cnt = 0.0, 0
        for t in range((steps - 1) // N_SAMPLE + 1):
            rep, kn = divmod(t, P.H)
            err += np.abs(P.q[kn + 2] + rep * stride - (q[t * N_SAMPLE + 2, r] - (q[1, r] - P.q[1]))).sum() / m.nq
            cnt += 1
        out.append(dict(plant_converged=bool(status[:, r].all()), plant_failures=int((~status[:, r]).sum()),
                        newton_iters_max=int(iters[:, r].max()), newton_iters_mean=float(iters[:, r].mean()),
                        newton_rnorm_max=float(rnorm[:, r].max()), q_tracking_error=float(err / cnt),
                        phi_min=float(phi[1:, r].min()), mrp_norm_max=float(np.linalg.norm(q[:, r, 3:6], axis=-1).max()),
                        body_above_foot_min=float((q[:, r, 2] - k[:, r, 2]).min()), progress_xy=(q[-1, r, 0:2] - q[1, r, 0:2]).tolist()))
        if verbose:
            o = out[-1]
            print("robot %d: plant converged %s (%d failures), Newton iterations per solve %.2f (max %d), residual norm max %.2e, "
                  "q tracking error %.4f, phi min %.2e, |p| max %.4f, body above foot min %.4f m, progress (x, y) (%.4f, %.4f)"
                  % (r, o["plant_converged"], o["plant_failures"], o["newton_iters_mean"], o["newton_iters_max"], o["newton_rnorm_max"],
                     o["q_tracking_error"], o["phi_min"], o["mrp_norm_max"], o["body_above_foot_min"], *o["progress_xy"]))
    ok = bool(status.all())
    if verbose:
        print("terrain %s: all plant steps converged: %s; %d plant steps, %d MPC solves of %d robots in %.2f s"
              % (TERRAINS[terrain_name], ok, steps, solves, B, dt))
    return ok, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--terrain", choices=sorted(TERRAINS), default="flat")
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--perturb", type=float, default=0.01)
    a = ap.parse_args()
    run(a.terrain, a.robots, a.steps, a.perturb)
