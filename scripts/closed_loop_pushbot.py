#!/usr/bin/env python3
"""examples/pushbot/push_recovery.jl (:16-98) and examples/cartpole/cartpole.jl (:15-80) with BOTH sides on the device: the MPC policy
on the model's real problem tables (the constant upright reference, `lcp_models.constant_reference`) and the device plant
(CIMPC_PLANT_PUSHBOT / CIMPC_PLANT_WALLEDCARTPOLE), pushed by the example's impulses.
  pushbot   reference H 100, h 0.04; H_mpc 40, N_sample 2, κ_mpc 1e-4, :configurationforce, the "fast recovery" TrackingVelocityObjective
            (q = 12 (t / H_mpc)² on both coordinates, v = (1, 0.01) / h², u = (100, 1), γ and b 1e-100), Newton r_tol 3e-4 / 10 iterations
            (the example's max_time = h / 2 is a wall-clock budget and is not applied), impulses (-5.5, 5.5, 5.5, -1.5, -6.5) on θ at
            simulator steps 20, 220, 300, 500, 530.
  cartpole  reference H 50, h 0.04; H_mpc 10, N_sample 2, κ_mpc 2e-4, :configurationforce, q = (1e-1, 1e-3, 1e-8, 1e-8) with the last knot
            (10, 1, 1e-8, 1e-8), v = (1, 30, 1e-8, 1e-8) with the last knot (10, 10, 1e-8, 1e-8), u = 3e-2, Newton r_tol 3e-4 / 5 iterations,
            impulses (0.2, 0.2, -0.2, 0.2, 0.2) on θ at steps 20, 220, 370, 570, 720; w has all four coordinates (A = I).
Robot 0 is the example as written; the other robots' impulses are scaled by U(0.8, 1.0) (seeded).  Prints per robot: plant convergence,
Newton iterations per solve, the largest |q| per coordinate, the lowest ϕ, the largest γ and the largest |θ| over the last 50 steps.
usage: python scripts/closed_loop_pushbot.py [--example pushbot|cartpole] [--robots 4] [--steps 1000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def example_settings(example):
    """The example's numbers: model name, reference (H, h), MPC settings, objective weights (H_mpc, n, n) and impulses."""
    tile = lambda rows: np.stack([np.diag(np.asarray(r, dtype=float)) for r in rows])
    if example == "pushbot":
        H_mpc, h = 40, 0.04
        s = [12.0 * ((t + 1) / H_mpc) ** 2 for t in range(H_mpc)]
        return dict(model="pushbot", H=100, h=h, H_mpc=H_mpc, N_sample=2, kappa=1e-4, newton_max_iter=10,
                    obj_q=tile([[a, a] for a in s]), obj_v=tile([[1.0 / h ** 2, 0.01 / h ** 2]] * H_mpc), obj_u=tile([[100.0, 1.0]] * H_mpc),
                    obj_gamma=tile([[1e-100] * 2] * H_mpc), obj_b=tile([[1e-100] * 4] * H_mpc),
                    impulse_steps=[20, 220, 300, 500, 530], impulses=[[-5.5, 0.0], [5.5, 0.0], [5.5, 0.0], [-1.5, 0.0], [-6.5, 0.0]])
    if example == "cartpole":
        H_mpc = 10
        return dict(model="walledcartpole", H=50, h=0.04, H_mpc=H_mpc, N_sample=2, kappa=2e-4, newton_max_iter=5,
                    obj_q=tile([[1e-1, 1e-3, 1e-8, 1e-8]] * (H_mpc - 1) + [[1e+1, 1e+0, 1e-8, 1e-8]]),
                    obj_v=tile([[1e-0, 3e+1, 1e-8, 1e-8]] * (H_mpc - 1) + [[1e+1, 1e+1, 1e-8, 1e-8]]), obj_u=tile([[3e-2]] * H_mpc),
                    obj_gamma=tile([[0.0] * 2] * H_mpc), obj_b=tile([[0.0] * 4] * H_mpc),
                    impulse_steps=[20, 220, 370, 570, 720],
                    impulses=[[0.2, 0, 0, 0], [0.2, 0, 0, 0], [-0.2, 0, 0, 0], [0.2, 0, 0, 0], [0.2, 0, 0, 0]])
    raise KeyError(example)


def gaps(model, q):
    """ϕ of both walls, q (..., nq) -> (..., 2) (pushbot/model.jl:87-91, walledcartpole/model.jl:101-109)."""
    if model == "pushbot":
        x = -1.0 * np.sin(q[..., 0]) + q[..., 1] * np.cos(q[..., 0])
        return np.stack([x + 0.5, 0.5 - x], -1)
    x = q[..., 1] - 0.6 * np.sin(q[..., 0])
    return np.stack([x - q[..., 2] + 0.35, 0.35 + q[..., 3] - x], -1)


def impulse_schedule(S, robots, seed=100):
    """`impulse_disturbances(impulses, idx)` for B robots: (B, nw) per impulse, robot 0 as written, the others scaled by U(0.8, 1.0)."""
    from contactimplicitmpc.jl_amd import plant
    scale = np.ones((len(S["impulses"]), robots))
    scale[:, 1:] = np.random.default_rng(seed).uniform(0.8, 1.0, (len(S["impulses"]), robots - 1))
    return plant.ImpulseDisturbance([np.asarray(w, dtype=float)[None] * scale[i][:, None] for i, w in enumerate(S["impulses"])],
                                    S["impulse_steps"])


def run(example="pushbot", robots=4, steps=1000, verbose=True):
    from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, lcp_models, plant
    from contactimplicitmpc.jl_amd.policy import CIMPCPolicy
    S = example_settings(example)
    m = lcp_models.MODELS[S["model"]]()
    P = lcp_models.reference_problem(m, lcp_models.constant_reference(m, np.zeros(m.nq), S["H"], S["h"]), S["kappa"])
    B = robots
    pol = CIMPCPolicy(P, S["obj_q"], S["obj_u"], H_mpc=S["H_mpc"], N_sample=S["N_sample"], kappa_mpc=S["kappa"], B=B, mode=1,
                      obj_gamma=S["obj_gamma"], obj_b=S["obj_b"], obj_v=S["obj_v"],
                      n_opts=NewtonOptions(kappa=S["kappa"], r_tol=3e-4, max_iter=S["newton_max_iter"]),
                      ip_opts=InteriorPointOptions(kappa_tol=S["kappa"], r_tol=1e-8))
    dist = impulse_schedule(S, B)
    h_sim = S["h"] / S["N_sample"]
    q = [np.zeros((B, m.nq)), np.zeros((B, m.nq))]                                      # q1 = 0, v1 = 0
    status, gamma = [], []
    t0 = time.perf_counter()
    for t in range(steps):
        q2, g, b, st, it = plant.plant_step(S["model"], q[t], q[t + 1], pol(q[t + 1]), m.mu_world, h_sim, w=dist(t + 1))
        status.append(st.astype(bool)); gamma.append(g); q.append(q2)
    dt = time.perf_counter() - t0
    q, status, gamma = np.array(q), np.array(status), np.array(gamma)
    iters = np.stack(pol.newton_iters)
    solves = pol.solves
    pol.close()
    phi = gaps(S["model"], q)
    out = []
    for r in range(B):
        out.append(dict(plant_converged=bool(status[:, r].all()), plant_failures=int((~status[:, r]).sum()),
                        newton_iters_max=int(iters[:, r].max()), newton_iters_mean=float(iters[:, r].mean()),
                        q_abs_max=np.abs(q[:, r]).max(axis=0).tolist(), phi_min=float(phi[2:, r].min()), gamma_max=float(gamma[:, r].max()),
                        theta_abs_max=float(np.abs(q[:, r, 0]).max()), theta_abs_last50=float(np.abs(q[-50:, r, 0]).max())))
        if verbose:
            o = out[-1]
            print("robot %d: plant converged %s (%d failures), Newton iterations per solve %.2f (max %d), max |q| %s, phi min %.2e, "
                  "gamma max %.3f, |theta| over the last 50 steps %.2e"
                  % (r, o["plant_converged"], o["plant_failures"], o["newton_iters_mean"], o["newton_iters_max"],
                     " ".join("%.4f" % v for v in o["q_abs_max"]), o["phi_min"], o["gamma_max"], o["theta_abs_last50"]))
    ok = bool(status.all())
    if verbose:
        print("%s: all plant steps converged: %s; %d plant steps, %d MPC solves of %d robots in %.2f s" % (example, ok, steps, solves, B, dt))
    return ok, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--example", choices=["pushbot", "cartpole"], default="pushbot")
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--steps", type=int, default=1000)
    a = ap.parse_args()
    run(a.example, a.robots, a.steps)
