#!/usr/bin/env python3
"""Writes tests/golden/walled_closed_loop.json: the four robots of scripts/closed_loop_pushbot.py (robot 0: the examples as written; the
others with their impulses scaled as the script scales them) run on the CPU with the reference algorithm on both sides -
oracle.plant.OraclePolicy on the model's real problem tables and the Newton solve of tests/walled_ref.py as the plant - for 400
simulator steps.  Recorded per example: the settings and, per robot, whether every plant step converged, the Newton iterations,
max |θ|, max |θ| over the last 50 steps, the lowest ϕ, the largest γ and θ at every 25th step.  tests/test_gpu_walled_models.py holds
every robot of the device loop to 1.5 x its own two |θ| figures.
usage: python tests/golden/make_walled_closed_loop.py"""
import importlib.util
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
STEPS, ROBOTS = 400, 4


def cpu_loop(example, robot=0, steps=STEPS):
    from contactimplicitmpc.jl_amd import lcp_models
    from oracle import ip as oip, lcp, newton as onewton, plant as pl
    from oracle.dims import Dims
    import walled_ref as ref
    spec = importlib.util.spec_from_file_location("closed_loop_pushbot", os.path.join(ROOT, "scripts", "closed_loop_pushbot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    S = mod.example_settings(example)
    m = lcp_models.MODELS[S["model"]]()
    P = lcp_models.reference_problem(m, lcp_models.constant_reference(m, np.zeros(m.nq), S["H"], S["h"]), S["kappa"])
    d = Dims(nq=m.nq, nu=m.nu, nw=m.nw, nc=m.nc, nb=m.nb, mode=1)
    tabs = [lcp.LinTable(d, P.z[t], P.theta[t], P.r0[t], P.rz0[t], P.rth0[t]) for t in range(P.H)]
    traj = onewton.Traj(q=P.q.copy(), u=P.u.copy(), w=P.w.copy(), gamma=P.gamma.copy(), b=P.b.copy(), theta=P.theta.copy())
    obj = onewton.Objective(q=S["obj_q"], u=S["obj_u"], gamma=S["obj_gamma"], b=S["obj_b"], v=S["obj_v"])
    pol = pl.OraclePolicy(d, tabs, traj, lcp_models.get_stride(m, P.q), obj, S["H_mpc"], S["N_sample"], S["kappa"],
                          onewton.NewtonOptions(r_tol=3e-4, max_iter=S["newton_max_iter"], solver="lu"),
                          oip.IPOptions(kappa_tol=S["kappa"], r_tol=1e-8))
    plant = ref.PLANTS[S["model"]]()
    h_sim = S["h"] / S["N_sample"]
    dist = mod.impulse_schedule(S, ROBOTS)                                             # (ROBOTS, nw) per step; this robot's row
    q, ok, gmax = [np.zeros(m.nq), np.zeros(m.nq)], True, 0.0
    for t in range(steps):
        u = pol(q, t)
        w = dist(t + 1)[robot]
        st, _, q2, gam, _ = pl.plant_step(plant, q[t], q[t + 1], u, w, plant.mu_world, h_sim, pl.SIM_OPTS)
        ok = ok and st
        gmax = max(gmax, float(gam.max()))
        q.append(q2)
    q = np.array(q)
    return dict(robot=robot, plant_converged=bool(ok), newton_iters_max=int(max(pol.iters)),
                newton_iters_mean=float(np.mean(pol.iters)), theta_abs_max=float(np.abs(q[:, 0]).max()),
                theta_abs_last50=float(np.abs(q[-50:, 0]).max()), q_abs_max=np.abs(q).max(axis=0).tolist(),
                phi_min=float(mod.gaps(S["model"], q)[2:].min()), gamma_max=gmax, theta_every_25_steps=[float(v) for v in q[1::25, 0]])


if __name__ == "__main__":
    spec = importlib.util.spec_from_file_location("closed_loop_pushbot", os.path.join(ROOT, "scripts", "closed_loop_pushbot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    jobs = [(ex, r) for ex in ("pushbot", "cartpole") for r in range(ROBOTS)]
    with multiprocessing.Pool(len(jobs)) as pool:
        res = pool.starmap(cpu_loop, jobs)
    keys = ("model", "H", "h", "H_mpc", "N_sample", "kappa", "newton_max_iter", "impulse_steps", "impulses")
    out = {ex: dict(settings={k: mod.example_settings(ex)[k] for k in keys}, steps=STEPS, robots=[o for (e, _), o in zip(jobs, res) if e == ex])
           for ex in ("pushbot", "cartpole")}
    for (ex, r), o in zip(jobs, res):
        print(ex, {k: v for k, v in o.items() if k != "theta_every_25_steps"})
    with open(os.path.join(HERE, "walled_closed_loop.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
