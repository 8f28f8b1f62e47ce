#!/usr/bin/env python3
"""Closed loop on terrain (examples/quadruped/sine.jl, examples/quadruped/piecewise.jl in spirit): B quadrupeds run gait2 with
the flat controller (H_mpc 10, N_sample 5, κ_mpc 1e-4, altitude_update with threshold 0.05) while the device plant steps them
on `--terrain` (a name of contactimplicitmpc/jl_amd/terrain.py).  Initial joint offsets U(-perturb, perturb) per robot.
Prints progress, the robots that fell (body below --fall-height above the terrain, or torso 0.5 rad off the gait's angle),
plant convergence and the time split between policy and plant."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import synth  # noqa: E402  (the objective constants only)
from real_problems import real_problem  # noqa: E402
from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, plant, terrain  # noqa: E402
from contactimplicitmpc.jl_amd.policy import CIMPCPolicy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--terrain", default="sine1_2D_lc")
ap.add_argument("--robots", type=int, default=4)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--perturb", type=float, default=0.0)
ap.add_argument("--kappa", type=float, default=1e-4)
ap.add_argument("--threshold", type=float, default=0.05)
ap.add_argument("--no-altitude", action="store_true")
ap.add_argument("--fall-height", type=float, default=0.15)
a = ap.parse_args()
H_MPC, N_SAMPLE = 10, 5
ter = terrain.get(a.terrain)
d, P, prob, tabs = real_problem("quadruped", a.kappa, True)
obj = synth.make_objective(d, H_MPC, kind="quadruped")
B = a.robots
pol = CIMPCPolicy(P, obj.q, obj.u, H_mpc=H_MPC, N_sample=N_SAMPLE, kappa_mpc=a.kappa, B=B,
                  n_opts=NewtonOptions(kappa=a.kappa, r_tol=3e-4, max_iter=5), ip_opts=InteriorPointOptions(kappa_tol=a.kappa, r_tol=1e-8),
                  altitude_update=not a.no_altitude, altitude_impact_threshold=a.threshold)
rng = np.random.default_rng(100)
q1 = np.tile(P.q[1], (B, 1)); v1 = np.tile((P.q[1] - P.q[0]) / P.h, (B, 1))
q1[:, 3:] += rng.uniform(-a.perturb, a.perturb, (B, d.nq - 3))
q1[:, 1] += ter.surface(q1[:, 0])                       # start on the terrain under the hip
t_pol = [0.0]
def policy(q):
    t0 = time.perf_counter(); u = pol(q); t_pol[0] += time.perf_counter() - t0
    return u
policy.observe = pol.observe                           # the plant hands each step's (q2, gamma) to the altitude update
t0 = time.perf_counter()
ok, q, u, g, b = plant.simulate("quadruped", policy, q1, v1, a.steps, P.h / N_SAMPLE, mu=1.0, terrain=ter)
wall = time.perf_counter() - t0
pol.close()
clearance = q[:, :, 1] - ter.surface(q[:, :, 0])         # body height above the terrain under the hip
pitch = np.abs(q[:, :, 2] - P.q[0][2])                   # torso angle off the gait's
fell = (clearance.min(axis=0) < a.fall_height) | (pitch.max(axis=0) > 0.5)
print("terrain %s, robots %d, plant steps %d, MPC solves %d, altitude update %s: all plant steps converged: %s"
      % (a.terrain, B, a.steps, pol.solves, not a.no_altitude, ok))
print("wall %.2f s: policy %.2f s, plant + host glue %.2f s" % (wall, t_pol[0], wall - t_pol[0]))
print("progress in x (m): min %.4f  mean %.4f  max %.4f" % tuple(f((q[-1, :, 0] - q[1, :, 0])) for f in (np.min, np.mean, np.max)))
print("min body clearance %.4f m, max |pitch| %.4f rad, fell: %d of %d" % (clearance.min(), pitch.max(), int(fell.sum()), B))
print("final altitudes (robot 0):", np.array2string(pol.altitude[0], precision=4))
