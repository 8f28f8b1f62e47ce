#!/usr/bin/env python3
"""The closed-loop rollout end to end: hopper_3D on its shipped in-place gait, the reference's time-varying LQR gains along it
(`gains.reference_gains`) as a `plant.Feedback` (`gains.gait_feedback`), and B robots under random pushes simulated over one gait
cycle in ONE device call - once under u = ū + K (x_ref − x) and once with K = 0 (the open-loop replay under the same pushes).
Reported: the share of robots whose body position stays within `--bound` metres of the gait's at every step, for both, and the mean
largest deviation.  The weights are those of tests/gains_cases.hopper_weights (no hopper example of the reference turns its gains on).
Recorded into profiles/plant_feedback.json under "closed_loop_gains_rollout"; nothing is asserted.
usage: python scripts/closed_loop_gains_rollout.py [--robots 256] [--push 0.02] [--bound 0.05] [--out profiles/plant_feedback.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contactimplicitmpc.jl_amd import gains, gait_io, plant  # noqa: E402

MU = 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--push", type=float, default=0.02, help="largest impulse of a push, per axis (N s)")
    ap.add_argument("--bound", type=float, default=0.05, help="tracking bound on the body position (m)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_feedback.json"))
    a = ap.parse_args()
    t = gait_io.load_joint_traj(os.path.join(ROOT, "tests", "golden", "gaits", "hopper_3D_gait_in_place.jld2"))
    B, T, nw = a.robots, t.H, 3
    weights = np.diag([1.0, 1.0, 1.0, 0.3, 0.3, 0.3, 0.1]), np.diag(1e-3 * np.ones(7)), np.diag([1e-2, 1e-2, 1e-1])
    K = gains.reference_gains("hopper_3D", t.z, t.theta, *weights, N=3)
    fb = gains.gait_feedback(t.q, K, N_sample=1)
    w = np.random.default_rng(a.seed).uniform(-a.push, a.push, (T, B, nw))      # a push at every step, each robot its own
    q1, v1 = np.tile(t.q[1], (B, 1)), np.tile((t.q[1] - t.q[0]) / t.h, (B, 1))
    out = {}
    for name, feedback in (("with_K", fb), ("K_zero", plant.Feedback(np.zeros(K.shape), fb.x_ref, hold=fb.hold))):
        t0 = time.perf_counter()
        ok, q, ua, gam, b, st, it, e = plant.rollout("hopper_3D", q1, v1, t.u, t.h, MU, w=w, feedback=feedback)
        ms = (time.perf_counter() - t0) * 1e3
        dev = np.abs(q[:, :, :3] - t.q[:T + 2, None, :3]).max(axis=(0, 2))      # per robot: largest body-position error over the cycle
        out[name] = {"share_within_bound": float((dev <= a.bound).mean()), "mean_largest_deviation_m": float(dev.mean()),
                     "steps_converged": float(st.mean()), "max_abs_feedback_control": float(np.abs(ua - t.u[:, None]).max()), "call_ms": round(ms, 1)}
        print(name, json.dumps(out[name]), flush=True)
    rec = {"model": "hopper_3D", "gait": "hopper_3D_gait_in_place", "robots": B, "steps": T, "push": a.push, "bound_m": a.bound, "seed": a.seed,
           "date": time.strftime("%Y-%m-%d"), "command": "python scripts/closed_loop_gains_rollout.py " + " ".join(sys.argv[1:]), **out}
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    old["closed_loop_gains_rollout"] = rec
    with open(a.out, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
