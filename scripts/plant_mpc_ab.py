#!/usr/bin/env python3
"""What a control step of iLQR-MPC costs with the plan and the problem resident on the device (`plant.ILQRPolicy.control`,
`cimpc_plant_mpc_control`) against the composition it is held to - `plant.ilqr(device_loop=True)` on the step's
goal window, which uploads the problem and the first nominal and downloads every T x B array at every step - in ONE process:

  the three hoppers of `plant_gradient_cases.rollout_case("hopper_2D")` (B 3, H 14, the contact cost, three step lengths), n_iter 1 and 2, and
  centroidal_quadruped B 64, H 60 (the leg of scripts/plant_ilqr_ab.py, its cost, four step lengths), n_iter 1.

Both sides run a FIXED number of iterations (tol = 0, rho_max = inf) from the SAME state and the SAME plan at every call: the policy's plan is
loaded again (`reset`) before each control step, INSIDE the clock - an upload of H x B x nu doubles that a policy in use does not pay, so
its figure is an upper bound.  Timed per turn, alternating: (a) the composition and (a') its twin, so that the A/A spread of the session is
on record, (b) the policy; a sample is `reps` calls back to back (20 for the hoppers, 1 for centroidal), reported per call.  A warm call
each, a host clock around whole calls (each ends in a stream synchronize); medians, minima and maxima over `--turns` turns.  The two results
are compared bit for bit before anything is timed.  that cross the bus per control step are counted from the two paths' argument lists, not measured.  Recorded, not asserted.
usage: python scripts/plant_mpc_ab.py [--turns 7] [--skip-centroidal] [--out profiles/plant_mpc.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from contactimplicitmpc.jl_amd import plant  # noqa: E402
from plant_gradients_ab import summary  # noqa: E402
import plant_ilqr_ab  # noqa: E402


def bus_bytes(model, B, H, n_iter, n_alpha, n_x, n_Q, n_R, limited):
    """(policy, composition) bytes per control step, up and down, from the argument lists of the entries each path calls."""
    mid, nq, nu, nc, fd, nw = plant.model_dims(model)
    nb, n, TB = fd * nc, 2 * nq, H * B
    D, I = 8, 4
    pol_up = 2 * B * nq * D
    pol_down = B * nu * D + B * D + n_iter * B * (3 * D + I) + B * I + n_iter * I
    traj = (H + 2) * B * nq * D + TB * nu * D + TB * nc * D + TB * nb * D + 2 * TB * I      # q, u, gamma, b, status, iters
    lin = (H + 1) * B * n * D + TB * nu * D
    # cimpc_plant_rollout_tape, then cimpc_plant_ilqr
    comp_up = 2 * B * nq * D + TB * nu * D                                                     # the rollout's start rows and controls
    comp_down = traj - TB * nu * D + TB * I                                                    # its trajectory and the tape's status
    comp_up += traj + lin + B * D                                                              # the first nominal with its cost
    comp_up += (n_Q * n * n + n * n + n_R * nu * nu) * D + ((H + 1) * n_x * n + H * n_x * nu) * D + (n_alpha + n_iter + 1) * D
    comp_down += traj + lin + TB * I + n_iter * B * (3 * D + I) + n_iter * I                   # the final nominal, the history, the per-iteration int
    comp_down += TB * nu * n * D + TB * nu * D + 2 * B * D + 2 * B * I + (TB * I if limited else 0)      # K, k, dV, lq_status, n_cut, clamped
    return {"policy": {"up": pol_up, "down": pol_down}, "composition": {"up": comp_up, "down": comp_down}}


def case(name, model, args, cost, kw, n_iter, turns, reps):
    model, q1, v1, u, h, mu = args
    B, H = np.atleast_2d(q1).shape[0], u.shape[0]
    kw = dict(kw, tol=0.0, rho_max=np.inf)
    ref = plant.TrackingReference(cost.Q, cost.R, cost.Qf, x_ref=cost.x_goal if cost.x_goal.ndim == 2 or cost.x_goal.shape[1] > 1 else cost.x_goal[:, 0],
                                  u_ref=cost.u_goal if cost.u_goal.ndim == 2 or cost.u_goal.shape[1] > 1 else cost.u_goal[:, 0])
    u0 = np.broadcast_to(u if u.ndim == 3 else u[:, None], (H, B, u.shape[-1])).copy()

    def composition():
        res = plant.ilqr(model, q1, v1, u0, h, mu, ref.window(0, H), max_iter=n_iter, device_loop=True, **kw)
        res.tape.close()
        return res

    with plant.ILQRPolicy(model, B, H, h, mu, ref, u0, n_iter=n_iter, **kw) as pol:
        def policy():
            pol.reset(u0)                                                # the same plan at every call
            return pol.control(q1, v1, shift=0)
        res, up = composition(), policy()                                # warm-up, and the comparison
        same = bool(np.array_equal(up, res.u[0]) and np.array_equal(pol.plan()[0], res.u) and np.array_equal(pol.plan()[1], res.q) and
                    np.array_equal(pol.last.J, res.J) and np.array_equal(pol.last.J0, res.J0))
        assert pol.last.n_done == res.J.shape[0] == n_iter, "a loop ended early: the iteration count is not fixed"
        runs = {"a_composition": composition, "a_twin": composition, "b_policy": policy}
        times = {k: [] for k in runs}
        for _ in range(turns):
            for k, f in runs.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                times[k].append((time.perf_counter() - t0) * 1e3 / reps)
        x = ref._arrays(B)[0]
    out = {"case": name, "model": model, "B": B, "H": H, "n_iter": n_iter, "calls_per_sample": reps, "alphas": list(kw["alphas"]), "policy_equals_composition_bit_for_bit": same,
           "ms_per_control_step": {k: summary(v) for k, v in times.items()},
           "bytes_per_control_step": bus_bytes(model, B, H, n_iter, len(kw["alphas"]), x.shape[1], 1 if cost.Q.ndim == 2 else H, 1 if cost.R.ndim == 2 else H, False)}
    med = lambda k: out["ms_per_control_step"][k]["median_ms"]
    out["twin_over_composition"] = round(med("a_twin") / med("a_composition"), 4)
    out["policy_over_composition"] = round(med("b_policy") / med("a_composition"), 4)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=7)
    ap.add_argument("--skip-centroidal", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_mpc.json"))
    a = ap.parse_args()
    assert a.turns >= 3, "medians of at least 3 turns"
    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    hop = plant_ilqr_ab.hoppers()
    cases = [case(hop["name"], hop["model"], hop["args"], hop["cost"], hop["kw"], n_iter, a.turns, 20) for n_iter in (1, 2)]
    if not a.skip_centroidal:
        cen = plant_ilqr_ab.centroidal()
        cases.append(case(cen["name"], cen["model"], cen["args"], cen["cost"], cen["kw"], 1, a.turns, 1))
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "cases": cases,
           "method": "alternating turns, a warm call each, host clock around whole calls, medians; the composition's twin gives the session's A/A spread"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
