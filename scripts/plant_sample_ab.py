#!/usr/bin/env python3
"""What a control step of the sampling policy costs with the plan and the problem resident on the device (`plant.SamplingPolicy.control`,
`cimpc_plant_sampler_control`) against (a) the composition it is held to, built from the pieces that exist
without it (`plant_sample_cases.compose`: N B H nu candidate controls formed in NumPy and sent up, ONE `plant.rollout` of N B robots, the
(H + 2) N B nq trajectory pulled down, `TrackingCost.evaluate`, the choice and the update on the host) and (r) ONE open-loop `plant.rollout`
of the B robots, in ONE process:

  the three hoppers of `plant_gradient_cases.rollout_case("hopper_2D")` (B 3, H 14, the contact cost), N 4 and 16, and
  centroidal_quadruped B 64, H 60 (the leg of scripts/plant_ilqr_ab.py, its cost), N 4 and 8; n_iter 1, lam 0 throughout.

Expectation, stated before measuring: the line search's figures (2, 4 and 8 step lengths at 1.013, 1.021 and 1.057 x one closed-loop rollout
on centroidal B 64, T 60, its three kernels beside the step kernel 0.4 to 0.6 ms) predict about 1.02 to 1.06 x one rollout on centroidal at
N 4 to 8, and a composition that pays the host's NumPy and the transfers on top.

The policy's plan is loaded again (`reset`) before each control step, INSIDE the clock.  Timed per turn, alternating: the composition and its
twin (the session's A/A spread), the policy, the B-robot rollout; a sample is `reps` calls back to back, reported per call.  A warm call each,
a host clock around whole calls; medians, minima and maxima over `--turns` turns.  The results are compared bit for bit before anything is
timed.  The bytes that cross the bus per control step are counted from the argument lists, not measured.  Recorded, not asserted.
usage: python scripts/plant_sample_ab.py [--turns 7] [--skip-centroidal] [--out profiles/plant_sample.json]"""
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
import plant_sample_cases as psc  # noqa: E402


def bus_bytes(model, B, H, N, n_iter):
    """(policy, composition) bytes per control step, up and down, from the argument lists of the entries each path calls."""
    mid, nq, nu, nc, fd, nw = plant.model_dims(model)
    nb, NB, D, I = fd * nc, N * B, 8, 4
    pol = {"up": 2 * B * nq * D, "down": B * nu * D + B * D + n_iter * B * (2 * D + 2 * I) + 2 * n_iter * NB * D + B * I}
    roll_up = 2 * NB * nq * D + H * NB * nu * D + NB * D      # q0, q1, the controls and mu tiled
    roll_down = (H + 2) * NB * nq * D + H * NB * (nc + nb) * D + 2 * H * NB * I
    return {"policy": pol, "composition": {"up": n_iter * roll_up, "down": n_iter * roll_down}}


def case(name, args, cost, N, turns, reps, seed=3):
    model, q1, v1, u, h, mu = args
    q1, v1 = np.atleast_2d(q1), np.atleast_2d(v1)
    B, H, nu = q1.shape[0], u.shape[0], u.shape[-1]
    squeeze = lambda a: a if a.ndim == 2 or a.shape[1] > 1 else a[:, 0]
    ref = plant.TrackingReference(cost.Q, cost.R, cost.Qf, x_ref=squeeze(cost.x_goal), u_ref=squeeze(cost.u_goal))
    u0 = np.broadcast_to(u if u.ndim == 3 else u[:, None], (H, B, nu)).copy()
    sigma = np.full(nu, 0.1 * np.abs(u0).max())

    def composition():
        return psc.compose(plant, model, q1, v1, u0, h, mu, ref, 0, H, N, sigma, seed=seed)

    def rollout():
        return plant.rollout(model, q1, v1, u0, h, mu)

    with plant.SamplingPolicy(model, B, H, h, mu, ref, u0, n_samples=N, sigma=sigma, seed=seed) as pol:
        def policy():
            pol.reset(u0)                                                # the same plan at every call
            return pol.control(q1, v1, shift=0)
        comp, up = composition(), policy()                               # warm-up, and the comparison
        rollout()
        same = bool(np.array_equal(up, comp["u"]) and np.array_equal(pol.plan()[0], comp["plan"]) and np.array_equal(pol.plan()[1], comp["traj"][0]) and
                    np.array_equal(pol.last.J, comp["J"], equal_nan=True) and np.array_equal(pol.last.choice, comp["choice"]))
        runs = {"a_composition": composition, "a_twin": composition, "b_policy": policy, "r_rollout_of_B": rollout}
        times = {k: [] for k in runs}
        for _ in range(turns):
            for k, f in runs.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                times[k].append((time.perf_counter() - t0) * 1e3 / reps)
        n_el = pol.last.n_eligible.tolist()
    out = {"case": name, "model": model, "B": B, "H": H, "N": N, "n_iter": 1, "lam": 0.0, "calls_per_sample": reps, "policy_equals_composition_bit_for_bit": same,
           "n_eligible": n_el, "ms_per_control_step": {k: summary(v) for k, v in times.items()}, "bytes_per_control_step": bus_bytes(model, B, H, N, 1)}
    med = lambda k: out["ms_per_control_step"][k]["median_ms"]
    out["twin_over_composition"] = round(med("a_twin") / med("a_composition"), 4)
    out["policy_over_composition"] = round(med("b_policy") / med("a_composition"), 4)
    out["policy_over_one_rollout_of_B"] = round(med("b_policy") / med("r_rollout_of_B"), 4)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=7)
    ap.add_argument("--skip-centroidal", action="store_true")
    ap.add_argument("--only", default=None, help="hoppers or centroidal: one leg, as for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_sample.json"))
    a = ap.parse_args()
    assert a.turns >= 3, "medians of at least 3 turns"
    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    cases = []
    if a.only in (None, "hoppers"):
        hop = plant_ilqr_ab.hoppers()
        cases += [case(hop["name"], hop["args"], hop["cost"], N, a.turns, 20) for N in (4, 16)]
    if a.only in (None, "centroidal") and not a.skip_centroidal:
        cen = plant_ilqr_ab.centroidal()
        cases += [case(cen["name"], cen["args"], cen["cost"], N, a.turns, 1) for N in (4, 8)]
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "cases": cases,
           "method": "alternating turns, a warm call each, host clock around whole calls, medians; the composition's twin gives the session's A/A spread"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
