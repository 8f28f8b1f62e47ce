#!/usr/bin/env python3
"""What a parallel line search costs, on the two legs of scripts/plant_gradients_ab.py (quadruped B 256 T 100, centroidal_quadruped B 64
T 60), in ONE process:

  (a) `rollout_tape(feedback=gains.feedback(q))` on B robots at the first step length: the path that exists without the line search;
      timed twice per turn (a and its twin), so that the A/A spread of the session is on record;
  (b) `RolloutTape.linesearch` with the first n_alpha = 1, 2, 4, 8 of the step lengths 1, 1/2, 1/4, ... - and, because a step length's
      work differs (a candidate that leaves the basin of its steps runs them to max_iter), with n_alpha = 4, 8 COPIES of the first step
      length: every robot's work n_alpha times over, which leaves the occupancy alone to show;
  (c) n_alpha = 4 sequential runs of (a), one per step length;
  (d) one `plant.ilqr` iteration (n_alpha = 4), split into its first rollout, `lqr`, `linesearch` and the host's rest.

One GPU, one process, a warm call each, then alternating turns, a host clock around whole calls (each ends in a stream synchronize);
medians, minima and maxima over `--turns` turns.  Recorded, not asserted.  `--one` runs a single n_alpha = 4 line search per leg and
exits: the run to put under a kernel trace; `--kernel-stats CSV` adds the rows of such a trace's kernel statistics as they stand.
usage: python scripts/plant_linesearch_ab.py [--turns 5] [--one] [--kernel-stats CSV] [--out profiles/plant_linesearch.json]"""
import argparse
import csv
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
from plant_adjoint_ab import leg_inputs  # noqa: E402
from plant_gradients_ab import LEGS, summary  # noqa: E402

# gfx950, -O3, from the compiler's metadata of csrc/plant_linesearch.hip (a compile, not a run)
KERNEL_RESOURCES = {"plant_ls_expand_kernel": {"vgprs": 16, "sgprs": 53, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8},
                    "plant_ls_cost_kernel": {"vgprs": 54, "sgprs": 97, "lds_bytes": 1040, "scratch_bytes": 0, "waves_per_simd": 8},
                    "plant_ls_gather_kernel": {"vgprs": 36, "sgprs": 90, "lds_bytes": 1040, "scratch_bytes": 0, "waves_per_simd": 8},
                    "plant_ls_restore_kernel": {"vgprs": 8, "sgprs": 23, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8}}
ALPHAS = tuple(0.5 ** i for i in range(8))


def setup(model, gait_file, B, T):
    import plant_gradient_cases as pgc
    import plant_riccati_cases as prc
    g, q1, v1, u = leg_inputs(model, gait_file, B, T)
    nq, nu = pgc.dims(model)[:2]
    rng = np.random.default_rng(0)
    Q, R, Qf = prc.weights(rng, 2 * nq, nu)
    ok, q, ua, gamma, b, status, iters, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
    x = np.concatenate([q[:-1], q[1:]], axis=2)
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x + 0.01 * rng.standard_normal(x.shape), u_goal=0.9 * ua)
    J, lq, lr = cost.evaluate(q, ua)
    gains = tape.lqr(Q, R, Qf, q=lq, r=lr, rho=1e-3)
    return dict(g=g, q1=q1, v1=v1, u=u, q=q, ua=ua, tape=tape, cost=cost, J=J, gains=gains, steps_converged=bool(status.all()))


def leg(name, model, gait_file, B, T, turns, one):
    s = setup(model, gait_file, B, T)
    g, tape, gains, cost = s["g"], s["tape"], s["gains"], s["cost"]
    fb = gains.feedback(s["q"])

    def closed_loop(alpha):
        *_, t, _ = plant.rollout_tape(model, s["q1"], s["v1"], s["ua"] + alpha * gains.k, g.h, g.mu, feedback=fb)
        t.close()

    def search(n, alphas=ALPHAS):
        ls = tape.linesearch(gains, s["q"], s["ua"], cost, s["J"], alphas[:n])
        ls.tape.close()
        return ls

    if one:
        search(4); search(4)
        tape.close()
        return {"leg": name}

    split = {}

    def one_iteration():
        """`plant.ilqr(max_iter=1)` with a clock around its three device calls."""
        clock = {"first_rollout_tape": 0.0, "lqr": 0.0, "linesearch": 0.0}
        kept = plant.rollout_tape, plant.RolloutTape.lqr, plant.RolloutTape.linesearch

        def timed(key, f):
            def run(*a, **kw):
                t0 = time.perf_counter()
                try:
                    return f(*a, **kw)
                finally:
                    clock[key] += (time.perf_counter() - t0) * 1e3
            return run
        plant.rollout_tape, plant.RolloutTape.lqr, plant.RolloutTape.linesearch = (timed(k, f) for k, f in zip(clock, kept))
        try:
            t0 = time.perf_counter()
            res = plant.ilqr(model, s["q1"], s["v1"], s["u"], g.h, g.mu, cost, alphas=ALPHAS[:4], max_iter=1, rho0=1e-3)
            total = (time.perf_counter() - t0) * 1e3
        finally:
            plant.rollout_tape, plant.RolloutTape.lqr, plant.RolloutTape.linesearch = kept
        res.tape.close()
        clock["host_rest"] = total - sum(clock.values())
        for k, v in clock.items():
            split.setdefault(k, []).append(v)
        return res

    runs = {"a_closed_loop_rollout_tape": lambda: closed_loop(ALPHAS[0]), "a_twin": lambda: closed_loop(ALPHAS[0])}
    runs.update({f"b_linesearch_{n}": (lambda n=n: search(n)) for n in (1, 2, 4, 8)})
    runs.update({f"b_copies_of_the_first_step_length_{n}": (lambda n=n: search(n, (ALPHAS[0],) * 8)) for n in (4, 8)})
    runs["c_four_sequential_closed_loop_rollouts"] = lambda: [closed_loop(a) for a in ALPHAS[:4]]
    runs["d_one_ilqr_iteration"] = one_iteration
    outs = {k: f() for k, f in runs.items()}                        # warm-up
    split.clear()
    times = {k: [] for k in runs}
    for _ in range(turns):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); times[k].append((time.perf_counter() - t0) * 1e3)
    tape.close()
    ls8, it = outs["b_linesearch_8"], outs["d_one_ilqr_iteration"]
    res = {"leg": name, "model": model, "B": B, "T": T, "alphas": list(ALPHAS), "nominal_steps_all_converged": s["steps_converged"],
           "robots_whose_backward_pass_ended": int((gains.status != 0).sum()),
           "candidates_acceptable_of_8_per_robot_mean": float(ls8.ok.sum(axis=0).mean()), "robots_without_an_acceptable_candidate": int((ls8.choice < 0).sum()),
           "ilqr_iteration_accepted_robots": int(it.accepted[0].sum()), "time": {k: summary(v) for k, v in times.items()},
           "ilqr_iteration_split": {k: summary(v) for k, v in split.items()}}
    med = lambda k: res["time"][k]["median_ms"]
    res["a_twin_over_a"] = round(med("a_twin") / med("a_closed_loop_rollout_tape"), 4)
    res["b1_over_a"] = round(med("b_linesearch_1") / med("a_closed_loop_rollout_tape"), 4)
    for n in (2, 4, 8):
        res[f"b{n}_over_b1"] = round(med(f"b_linesearch_{n}") / med("b_linesearch_1"), 4)
    for n in (4, 8):
        res[f"b{n}_copies_over_b1"] = round(med(f"b_copies_of_the_first_step_length_{n}") / med("b_linesearch_1"), 4)
    res["c4_over_b4"] = round(med("c_four_sequential_closed_loop_rollouts") / med("b_linesearch_4"), 4)
    print(json.dumps(res), flush=True)
    return res


def kernel_rows(path):
    keep = ("plant_ls_", "plant_step_kernel", "plant_sensitivity_kernel", "plant_riccati_kernel")
    with open(path) as f:
        return [row for row in csv.DictReader(f) if any(k in row.get("Name", "") for k in keep)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--one", action="store_true", help="one n_alpha = 4 line search per leg and exit (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="kernel statistics of a trace of `--one`")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_linesearch.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    legs = [leg(*l, a.turns, a.one) for l in LEGS]
    if a.one:
        return
    assert a.turns >= 3, "medians of at least 3 turns"
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "kernel_resources_gfx950": KERNEL_RESOURCES, "legs": legs}
    if a.kernel_stats:
        res["kernel_trace_of_one_linesearch_n_alpha_4_per_leg_twice"] = kernel_rows(a.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
