#!/usr/bin/env python3
"""What multiple-shooting iLQR costs when the horizon is cut into segments that roll out abreast: the stages
(`plant.rollout_segments`, `RolloutTape.lqr(defects=)`) against the sequential calls (`plant.rollout_tape`, `RolloutTape.lqr`), and an
iteration of `plant.ilqr_shooting` against one of `plant.ilqr`'s host loop, in ONE process:

  centroidal_quadruped B 64 T 60 (the leg of scripts/plant_linesearch_ab.py and its cost) and the three hoppers of
  `plant_gradient_cases.rollout_case("hopper_2D")` cut to T 12, at M = 1, 2, 4, 6, 12 segments; the nodes are those of the sequential
  rollout, so every segment does the work its steps do in the sequential call.

THE PREDICTION, written before the first run.  The step kernel is one wavefront per robot walking its steps one after another, and the
card is nearly empty at these shapes (profiles/plant_linesearch.json: four step lengths of 64 robots in 1.02 x the time of one).  So the
rollout's share scales with L / T: `rollout_segments` at M segments should take about 1 / M of `rollout_tape`'s time plus what does not
scale - the sensitivity launch over the same T B entries, the copies of the same rows, and the two new row-moving kernels, of the order of
the line search's 0.4 to 0.6 ms.  The backward pass does not shorten: it is a chain over T steps whatever M is, the hook adds n^2
multiply-adds at M - 1 of its steps, and `lqr(defects=)` should cost what the limited `lqr` costs, about 7 ms on centroidal.
Whether that held is recorded in the output under "prediction".

THE LOOP (`loop_case`).  ms per iteration of `ilqr_shooting` at M = 1, 2, 4, 6, 12 against `plant.ilqr`'s host loop and its A/A twin, on
alternating turns: every loop runs a FIXED number of iterations (tol = 0, rho_max = inf, defect_tol = 0, so that no robot stops), once with
LOOP_ITERS and once with 1 iteration, and the per-iteration time is the difference of the two medians over LOOP_ITERS - 1: what the loops do
before their first iteration drops out.  Prediction, written before the first run: the iteration's rollout share - the line search's one
closed-loop rollout - scales with L / T as the rollout above does; the new kernels are of the order of the line search's 0.4 to 0.6 ms;
the backward pass and the linear forward pass do not scale, the forward pass being of the order of `lqr`'s 7 ms on centroidal; so an iteration
at M segments should cost about (line search) / M + (lqr + forward + host) and stop falling where the second term takes over.  On the
hoppers also: the iterations and the wall time `ilqr_shooting` (from the sequential start, the settings of the contact test) needs to bring
every robot's J within REACH_GAP of the single-shooting final J with D <= defect_tol.

NOT measured here: the forward kernel alone; a kernel trace; quadruped B = 256.

Timed per turn, alternating: (a) the sequential call and (a') its twin, so that the A/A spread of the session is on record, then one call
per M; the backward pass twice - (b) as called, all T steps' gains read back, and (c) with keep = 1, five calls back to back per turn,
so that the chain and not the read-back is what the clock sees.  A warm call each, a host clock around whole calls (each ends in a stream synchronize); medians, minima and maxima over `--turns`
turns.  Recorded, not asserted.
usage: python scripts/plant_shooting_ab.py [--turns 7] [--out profiles/plant_shooting.json]"""
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
from plant_ilqr_ab import centroidal  # noqa: E402

SEGMENTS = (1, 2, 4, 6, 12)
LQR_REPEATS = 5
LOOP_ITERS = 3
REACH_GAP = 1e-2      # relative, of J against the single-shooting final J


def hoppers():
    import plant_linesearch_cases as plc
    import plant_shooting_cases as psc
    c = psc.problem("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    T = c["T"]
    return dict(name="three hoppers through contact", model="hopper_2D", B=3, T=T, args=(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"]),
                cost=plant.TrackingCost(Q, R, Qf, x_goal=x_goal[:T + 1], u_goal=u_goal[:T]))


def case(c, turns):
    model, q1, v1, u, h, mu = c["args"]
    cost, T = c["cost"], c["T"]
    ok, q, ua, *_, tape = plant.rollout_tape(model, q1, v1, u, h, mu)
    J, lq, lr = cost.evaluate(q, ua)
    rho = np.full(c["B"], 1e-3)

    def sequential():
        *_, t = plant.rollout_tape(model, q1, v1, u, h, mu)
        t.close()

    def segments(M):
        def run():
            plant.rollout_segments(model, plant.segment_nodes(q, M), ua, h, mu, segments=M, cost=cost).tape.close()
        return run

    noms = {M: plant.rollout_segments(model, plant.segment_nodes(q, M), ua, h, mu, segments=M, cost=cost) for M in SEGMENTS}
    closed = {M: bool((n.defects == 0.0).all() and np.array_equal(n.q_stitched(), q) and np.array_equal(n.J, J)) for M, n in noms.items()}
    runs = {"a_rollout_tape": sequential, "a_twin": sequential}
    runs.update({f"rollout_segments_M{M}": segments(M) for M in SEGMENTS})
    runs["b_lqr_limited"] = lambda: tape.lqr(cost.Q, cost.R, cost.Qf, q=lq, r=lr, rho=rho)
    runs["b_twin"] = runs["b_lqr_limited"]
    runs.update({f"lqr_defects_M{M}": (lambda n=noms[M], M=M: n.tape.lqr(cost.Q, cost.R, cost.Qf, q=n.lin_q, r=n.lin_r, rho=rho, defects=n.defects, segment_len=T // M))
                 for M in SEGMENTS})
    # the same chains with keep = 1: the whole chain runs, one step's gains come back - the read-back of T steps' gains (13 MB on centroidal) is
    # taken out of the clock; LQR_REPEATS calls back to back per turn, the time divided by them
    def repeated(f):
        def run():
            for _ in range(LQR_REPEATS):
                f()
        return run
    runs["c_lqr_limited_keep1"] = repeated(lambda: tape.lqr(cost.Q, cost.R, cost.Qf, q=lq, r=lr, rho=rho, keep=1))
    runs["c_twin"] = runs["c_lqr_limited_keep1"]
    runs.update({f"lqr_defects_keep1_M{M}": repeated(lambda n=noms[M], M=M: n.tape.lqr(cost.Q, cost.R, cost.Qf, q=n.lin_q, r=n.lin_r, rho=rho, keep=1,
                                                                                     defects=n.defects, segment_len=T // M)) for M in SEGMENTS})
    for f in runs.values():
        f()                                                          # warm-up
    times = {k: [] for k in runs}
    for _ in range(turns):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); times[k].append((time.perf_counter() - t0) * 1e3 / (LQR_REPEATS if "keep1" in k or k == "c_twin" else 1))
    tape.close()
    for n in noms.values():
        n.tape.close()
    res = {"case": c["name"], "model": c["model"], "B": c["B"], "T": T, "segments": list(SEGMENTS),
           "zero_defects_and_the_sequential_trajectory_and_J_to_the_bit": closed, "time_of_a_whole_call": {k: summary(v) for k, v in times.items()}}
    med = lambda k: res["time_of_a_whole_call"][k]["median_ms"]
    res["rollout_twin_over_sequential"] = round(med("a_twin") / med("a_rollout_tape"), 4)
    res["rollout_segments_over_sequential"] = {str(M): round(med(f"rollout_segments_M{M}") / med("a_rollout_tape"), 4) for M in SEGMENTS}
    res["one_over_M"] = {str(M): round(1.0 / M, 4) for M in SEGMENTS}
    res["lqr_twin_over_limited"] = round(med("b_twin") / med("b_lqr_limited"), 4)
    res["lqr_defects_over_limited"] = {str(M): round(med(f"lqr_defects_M{M}") / med("b_lqr_limited"), 4) for M in SEGMENTS}
    res["lqr_keep1_twin_over_limited"] = round(med("c_twin") / med("c_lqr_limited_keep1"), 4)
    res["lqr_keep1_defects_over_limited"] = {str(M): round(med(f"lqr_defects_keep1_M{M}") / med("c_lqr_limited_keep1"), 4) for M in SEGMENTS}
    print(json.dumps(res), flush=True)
    return res


def loop_case(c, turns, alphas, rho0, reach):
    args, cost = c["args"], c["cost"]
    fixed = dict(alphas=alphas, rho0=rho0, tol=0.0, rho_max=np.inf)

    def single(n):
        def run():
            plant.ilqr(*args, cost, max_iter=n, **fixed).tape.close()
        return run

    def shooting(M, n):
        def run():
            plant.ilqr_shooting(*args, cost, segments=M, defect_weight=100.0, defect_tol=0.0, max_iter=n, **fixed).tape.close()
        return run

    runs = {"a_ilqr": single(LOOP_ITERS), "a_twin": single(LOOP_ITERS), "a_ilqr_1": single(1)}
    for M in SEGMENTS:
        runs[f"shooting_M{M}"] = shooting(M, LOOP_ITERS)
        runs[f"shooting_M{M}_1"] = shooting(M, 1)
    for f in runs.values():
        f()                                                          # warm-up
    times = {k: [] for k in runs}
    for _ in range(turns):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"case": c["name"], "model": c["model"], "B": c["B"], "T": c["T"], "iterations": LOOP_ITERS, "alphas": list(alphas),
           "time_of_a_whole_call": {k: summary(v) for k, v in times.items()}}
    med = lambda k: res["time_of_a_whole_call"][k]["median_ms"]
    per = lambda k, one: round((med(k) - med(one)) / (LOOP_ITERS - 1), 3)
    res["ms_per_iteration"] = {"ilqr_host_loop": per("a_ilqr", "a_ilqr_1"), "ilqr_host_loop_twin": per("a_twin", "a_ilqr_1")}
    res["ms_per_iteration"].update({f"ilqr_shooting_M{M}": per(f"shooting_M{M}", f"shooting_M{M}_1") for M in SEGMENTS})
    base = res["ms_per_iteration"]["ilqr_host_loop"]
    res["twin_over_host"] = round(res["ms_per_iteration"]["ilqr_host_loop_twin"] / base, 4)
    res["shooting_over_host"] = {str(M): round(res["ms_per_iteration"][f"ilqr_shooting_M{M}"] / base, 4) for M in SEGMENTS}
    if reach:      # iterations and wall time to the single-shooting final J
        ss = plant.ilqr(*args, cost, alphas=alphas, rho0=rho0, max_iter=10)
        ss.tape.close()
        res["single_shooting"] = {"iterations": int(ss.J.shape[0]), "J": ss.J[-1].tolist()}
        res["to_reach_single_shooting_J_within"] = REACH_GAP
        res["reach"] = {}
        for M in SEGMENTS:
            kw = dict(segments=M, defect_weight=100.0, defect_tol=1e-6, alphas=alphas, rho0=rho0)
            full = plant.ilqr_shooting(*args, cost, max_iter=60, **kw)
            full.tape.close()
            hit = [i for i in range(full.J.shape[0]) if (full.J[i] <= ss.J[-1] * (1 + REACH_GAP)).all() and (full.D[i] <= 1e-6).all()]
            entry = {"iterations_run": int(full.J.shape[0]), "iterations_to_reach": hit[0] + 1 if hit else None, "J": full.J[-1].tolist(), "D": full.D[-1].tolist()}
            if hit:
                wall = []
                for _ in range(3):
                    t0 = time.perf_counter(); plant.ilqr_shooting(*args, cost, max_iter=hit[0] + 1, **kw).tape.close(); wall.append((time.perf_counter() - t0) * 1e3)
                entry["wall_ms_to_reach"] = summary(wall)
            res["reach"][str(M)] = entry
        wall = []
        for _ in range(3):
            t0 = time.perf_counter(); plant.ilqr(*args, cost, alphas=alphas, rho0=rho0, max_iter=10).tape.close(); wall.append((time.perf_counter() - t0) * 1e3)
        res["single_shooting"]["wall_ms"] = summary(wall)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_shooting.json"))
    a = ap.parse_args()
    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.turns >= 3, "medians of at least 3 turns"
    cases = [case(c, a.turns) for c in (centroidal(), hoppers())]
    loops = [loop_case(centroidal(), max(3, a.turns // 2), (1.0, 0.5, 0.25, 0.125), 1e-3, False), loop_case(hoppers(), a.turns, (1.0, 0.5, 0.25), 1e-6, True)]
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "cases": cases, "loops": loops,
           "prediction": "rollout_segments at M segments takes about 1 / M of rollout_tape plus a part that does not scale (sensitivity launch, copies, two "
                         "row-moving kernels of the order of 0.5 ms); lqr(defects=) costs what the limited lqr costs.  Compare rollout_segments_over_sequential "
                         "with one_over_M, and lqr_defects_over_limited with 1, against the twins' spread.",
           "loop_prediction": "an iteration at M segments costs about (line search) / M + (lqr + forward pass + host); see ms_per_iteration and shooting_over_host "
                              "against twin_over_host",
           "not_measured": "the forward kernel alone; a kernel trace of the new kernels; iterations to the single-shooting J on centroidal; quadruped B = 256"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
