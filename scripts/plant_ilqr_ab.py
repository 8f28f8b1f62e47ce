#!/usr/bin/env python3
"""What an iLQR iteration costs with the loop on the device (`plant.ilqr(device_loop=True)`, `cimpc_plant_ilqr`; DESIGN.md section 3,
item 3h) against the host loop (`device_loop=False`: one `lqr` per rho level or one limited `lqr`, one `linesearch`, NumPy between
them), in ONE process:

  centroidal_quadruped B 64 T 60 (the leg of scripts/plant_linesearch_ab.py, its cost, four step lengths) and the three hoppers of
  `plant_gradient_cases.rollout_case("hopper_2D")` (B 3 T 14, the contact cost, three step lengths), each without and with control limits
  (0.6 of the largest |u| the unlimited host run ends with).

Both sides run a FIXED number of iterations: tol = 0 and rho_max = inf, so that no robot ever stops and the loops cannot end early.  Timed
per turn, alternating: (a) the host loop and (a') its twin, so that the A/A spread of the session is on record, (b) the device loop, and
(f) what both do before their first iteration - `rollout_tape` and `cost.evaluate` - whose median is taken off (a) and (b) before dividing
by the iteration count.  A warm call each, a host clock around whole calls (each ends in a stream synchronize); medians, minima and maxima
over `--turns` turns.  The host loop's split - `lqr`, `linesearch`, the rest - comes from clocks around its two device calls; the device
loop's split needs a kernel trace: `--one` runs two device loops per case and exits, and `--kernel-stats CSV` adds the rows of such a
trace's kernel statistics (the Riccati kernel, the line search's kernels, the new plant_ilqr_* kernels) as they stand.  The two results
are compared bit for bit before anything is timed.  Recorded, not asserted.
usage: python scripts/plant_ilqr_ab.py [--turns 5] [--iters 3] [--one] [--kernel-stats CSV] [--copy-stats CSV] [--out profiles/plant_ilqr.json]"""
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


# gfx950, -O3, from the compiler's metadata of csrc/plant_ilqr.hip (a compile, not a run)
KERNEL_RESOURCES = {"plant_ilqr_rho_kernel": {"vgprs": 6, "sgprs": 14, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8},
                    "plant_ilqr_nominal_kernel": {"vgprs": 8, "sgprs": 18, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8},
                    "plant_ilqr_commit_kernel": {"vgprs": 12, "sgprs": 65, "lds_bytes": 0, "scratch_bytes": 0, "waves_per_simd": 8}}


def centroidal():
    import plant_gradient_cases as pgc
    import plant_riccati_cases as prc
    name, model, gait_file, B, T = LEGS[1]
    g, q1, v1, u = leg_inputs(model, gait_file, B, T)
    nq, nu = pgc.dims(model)[:2]
    rng = np.random.default_rng(0)
    Q, R, Qf = prc.weights(rng, 2 * nq, nu)
    ok, q, ua, *_, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
    tape.close()
    x = np.concatenate([q[:-1], q[1:]], axis=2)
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x + 0.01 * rng.standard_normal(x.shape), u_goal=0.9 * ua)
    return dict(name=name, model=model, B=B, T=T, args=(model, q1, v1, u, g.h, g.mu), cost=cost, kw=dict(alphas=(1.0, 0.5, 0.25, 0.125), rho0=1e-3))


def hoppers():
    import plant_gradient_cases as pgc
    import plant_ilqr_cases as pic
    import plant_linesearch_cases as plc
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    return dict(name="three hoppers through contact", model="hopper_2D", B=3, T=c["T"], args=pic.args(c), cost=plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal),
                kw=dict(alphas=(1.0, 0.5, 0.25), rho0=1e-6))


def same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in ("u", "q", "gamma", "b", "J", "alpha", "rho", "accepted", "J0")) and \
        all(np.array_equal(getattr(a.gains, k), getattr(b.gains, k)) for k in ("K", "k", "dV", "status", "n_cut"))


def case(c, limited, iters, turns, one):
    kw = dict(c["kw"], max_iter=iters, tol=0.0, rho_max=np.inf)
    if limited:
        free = plant.ilqr(*c["args"], c["cost"], **kw)
        free.tape.close()
        bound = 0.6 * np.abs(free.u).max()
        kw.update(u_lo=np.full(free.u.shape[2], -bound), u_hi=np.full(free.u.shape[2], bound))

    def loop(device):
        res = plant.ilqr(*c["args"], c["cost"], device_loop=device, **kw)
        res.tape.close()
        return res

    def first():
        u = c["args"][3]
        if limited:
            u = np.clip(u, kw["u_lo"], kw["u_hi"])
        ok, q, ua, *_, tape = plant.rollout_tape(c["args"][0], c["args"][1], c["args"][2], u, *c["args"][4:])
        tape.close()
        return c["cost"].evaluate(q, ua)

    if one:
        loop(True); loop(True)
        return {"case": c["name"], "limited": limited}
    split = {}

    def host_with_clocks():
        clock = {"lqr": 0.0, "linesearch": 0.0}
        kept = plant.RolloutTape.lqr, plant.RolloutTape.linesearch

        def timed(key, f):
            def run(*a, **k):
                t0 = time.perf_counter()
                try:
                    return f(*a, **k)
                finally:
                    clock[key] += (time.perf_counter() - t0) * 1e3
            return run
        plant.RolloutTape.lqr, plant.RolloutTape.linesearch = (timed(k, f) for k, f in zip(clock, kept))
        try:
            res = loop(False)
        finally:
            plant.RolloutTape.lqr, plant.RolloutTape.linesearch = kept
        for k, v in clock.items():
            split.setdefault(k, []).append(v / iters)
        return res

    runs = {"a_host_loop": host_with_clocks, "a_twin": lambda: loop(False), "b_device_loop": lambda: loop(True), "f_first_rollout_and_cost": first}
    outs = {k: f() for k, f in runs.items()}                        # warm-up
    host, dev = outs["a_host_loop"], outs["b_device_loop"]
    assert host.J.shape[0] == dev.J.shape[0] == iters, "a loop ended early: the iteration count is not fixed"
    split.clear()
    times = {k: [] for k in runs}
    for _ in range(turns):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"case": c["name"], "model": c["model"], "B": c["B"], "T": c["T"], "limited": limited, "iterations": iters, "alphas": list(kw["alphas"]),
           "device_loop_equals_host_loop_bit_for_bit": bool(same(dev, host)), "accepted_per_iteration": host.accepted.sum(axis=1).tolist(),
           "J0": host.J0.tolist() if c["B"] <= 8 else float(host.J0.sum()), "J_end": host.J[-1].tolist() if c["B"] <= 8 else float(host.J[-1].sum()),
           "time_of_a_whole_call": {k: summary(v) for k, v in times.items()},
           "host_loop_split_ms_per_iteration": {k: summary(v) for k, v in split.items()}}
    med = lambda k: res["time_of_a_whole_call"][k]["median_ms"]
    per = lambda k: round((med(k) - med("f_first_rollout_and_cost")) / iters, 3)
    res["ms_per_iteration"] = {"host_loop": per("a_host_loop"), "host_loop_twin": per("a_twin"), "device_loop": per("b_device_loop")}
    res["host_loop_split_ms_per_iteration"]["rest_median_ms"] = round(per("a_host_loop") - sum(v["median_ms"] for v in res["host_loop_split_ms_per_iteration"].values()), 3)
    res["twin_over_host"] = round(per("a_twin") / per("a_host_loop"), 4)
    res["device_over_host"] = round(per("b_device_loop") / per("a_host_loop"), 4)
    print(json.dumps(res), flush=True)
    return res


def kernel_rows(path):
    keep = ("plant_ilqr_", "plant_ls_", "plant_step_kernel", "plant_sensitivity_kernel", "plant_riccati_kernel")
    with open(path) as f:
        return [row for row in csv.DictReader(f) if any(k in row.get("Name", "") for k in keep)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--one", action="store_true", help="two device loops per case and exit (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="kernel statistics of a trace of `--one`")
    ap.add_argument("--copy-stats", default=None, metavar="CSV", help="memory-copy statistics of the same trace (never one taken with counters)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_ilqr.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    cases = [case(c, limited, a.iters, a.turns, a.one) for c in (centroidal(), hoppers()) for limited in (False, True)]
    if a.one:
        return
    assert a.turns >= 3, "medians of at least 3 turns"
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "kernel_resources_gfx950": KERNEL_RESOURCES, "cases": cases,
           "not_measured": "quadruped B = 256, T = 100 (an iteration of the host loop takes 7.7 s there: profiles/plant_linesearch.json)"}
    if a.kernel_stats:
        res["kernel_trace_of_two_device_loops_per_case"] = {"iterations_per_loop": a.iters, "rows": kernel_rows(a.kernel_stats)}
    if a.copy_stats:
        with open(a.copy_stats) as f:
            res["memory_copies_of_that_trace"] = list(csv.DictReader(f))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
