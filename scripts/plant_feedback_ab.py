#!/usr/bin/env python3
"""What closing the loop inside the device rollout costs, and that it costs the open loop nothing, on the two legs of
scripts/plant_adjoint_ab.py (quadruped B = 256, T = 100; centroidal_quadruped B = 64, T = 60):

  (1) closed-loop `plant.rollout(feedback=)` against the open-loop `plant.rollout` of the same shape on this build, alternating - with
      K = 0, which walks the open loop's trajectory and so costs the same interior-point work plus the law and its stores (the
      feature's own cost), and with seeded random gains, whose trajectory and iteration counts are its own;
  (2) closed-loop `plant.rollout` under the random gains against the host loop it replaces, `plant.simulate` with the law in NumPy;
  (3) `plant.rollout_tape(feedback=)` + `vjp` (K = 0) against the plain rollout;
  (4) open-loop `rollout` and `vjp` of this build against a build of the parent commit (`--parent-root DIR`, a checkout of the parent
      with its library built), in alternating fresh processes, three alternations (`vjp`: medians of 20 x `--turns` calls): the ratio of the medians' medians beside the
      spread of the parent's own medians (max - min);
  (5) with the same `--parent-root`, `rollout`, `rollout(diff_sol=True)` and `rollout_tape(...).vjp(...)` on the cases of
      tests/plant_gradient_cases.ROLLOUTS dumped by both builds and compared array by array with `np.array_equal`.

One GPU; a warm call, then alternating turns, a host clock around whole calls, medians of `--turns` turns (at least 7).  Recorded, not
asserted.
usage: python scripts/plant_feedback_ab.py [--turns 7] [--parent-root DIR] [--out profiles/plant_feedback.json]
       python scripts/plant_feedback_ab.py --worker ROOT [--dump FILE.npz]      (what (4) and (5) start: one build, one process)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAITS = os.path.join(ROOT, "tests", "golden", "gaits")
LEGS = (("quadruped gait2 replay", "quadruped", "quadruped_gait2", 256, 100), ("centroidal in-place trot replay", "centroidal_quadruped", "centroidal_inplace_trot_v7", 64, 60))
# standard deviation of the random gains: at 0.02 the planar quadruped leaves its gait (a third of its steps then run to max_iter and
# the rollout takes 3.1 x the open loop's time), so its leg is measured at a tenth of that
GAIN_SCALE = {"quadruped": 0.002, "centroidal_quadruped": 0.02}


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "turns": len(ms)}


def timed(runs, turns):
    """{name: [ms]} of callables run in alternating turns after one warm call each."""
    for f in runs.values():
        f()
    times = {n: [] for n in runs}
    for _ in range(turns):
        for n, f in runs.items():
            t0 = time.perf_counter(); f(); times[n].append((time.perf_counter() - t0) * 1e3)
    return times


def leg_inputs(gait_io, gait_file, B, T):
    g = gait_io.load_gait(os.path.join(GAITS, gait_file + ".jld2"))
    k = np.arange(B) * g.H // B
    q1, v1 = np.ascontiguousarray(g.q[k + 1]), (g.q[k + 1] - g.q[k]) / g.h
    u = np.ascontiguousarray(np.stack([g.u[(k + t) % g.H] for t in range(T)]))
    x_ref = np.stack([np.concatenate([g.q[(k + t) % g.H], g.q[(k + t) % g.H + 1]], axis=1) for t in range(T)])      # (T, B, 2nq): each robot's own phase
    return g, q1, v1, u, x_ref


# ---- one build in one process: (4) and (5) ---------------------------------------------------------------------------------------------------
def worker(root, turns, dump):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)      # the package of the build under test
    sys.path.append(ROOT)         # whatever else the test helpers import
    from contactimplicitmpc.jl_amd import gait_io, plant
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    if dump:
        out = {}
        for which in pgc.ROLLOUTS:
            c = pgc.rollout_case(which)
            nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
            args = (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])
            for name, a in zip(("q", "u_applied", "gamma", "b", "status", "iters"), plant.rollout(*args, terrain=c["terrain"])[1:]):
                out[f"{which}/rollout/{name}"] = a
            *plain, G = plant.rollout(*args, terrain=c["terrain"], diff_sol=True, grad_cols=nth)
            for name, a in zip(("q", "u_applied", "gamma", "b", "status", "iters"), plain[1:]):
                out[f"{which}/diff_sol/{name}"] = a
            out[f"{which}/diff_sol/dz"], out[f"{which}/diff_sol/z"], out[f"{which}/diff_sol/grad_status"] = G.dz, G.z, G.status
            *_, tape = plant.rollout_tape(*args, terrain=c["terrain"], grad_cols=nth)
            gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), c["T"], c["q1"].shape[0], nq, nc, nb)
            with tape:
                cot = tape.vjp(gq, gg, gb)
            for name in ("q1", "v1", "u", "u_step", "mu", "h", "n_cut", "g_q0", "g_q1", "w_step", "g_mu", "g_h"):
                out[f"{which}/vjp/{name}"] = np.asarray(getattr(cot, name))
        np.savez(dump, **out)
        print(json.dumps({"dumped": len(out)}), flush=True)
        return
    res = {}
    for name, model, gait_file, B, T in LEGS:
        g, q1, v1, u, _ = leg_inputs(gait_io, gait_file, B, T)
        nq, nu, nc, nb = pgc.dims(model)[:4]
        gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), T, B, nq, nc, nb)
        *_, held = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
        t = timed({"rollout": lambda: plant.rollout(model, q1, v1, u, g.h, g.mu)}, turns)
        t.update(timed({"vjp": lambda: held.vjp(gq, gg, gb)}, 20 * turns))      # a call of about 1 ms: many more turns than the rollout's
        held.close()
        res[name] = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps(res), flush=True)


def run_worker(root, turns, dump=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--turns", str(turns)] + (["--dump", dump] if dump else [])
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().split("\n")[-1])


def against_parent(parent_root, turns, tmp):
    a, b = os.path.join(tmp, "parent.npz"), os.path.join(tmp, "this.npz")
    run_worker(parent_root, turns, a); run_worker(ROOT, turns, b)
    pa, pb = np.load(a), np.load(b)
    assert sorted(pa.files) == sorted(pb.files)
    equal = {k: bool(np.array_equal(pa[k], pb[k])) for k in sorted(pa.files)}
    rounds = [(run_worker(parent_root, turns), run_worker(ROOT, turns)) for _ in range(3)]
    legs = {}
    for name, *_ in LEGS:
        legs[name] = {}
        for what in ("rollout", "vjp"):
            par, new = [r[0][name][what] for r in rounds], [r[1][name][what] for r in rounds]
            legs[name][what] = {"parent_medians_ms": [round(x, 3) for x in par], "this_medians_ms": [round(x, 3) for x in new],
                                "this_minus_parent_ms": round(statistics.median(new) - statistics.median(par), 3),
                                "parent_spread_ms": round(max(par) - min(par), 3), "this_over_parent": round(statistics.median(new) / statistics.median(par), 4)}
    return {"open_loop_bit_for_bit": {"arrays": len(equal), "array_equal": equal, "all_equal": all(equal.values())}, "open_loop_against_parent": legs}


# ---- this build: (1), (2), (3) ---------------------------------------------------------------------------------------------------------------
def leg(name, model, gait_file, B, T, turns):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from contactimplicitmpc.jl_amd import gait_io, plant
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    g, q1, v1, u, x_ref = leg_inputs(gait_io, gait_file, B, T)
    nq, nu, nc, nb = pgc.dims(model)[:4]
    K = GAIN_SCALE[model] * np.random.default_rng(1).standard_normal((T, B, nu, 2 * nq))
    fb, fb0 = plant.Feedback(K, x_ref), plant.Feedback(np.zeros(K.shape), x_ref)
    gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), T, B, nq, nc, nb)

    class Law:      # the host loop's policy: the law in NumPy, batched over the robots
        def __init__(self):
            self.t, self.prev = 0, q1 - g.h * v1

        def __call__(self, q):
            x = np.concatenate([q - 1.0 * (q - self.prev), q], axis=1)
            ut = u[self.t] + np.einsum("bij,bj->bi", K[self.t], x_ref[self.t] - x)
            self.t, self.prev = self.t + 1, q.copy()
            return ut

    def tape_route():
        *_, tape, _ = plant.rollout_tape(model, q1, v1, u, g.h, g.mu, feedback=fb0)
        with tape:
            return tape.vjp(gq, gg, gb)

    closed = plant.rollout(model, q1, v1, u, g.h, g.mu, feedback=fb)
    host = plant.simulate(model, Law(), q1, v1, T, g.h, g.mu)
    t = timed({"rollout_open_loop": lambda: plant.rollout(model, q1, v1, u, g.h, g.mu),
               "rollout_closed_loop_zero_gains": lambda: plant.rollout(model, q1, v1, u, g.h, g.mu, feedback=fb0),
               "rollout_closed_loop": lambda: plant.rollout(model, q1, v1, u, g.h, g.mu, feedback=fb),
               "rollout_tape_feedback_and_vjp": tape_route}, turns)
    t.update(timed({"host_loop_simulate_with_numpy_law": lambda: plant.simulate(model, Law(), q1, v1, T, g.h, g.mu)}, 3))
    med = {n: statistics.median(v) for n, v in t.items()}
    plain = plant.rollout(model, q1, v1, u, g.h, g.mu)
    res = {"leg": name, "model": model, "B": B, "T": T, "gain_scale": GAIN_SCALE[model], "open_loop_steps_converged": float(plain[5].mean()),
           "closed_loop_steps_converged": float(closed[5].mean()),
           "host_loop_max_abs_dq": float(np.abs(host[1] - closed[1]).max()), "time": {n: summary(v) for n, v in t.items()},
           "closed_zero_gains_over_open_loop": round(med["rollout_closed_loop_zero_gains"] / med["rollout_open_loop"], 4),
           "closed_over_open_loop": round(med["rollout_closed_loop"] / med["rollout_open_loop"], 4),
           "host_loop_over_closed_loop": round(med["host_loop_simulate_with_numpy_law"] / med["rollout_closed_loop"], 3),
           "tape_feedback_zero_gains_and_vjp_over_open_loop": round(med["rollout_tape_feedback_and_vjp"] / med["rollout_open_loop"], 4)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=7)
    ap.add_argument("--parent-root", default=None, metavar="DIR", help="a checkout of the parent commit with its library built")
    ap.add_argument("--worker", default=None, metavar="ROOT")
    ap.add_argument("--dump", default=None, metavar="FILE")
    ap.add_argument("--tmp", default=None, metavar="DIR", help="where the two dumps go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_feedback.json"))
    a = ap.parse_args()
    assert a.turns >= 7, "medians of at least 7 turns"
    if a.worker:
        return worker(os.path.abspath(a.worker), a.turns, a.dump)
    sys.path.insert(0, ROOT)
    import tempfile
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "turns": a.turns,
           "command": "python scripts/plant_feedback_ab.py " + " ".join(sys.argv[1:]),
           "legs": [leg(*l, a.turns) for l in LEGS]}
    if a.parent_root:
        with tempfile.TemporaryDirectory() as tmp:
            res.update(against_parent(os.path.abspath(a.parent_root), a.turns, a.tmp or tmp))
    if os.path.exists(a.out):      # keep what other tools recorded there (scripts/closed_loop_gains_rollout.py)
        old = json.load(open(a.out))
        res = {**{k: v for k, v in old.items() if k not in res}, **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
