#!/usr/bin/env python3
"""What a loss gradient through a device rollout costs, three ways, on the two legs of scripts/plant_gradients_ab.py:

  (a) `plant.rollout` alone, of this build and of another build of the library (`--parent-lib PATH`, a build of the parent commit);
  (b) `plant.rollout(diff_sol=True)` - every step's block read back and transposed - and the reverse chain on the host in NumPy
      (batched over the robots with `@`, what a user would write);
  (c) `plant.rollout_tape` and `RolloutTape.vjp`: the blocks stay on the device, one more launch walks the chain.

Also the `vjp` call alone on a tape made beforehand and, with `--kernel-stats FILE` (the kernel statistics of a profiler run of
`--vjp-only N`, made separately), the time of `plant_adjoint_kernel` itself.  One GPU, one process, a warm call, then alternating turns,
a host clock around whole calls; medians over `--turns` turns (at least 20).  Recorded, not asserted; (a) of this build is compared
with the parent build's outputs bit for bit.
usage: python scripts/plant_adjoint_ab.py [--turns 20] [--parent-lib PATH] [--kernel-stats FILE] [--out profiles/plant_adjoint.json]
       python scripts/plant_adjoint_ab.py --vjp-only 20      (under a profiler: N `vjp` calls per leg, nothing written)"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from contactimplicitmpc.jl_amd import _lib, gait_io, plant  # noqa: E402
from plant_gradients_ab import GAITS, LEGS, parent_rollout, summary  # noqa: E402


def host_chain(D, gq, gg, gb, nq, nu):
    """The reverse chain in float64 NumPy over StepGradients.dz (T, B, nr, n_cols), batched over the robots."""
    T, B = D.shape[:2]
    lam = gq.copy()
    u_step = np.zeros((T, B, nu))
    for t in range(T - 1, -1, -1):
        a = np.concatenate([lam[t + 2], gg[t], gb[t]], axis=1)
        v = (a[:, None, :] @ D[t])[:, 0]
        lam[t + 1] += v[:, nq:2 * nq]
        lam[t] += v[:, :nq]
        u_step[t] = v[:, 2 * nq:2 * nq + nu]
    return lam[0], lam[1], u_step


def leg_inputs(model, gait_file, B, T):
    g = gait_io.load_gait(os.path.join(GAITS, gait_file + ".jld2"))
    k = np.arange(B) * g.H // B
    q1, v1 = np.ascontiguousarray(g.q[k + 1]), (g.q[k + 1] - g.q[k]) / g.h
    u = np.ascontiguousarray(np.stack([g.u[(k + t) % g.H] for t in range(T)]))
    return g, q1, v1, u


def leg(name, model, gait_file, B, T, turns, parent):
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    g, q1, v1, u = leg_inputs(model, gait_file, B, T)
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(model)
    gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), T, B, nq, nc, nb)
    plain = lambda: plant.rollout(model, q1, v1, u, g.h, g.mu)

    def host_route():
        *_, G = plant.rollout(model, q1, v1, u, g.h, g.mu, diff_sol=True)
        return host_chain(G.dz, gq, gg, gb, nq, nu)

    def tape_route():
        *_, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
        with tape:
            c = tape.vjp(gq, gg, gb)
        return c.g_q0, c.g_q1, c.u_step

    *_, held = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
    runs = {"rollout": plain, "rollout_diff_sol_and_host_chain": host_route, "rollout_tape_and_vjp": tape_route, "vjp_alone": lambda: held.vjp(gq, gg, gb)}
    if parent is not None:
        runs["rollout_parent_build"] = parent_rollout(parent, model, q1, v1, u, g.h, g.mu)
    outs = {n: f() for n, f in runs.items()}                        # warm-up, and the outputs side by side
    times = {n: [] for n in runs}
    for _ in range(turns):
        for n, f in runs.items():
            t0 = time.perf_counter(); f(); times[n].append((time.perf_counter() - t0) * 1e3)
    held.close()
    host, dev = outs["rollout_diff_sol_and_host_chain"], outs["rollout_tape_and_vjp"]
    res = {"leg": name, "model": model, "B": B, "T": T, "n_cols": 2 * nq + nu, "block_bytes_read_back_by_the_host_route": T * B * nr * (2 * nq + nu) * 8,
           "cotangent_bytes_up": (gq.size + gg.size + gb.size) * 8, "gradient_bytes_down": (2 * B * nq + T * B * nu) * 8 + 4 * B,
           "n_cut_total": int(outs["vjp_alone"].n_cut.sum()), "time": {n: summary(v) for n, v in times.items()},
           "tape_vs_host_chain_max_rel": max(pac.distance(d, h) for d, h in zip(dev, host))}
    med = lambda n: res["time"][n]["median_ms"]
    res["tape_and_vjp_over_rollout_this_build"] = round(med("rollout_tape_and_vjp") / med("rollout"), 4)
    res["host_route_over_rollout_this_build"] = round(med("rollout_diff_sol_and_host_chain") / med("rollout"), 4)
    res["host_route_over_tape_and_vjp"] = round(med("rollout_diff_sol_and_host_chain") / med("rollout_tape_and_vjp"), 3)
    if parent is not None:
        res["rollout_identical_to_parent_build"] = all(np.array_equal(x, y) for x, y in zip(outs["rollout"][1:2] + outs["rollout"][3:], outs["rollout_parent_build"]))
        res["tape_and_vjp_over_rollout_parent_build"] = round(med("rollout_tape_and_vjp") / med("rollout_parent_build"), 4)
        res["host_route_over_rollout_parent_build"] = round(med("rollout_diff_sol_and_host_chain") / med("rollout_parent_build"), 4)
        res["rollout_this_over_parent_build"] = round(med("rollout") / med("rollout_parent_build"), 4)
    print(json.dumps(res), flush=True)
    return res


def vjp_only(n):
    """For a profiler run: per leg one tape and n walks of it."""
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    for name, model, gait_file, B, T in LEGS:
        g, q1, v1, u = leg_inputs(model, gait_file, B, T)
        nq, nu, nc, nb = pgc.dims(model)[:4]
        gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), T, B, nq, nc, nb)
        *_, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
        with tape:
            for _ in range(n):
                tape.vjp(gq, gg, gb)
        print(name, "walked", n, "times", flush=True)


def kernel_stats(path):
    """The plant_adjoint_kernel rows of a profiler's kernel statistics (CSV with a name column and its timing columns), as they stand."""
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if any("plant_adjoint_kernel" in str(v) for v in row.values())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, metavar="PATH", help="libcimpc_hip.so of the parent commit")
    ap.add_argument("--kernel-stats", default=None, metavar="FILE", help="kernel statistics (CSV) of a profiler run of --vjp-only")
    ap.add_argument("--vjp-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_adjoint.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    if a.vjp_only:
        return vjp_only(a.vjp_only)
    assert a.turns >= 20, "medians of at least 20 turns"
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.cimpc_plant_rollout.restype, parent.cimpc_plant_rollout.argtypes = _lib.SIGNATURES["cimpc_plant_rollout"]
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "parent_build_measured": parent is not None,
           "legs": [leg(*l, a.turns, parent) for l in LEGS]}
    if a.kernel_stats:
        res["plant_adjoint_kernel_profiler_rows"] = kernel_stats(a.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
