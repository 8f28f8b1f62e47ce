#!/usr/bin/env python3
"""What time-varying LQR gains along a device rollout cost, on the two legs of scripts/plant_gradients_ab.py (quadruped B 256 T 100,
centroidal_quadruped B 64 T 60), in ONE process:

  (a) `RolloutTape.lqr` alone on a tape made beforehand, the pure-gain call and the call with linear terms;
  (b) `rollout_tape` + `lqr` (+ closing the tape) against the plain `rollout`: what the gains add to a rollout;
  (c) the host path it replaces, with calls that exist without this kernel: `rollout(diff_sol=True)` - every block read back -, A_t, B_t
      gathered on the host, `gains.tvlqr` with n_prob = B (which uploads them again); the gather and `tvlqr` are also timed alone on
      blocks already on the host.

One GPU, one process, a warm call each, then alternating turns, a host clock around whole calls (each ends in a stream synchronize);
medians, minima and maxima over `--turns` turns (at least 20).  Recorded, not asserted.  The two paths' gains are compared (they are not
equal bit for bit: the dense chain sums over the zero blocks too).  `--figures-from LOG` adds the figures a `pytest -s` run of
tests/test_gpu_plant_riccati.py printed, as they stand.
usage: python scripts/plant_riccati_ab.py [--turns 20] [--figures-from LOG] [--out profiles/plant_riccati.json]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from contactimplicitmpc.jl_amd import gains, plant  # noqa: E402
from plant_adjoint_ab import leg_inputs  # noqa: E402
from plant_gradients_ab import LEGS, summary  # noqa: E402

# gfx950, -O3, from the compiler's metadata of csrc/plant_riccati.hip (a compile, not a run)
KERNEL_RESOURCES = {"plant_riccati_kernel<false>": {"vgprs": 118, "sgprs": 106, "scratch_bytes": 0, "vgpr_spills": 0},
                    "plant_riccati_kernel<true>": {"vgprs": 129, "sgprs": 106, "scratch_bytes": 0, "vgpr_spills": 0}}


def gather(dz, nq, nu):
    """A (B, T, n, n), B (B, T, n, m) of StepGradients.dz (T, B, nr, n_cols), vectorized."""
    T, B = dz.shape[:2]
    n = 2 * nq
    A, Bm = np.zeros((B, T, n, n)), np.zeros((B, T, n, nu))
    A[:, :, :nq, nq:] = np.eye(nq)
    A[:, :, nq:, :] = dz[:, :, :nq, :n].transpose(1, 0, 2, 3)
    Bm[:, :, nq:, :] = dz[:, :, :nq, n:n + nu].transpose(1, 0, 2, 3)
    return A, Bm


def leg(name, model, gait_file, B, T, turns):
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    import plant_riccati_cases as prc
    g, q1, v1, u = leg_inputs(model, gait_file, B, T)
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(model)
    n, m = 2 * nq, nu
    rng = np.random.default_rng(0)
    Q, R, Qf = prc.weights(rng, n, m)
    q, r = rng.standard_normal((T + 1, B, n)), rng.standard_normal((T, B, m))
    Qh = np.broadcast_to(np.concatenate([np.broadcast_to(Q, (T, n, n)), Qf[None]])[None], (B, T + 1, n, n))
    Rh = np.broadcast_to(R[None, None], (B, 1, m, m))
    *_, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
    *_, G = plant.rollout(model, q1, v1, u, g.h, g.mu, diff_sol=True)

    def tape_and_lqr():
        *_, t = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
        with t:
            return t.lqr(Q, R, Qf)

    def host_gains(dz):
        A, Bm = gather(dz, nq, nu)
        return gains.tvlqr(A, Bm, Qh, Rh)

    def host_path():
        *_, G2 = plant.rollout(model, q1, v1, u, g.h, g.mu, diff_sol=True)
        return host_gains(G2.dz)

    runs = {"lqr_pure_gains": lambda: tape.lqr(Q, R, Qf),
            "lqr_with_linear_terms": lambda: tape.lqr(Q, R, Qf, q=q, r=r),
            "rollout_plain": lambda: plant.rollout(model, q1, v1, u, g.h, g.mu),
            "rollout_tape_and_lqr": tape_and_lqr,
            "host_path_rollout_diff_sol_gather_tvlqr": host_path,
            "host_gather_and_tvlqr_alone": lambda: host_gains(G.dz)}
    outs = {k: f() for k, f in runs.items()}                        # warm-up, and the outputs side by side
    times = {k: [] for k in runs}
    for _ in range(turns):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); times[k].append((time.perf_counter() - t0) * 1e3)
    tape.close()
    mine, (K_host, P_host) = outs["lqr_pure_gains"], outs["host_path_rollout_diff_sol_gather_tvlqr"]
    res = {"leg": name, "model": model, "B": B, "T": T, "n": n, "m": m, "blocks_read_back_by_the_host_path_bytes": T * B * nr * (n + m) * 8,
           "corner_bytes_the_kernel_reads": T * B * nq * (n + m) * 8, "lds_bytes_a_workgroup": 8 * (2 * n * n + 2 * nq * (n + m) + 2 * nq * n + m * nq
                                                                                                   + 3 * m * n + m * (n + 1) + 2 * m * m + 2 * n + 3 * m + nq + 4),
           "n_cut_total": int(mine.n_cut.sum()), "robots_whose_chain_ended": int((mine.status != 0).sum()),
           "time": {k: summary(v) for k, v in times.items()},
           "device_K_vs_host_path_K_max_rel": pac.distance(mine.K, K_host.transpose(1, 0, 2, 3)),
           "device_P0_vs_host_path_P1_max_rel": pac.distance(mine.P0, P_host),
           "tape_and_lqr_equals_lqr_on_the_tape_bit_for_bit": bool(outs["rollout_tape_and_lqr"].K.tobytes() == mine.K.tobytes())}
    med = lambda k: res["time"][k]["median_ms"]
    res["rollout_tape_and_lqr_over_rollout_plain"] = round(med("rollout_tape_and_lqr") / med("rollout_plain"), 3)
    res["host_path_over_rollout_tape_and_lqr"] = round(med("host_path_rollout_diff_sol_gather_tvlqr") / med("rollout_tape_and_lqr"), 3)
    res["host_gather_and_tvlqr_alone_over_lqr"] = round(med("host_gather_and_tvlqr_alone") / med("lqr_pure_gains"), 3)
    print(json.dumps(res), flush=True)
    return res


def figures(path):
    """The lines of a `pytest -s` log of tests/test_gpu_plant_riccati.py that state a measured figure, as they stand."""
    keep = re.compile(r"at most .* from lq_ld|from tvlqr|closed loop, |from the longdouble product")
    with open(path) as f:
        return [line.strip().lstrip(".") for line in f if keep.search(line)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=20)
    ap.add_argument("--figures-from", default=None, metavar="LOG", help="a `pytest -s` log of tests/test_gpu_plant_riccati.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_riccati.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.turns >= 20, "medians of at least 20 turns"
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "kernel_resources_gfx950": KERNEL_RESOURCES,
           "legs": [leg(*l, a.turns) for l in LEGS]}
    if a.figures_from:
        res["figures_of_tests_test_gpu_plant_riccati"] = figures(a.figures_from)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
