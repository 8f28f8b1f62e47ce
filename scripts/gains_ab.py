#!/usr/bin/env python3
"""`reference_gains` on the device against the NumPy restatement of gains.jl (tests/gains_ref.py) on the host: the full centroidal trot
(H = 71 knots, N = 10 repeats: a chain of 710 Riccati steps at n = 36, m = 12) and the wall stand (nz = 114).  Wall-clock time of a whole
call, host to host, after warm-up: the median of `--repeats` calls.  The split of the device call comes from timing its pieces the same
way: the linearization alone (`plant.linearize`), the Riccati chain alone (`gains.tvlqr` on the restatement's A_t, B_t), the chain's
cost per step from N = 1 against N = 10, and what remains for dz/dθ (gains_dynamics_kernel) and the transfers.  The host column takes
the torch linearization as given (it times the restatement from rz0, rθ0 on).
usage: python scripts/gains_ab.py [--repeats 20] [--warmup 3] [--out profiles/gains_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from contactimplicitmpc.jl_amd import gains, plant  # noqa: E402
import gains_cases as gc  # noqa: E402
import gains_ref  # noqa: E402

LEGS = {"centroidal trot, H = 71, N = 10": ("centroidal_quadruped", "centroidal_inplace_trot_v7.jld2", 10),
        "wall stand, all knots, N = 10": ("centroidal_quadruped_wall", "wall_stand_FL_4.jld2", 10)}


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gains_ab.json"))
    a = ap.parse_args()
    w = gc.centroidal_weights()
    rows = []
    for leg, (name, file, N) in LEGS.items():
        model, z, th = gc.knots(name, file, "gait")
        H, nq, nu = z.shape[0], model.nq, model.nu
        _, rz0, rth0 = model.linearize_batch(z, th, gc.KAPPA)
        rz0, rth0 = np.asarray(rz0, dtype=np.float64), np.asarray(rth0, dtype=np.float64)
        AB = [gains_ref.dynamics(nq, nu, rz0[t], rth0[t]) for t in range(H)]
        A, B = np.stack([x[0] for x in AB]), np.stack([x[1] for x in AB])
        Q, R = gains_ref.weights(*w)
        Rs = np.tile(R[None], (N * H, 1, 1))
        med = lambda fn, reps=a.repeats: median_ms(fn, a.warmup, reps)
        dev = med(lambda: gains.reference_gains(name, z, th, *w, N=N))
        dev1 = med(lambda: gains.reference_gains(name, z, th, *w, N=1))
        lin = med(lambda: plant.linearize(name, z, th, gc.KAPPA))
        chain = med(lambda: gains.tvlqr(A, B, Q[None], Rs, n_keep=H))
        host = med(lambda: gains_ref.reference_gains(nq, nu, rz0, rth0, *w, N=N), max(3, a.repeats // 4))
        K_ref = gains_ref.reference_gains(nq, nu, rz0, rth0, *w, N=N)
        K_dev = gains.reference_gains(name, z, th, *w, N=N)
        per_step_us = 1e3 * (dev[0] - dev1[0]) / ((N - 1) * H)
        rows.append(dict(leg=leg, model=name, H=int(H), N=N, nz=int(model.nz), n=2 * nq, m=nu, riccati_steps=N * H,
                         device_ms=dict(median=dev[0], min=dev[1], max=dev[2]), device_N1_ms=dict(median=dev1[0], min=dev1[1], max=dev1[2]),
                         linearize_alone_ms=dict(median=lin[0], min=lin[1], max=lin[2], note="reads r0, rz0, rth0 back; the gains call reads none of them back"),
                         tvlqr_alone_ms=dict(median=chain[0], min=chain[1], max=chain[2]),
                         riccati_us_per_step=per_step_us, riccati_chain_ms=per_step_us * N * H * 1e-3,
                         rest_ms=dev[0] - per_step_us * N * H * 1e-3,
                         numpy_ms=dict(median=host[0], min=host[1], max=host[2]), speedup=host[0] / dev[0],
                         parity=float(np.abs(K_dev - K_ref).max() / np.abs(K_ref).max())))
        print(json.dumps(rows[-1]))
    doc = dict(what="reference_gains on the device against the NumPy restatement on the host, wall clock host to host, median of "
                    f"{a.repeats} calls after {a.warmup} warm-up calls", repeats=a.repeats, warmup=a.warmup, legs=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
