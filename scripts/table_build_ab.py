#!/usr/bin/env python3
"""From (z, θ) on the host to the linearization tables in a solver handle, by two paths, on the knots of quadruped gait2 (60 knots)
and of wall_stand_FL_4 (centroidal_quadruped_wall, 50 knots):
  (a) `plant.linearize` (one device call, the triple read back and transposed) followed by one `set_linearization` per knot (the table
      packed on the host, one synchronous copy each);
  (b) `CIMPCSolver.linearize_knots`: the same linearization kernel and the table build kernel on the handle's stream, nothing but z, θ
      going up and one status word per knot coming back.
Per leg and path: the median wall time of `--calls` calls after `--warmup` warm-up calls (a host clock around calls that return
synchronized), path (a) also split into its two halves; and whether the two handles' tables are equal bit for bit.
usage: python scripts/table_build_ab.py [--calls 20] [--warmup 3] [--out profiles/table_build_ab.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contactimplicitmpc.jl_amd import CIMPCSolver, InteriorPointOptions, NewtonOptions, gait_io, lcp_models, plant  # noqa: E402

GAITS = os.path.join(ROOT, "tests", "golden", "gaits")
LEGS = (("quadruped gait2", "quadruped", "quadruped_gait2", 1e-4), ("wall_stand_FL_4", "centroidal_quadruped_wall", "wall_stand_FL_4", 1e-3))


def stats(ms, calls, warmup):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls": calls, "warmup": warmup}


def leg(name, model_name, gait_file, kappa, calls, warmup):
    model = lcp_models.MODELS[model_name]()
    P = lcp_models.reference_problem(model, gait_io.load_gait(os.path.join(GAITS, gait_file + ".jld2")), kappa, tables=False)
    z, th, N = P.z, P.theta, P.H
    handle = lambda: CIMPCSolver(model.nq, model.nu, model.nw, model.nc, model.nb, N, min(N, 10), B=1, mode=0,
                                 ip_opts=InteriorPointOptions(kappa_tol=kappa), newton_opts=NewtonOptions(kappa=kappa))
    A, B = handle(), handle()
    a_ms, a_lin_ms, a_set_ms, b_ms = [], [], [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        r0, rz0, rth0 = plant.linearize(model_name, z, th, kappa)
        t1 = time.perf_counter()
        for t in range(N):
            A.set_linearization(t + 1, z[t], th[t], r0[t], rz0[t], rth0[t])
        t2 = time.perf_counter()
        B.linearize_knots(model_name, z, th, kappa)
        t3 = time.perf_counter()
        if i >= warmup:
            a_ms.append((t2 - t0) * 1e3); a_lin_ms.append((t1 - t0) * 1e3); a_set_ms.append((t2 - t1) * 1e3); b_ms.append((t3 - t2) * 1e3)
    equal = all(np.array_equal(A.get_table(t + 1), B.get_table(t + 1)) for t in range(N))
    out = {"leg": name, "model": model_name, "knots": int(N), "nz": int(z.shape[1]), "nth": int(th.shape[1]), "kappa": kappa,
           "table_doubles": int(A.query_sizes()[0]),
           "a_linearize_then_set_linearization_ms": stats(a_ms, calls, warmup), "a_plant_linearize_ms": stats(a_lin_ms, calls, warmup),
           "a_set_linearization_x_knots_ms": stats(a_set_ms, calls, warmup), "b_linearize_knots_ms": stats(b_ms, calls, warmup),
           "a_over_b": round(statistics.median(a_ms) / statistics.median(b_ms), 2), "tables_equal_bit_for_bit": bool(equal)}
    A.close(); B.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_build_ab.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "legs": [leg(*l, a.calls, a.warmup) for l in LEGS]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
