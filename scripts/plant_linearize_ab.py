#!/usr/bin/env python3
"""`plant.linearize` (the linearization tables of every knot from one device call) against `ContactModel.linearize_batch` (torch.func on
the host) on the same inputs: the knots of quadruped gait2 (60 knots, 77 Jacobian columns each) and of wall_stand_FL_4
(centroidal_quadruped_wall, 50 knots, 167 columns).  Per leg: the median wall time of `--calls` `plant.linearize` calls after `--warmup`
warm-up calls (a host clock around calls that end in the stream synchronize; the time includes the upload, the read-back and the
transposes to row-major), the host's first call (tracing included) and second call, and the largest deviation of each device table
from the torch one, absolute and relative to the table's largest |entry|.
usage: python scripts/plant_linearize_ab.py [--calls 20] [--warmup 3] [--out profiles/plant_linearize.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from contactimplicitmpc.jl_amd import gait_io, lcp_models, plant  # noqa: E402

GAITS = os.path.join(ROOT, "tests", "golden", "gaits")
LEGS = (("quadruped gait2", "quadruped", "quadruped_gait2", 1e-4), ("wall_stand_FL_4", "centroidal_quadruped_wall", "wall_stand_FL_4", 1e-3))


def leg(name, model_name, gait_file, kappa, calls, warmup):
    model = lcp_models.MODELS[model_name]()
    grabbed = {}

    def grab(z, th, k):                     # the stacked knots `reference_problem` linearizes, and the host's first call on them
        grabbed["z"], grabbed["th"] = z, th
        t0 = time.perf_counter()
        out = model.linearize_batch(z, th, k)
        grabbed["first_ms"] = (time.perf_counter() - t0) * 1e3
        return out
    lcp_models.reference_problem(model, gait_io.load_gait(os.path.join(GAITS, gait_file + ".jld2")), kappa, linearize=grab)
    z, th = grabbed["z"], grabbed["th"]
    t0 = time.perf_counter()
    ref = model.linearize_batch(z, th, kappa)
    host_second_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(warmup):
        got = plant.linearize(model_name, z, th, kappa)
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        got = plant.linearize(model_name, z, th, kappa)
        ms.append((time.perf_counter() - t0) * 1e3)
    dev = {k: {"max_abs_entry": float(np.abs(w).max()), "max_deviation": float(np.abs(g - w).max()),
               "relative": float(np.abs(g - w).max() / max(1.0, np.abs(w).max()))} for k, g, w in zip(("r0", "rz0", "rth0"), got, ref)}
    out = {"leg": name, "model": model_name, "knots": int(z.shape[0]), "nz": int(z.shape[1]), "nth": int(th.shape[1]), "kappa": kappa,
           "device_ms": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls": calls, "warmup": warmup},
           "host_linearize_batch_ms": {"first_call": round(grabbed["first_ms"], 2), "second_call": round(host_second_ms, 2)},
           "host_second_over_device": round(host_second_ms / statistics.median(ms), 1), "device_against_torch": dev}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_linearize.json"))
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
