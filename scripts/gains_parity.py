#!/usr/bin/env python3
"""Device feedback gains against the NumPy restatement of gains.jl on the shipped gaits (the cases of tests/gains_cases.py, which
tests/test_gpu_gains.py asserts at 1e-9): max|K_dev - K_ref| / max|K_ref| and the same for P1, for the entry that takes a
linearization (`reference_gains_lin`, torch tables) and the one that linearizes on the device (`reference_gains`).
usage: python scripts/gains_parity.py [--out profiles/gains_parity.json]
       python scripts/gains_parity.py --edges [--out profiles/gains_parity_edges.json]
--edges: the synthetic edge cases of tests/gains_edge_cases.py (which tests/test_gpu_gains_edges.py asserts) against the longdouble solve:
per case the device's distances, the two float64 restatements' own distances to the longdouble solve, and the bound derived from them."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from contactimplicitmpc.jl_amd import gains  # noqa: E402
import gains_cases as gc  # noqa: E402


def edges(out):
    import gains_edge_cases as ec
    rows = []
    for name in ec.LIN_NAMES:
        c = ec.lin_case(name)
        K, P1 = gains.reference_gains_lin(c["nq"], c["nu"], c["rz0"], c["rth0"], *c["weights"], N=c["N"], return_P1=True)
        rows.append(dict(case=name, entry="reference_gains_lin", lds_bytes=8 * (c["nz"] ** 2 + c["nz"] * c["nq"] + c["nz"] + 2),
                         K_dev=ec._rel(K, c["K_ld"]), P1_dev=ec._rel(P1, c["P1_ld"]),
                         K_direct=c["d_direct"][0], P1_direct=c["d_direct"][1], K_adjoint=c["d_adjoint"][0], P1_adjoint=c["d_adjoint"][1],
                         K_bound=ec.bound(c["d_direct"][0], c["d_adjoint"][0]), P1_bound=ec.bound(c["d_direct"][1], c["d_adjoint"][1])))
        print(rows[-1])
    singles = [(name, ec.tvlqr_case(name), None) for name in ec.TVLQR_NAMES]
    batches = [("batch of 3, n_q = T, n_keep = 4", ec.batch_case("3"), ec.BATCH_3_KEEP), ("batch of 300", ec.batch_case("300"), None)]
    for name, c, keep in singles + batches:
        Q = c["Q"] if c["Q"].shape[1] > 1 or c["R"].shape[1] > 1 else np.repeat(c["Q"], c["T"], axis=1)      # T = 2: something must carry the horizon
        K, P1 = gains.tvlqr(c["A"], c["B"], Q, c["R"], n_keep=keep)
        n_prob = K.shape[0]
        d = np.array([(ec._rel(K[p], c["K_ld"][p, :K.shape[1]]), ec._rel(P1[p], c["P1_ld"][p])) for p in range(n_prob)])
        b = np.array([(ec.bound(x), ec.bound(y)) for x, y in c["d_f64"]])
        w = [int(np.argmax(d[:, i] / b[:, i])) for i in range(2)]      # per figure, the problem closest to its bound
        rows.append(dict(case=name, entry="tvlqr", n_prob=n_prob, K_dev=d[w[0], 0], P1_dev=d[w[1], 1], K_direct=c["d_f64"][w[0], 0],
                         P1_direct=c["d_f64"][w[1], 1], K_bound=b[w[0], 0], P1_bound=b[w[1], 1]))
        print(rows[-1])
    doc = dict(what="max|x - longdouble solve| / max|longdouble solve| of K and P[1] on the synthetic edge cases: _dev the device, _direct and "
                    "_adjoint the float64 restatements (tvlqr has one); _bound = min(1e-9, 100 max(_direct, _adjoint, 2.2e-16)), what the "
                    "tests assert of _dev.  A batch's row is the problem closest to its bound.", cases=rows)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    bad = [r["case"] for r in rows if r["K_dev"] > r["K_bound"] or r["P1_dev"] > r["P1_bound"]]
    print("over the bound:", bad or "none")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", action="store_true", help="the synthetic edge cases against the longdouble solve")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.edges:
        return edges(a.out or os.path.join(ROOT, "profiles", "gains_parity_edges.json"))
    a.out = a.out or os.path.join(ROOT, "profiles", "gains_parity.json")
    rel = lambda x, ref: float(np.abs(x - ref).max() / np.abs(ref).max())
    rows = []
    for name in gc.CASES:
        c = gc.case(name)
        m = c["model"]
        K_lin, P_lin = gains.reference_gains_lin(m.nq, m.nu, c["rz0"], c["rth0"], *c["weights"], N=c["N"], return_P1=True)
        K_dev, P_dev = gains.reference_gains(m.name, c["z"], c["theta"], *c["weights"], N=c["N"], return_P1=True)
        rows.append(dict(case=name, model=m.name, knots=int(c["z"].shape[0]), N=int(c["N"]), nz=int(m.nz), n=2 * int(m.nq), m=int(m.nu),
                         max_abs_K_ref=float(np.abs(c["K"]).max()), max_abs_P1_ref=float(np.abs(c["P1"]).max()),
                         K_lin=rel(K_lin, c["K"]), P1_lin=rel(P_lin, c["P1"]), K_dev=rel(K_dev, c["K"]), P1_dev=rel(P_dev, c["P1"])))
        print(rows[-1])
    doc = dict(what="max|device - NumPy restatement| / max|restatement| of the feedback gains K[1:H] and of P[1]; _lin: from the torch "
                    "linearization, _dev: linearized on the device from (z, theta)", tolerance_of_the_tests=gc.TOL, cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
