#!/usr/bin/env python3
"""Device feedback gains against the NumPy restatement of gains.jl on the shipped gaits (the cases of tests/gains_cases.py, which
tests/test_gpu_gains.py asserts at 1e-9): max|K_dev - K_ref| / max|K_ref| and the same for P1, for the entry that takes a
linearization (`reference_gains_lin`, torch tables) and the one that linearizes on the device (`reference_gains`).
usage: python scripts/gains_parity.py [--out profiles/gains_parity.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gains_parity.json"))
    a = ap.parse_args()
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
    main()
