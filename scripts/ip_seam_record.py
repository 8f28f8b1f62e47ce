"""Records the figures of tests/test_gpu_ip_seam.py on one MI355X to profiles/ip_seam.json (tests/README_ip_seam.md quotes them).

Runs the test file in THIS process (`pytest.main`), then writes what the tests left in their RECORD once, with the reference figures
of the cases beside them.  Where :configurationforce mode gave the figures of :configuration mode, only the latter are kept.

    python scripts/ip_seam_record.py [--out profiles/ip_seam.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_seam.json"))
    args = ap.parse_args()
    import pytest
    t0 = time.perf_counter()
    rc = int(pytest.main([os.path.join(ROOT, "tests", "test_gpu_ip_seam.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"]))
    seconds = time.perf_counter() - t0
    rec = dict(sys.modules["test_gpu_ip_seam"].RECORD)
    cases = sys.modules["ip_seam_cases"]
    same_modes = []
    for key in sorted(k for k in rec if k.startswith("a/") and k.endswith("/mode1")):
        if rec[key] == rec.get(key[:-1] + "0"):
            del rec[key]
            same_modes.append(key[2:-6])
    out = dict(pytest_exit=rc, seconds=round(seconds, 1), point_seed=cases.POINT_SEED, n_noise=cases.N_NOISE,
               mode1_figures_equal_mode0=same_modes, figures=rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {args.out}: {len(rec)} entries, pytest exit {rc}, {seconds:.1f} s")
    return rc


if __name__ == "__main__":
    sys.exit(main())
