#!/usr/bin/env python3
"""What control limits cost, on the two legs of scripts/plant_gradients_ab.py (quadruped B 256 T 100,
centroidal_quadruped B 64 T 60), in ONE process, a host clock around whole calls (each ends in a stream synchronize), a warm call each,
then alternating turns; medians, minima and maxima.  Recorded, not asserted.

  existing paths against the parent   `--parent-lib PATH` (a build of the parent commit) and `--parent-copy PATH` (a copy of that file,
                                      loaded beside it: the A/A spread): the unchanged `lqr` with linear terms, `rollout(feedback=)` and
                                      `linesearch` (one step length) through this build, the parent and the parent's copy, each on a tape
                                      of its own build; their outputs are compared bit for bit
  new paths                           `lqr` with infinite limits and with binding limits against `lqr`; the limited closed loop against
                                      the unlimited one with the same K; the backward pass of an `ilqr` iteration with three rho levels in
                                      use: ONE launch with the rho array against one launch per level merged on the host
  the compiler's resource table       `--resources JSON`, made without a device by `--compile-resources` (hipcc -Rpass-analysis=
                                      kernel-resource-usage over plant_riccati.hip and plant_kernel.hip), is copied in as it stands

usage: python scripts/plant_boxqp_ab.py [--turns 3] [--parent-lib PATH --parent-copy PATH] [--resources JSON] [--figures-from LOG]
                                        [--out profiles/plant_boxqp.json]
       python scripts/plant_boxqp_ab.py --compile-resources OUT.json        (no device)"""
import argparse
import contextlib
import ctypes as C
import dataclasses
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CSRC = os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc")


def compile_resources(out):
    """VGPRs, SGPR spills, scratch, LDS and occupancy of every instantiation of the two kernels, as the compiler reports them."""
    table = {}
    for unit in ("plant_riccati.hip", "plant_kernel.hip"):
        res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "--cuda-device-only", "-S", "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage", unit], cwd=CSRC, capture_output=True, text=True, check=True)
        cur = None
        for line in res.stderr.splitlines():
            m = re.search(r"remark: \s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key == "Function Name":
                cur = re.sub(r"\(.*", "", subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip()).replace("void cimpc::", "")
                table[cur] = {}
            elif cur and key in ("VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size"):
                table[cur][key] = int(val)
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("wrote", out)


def bound_library(path):
    """Another build of the library with the signatures it has."""
    from contactimplicitmpc.jl_amd import _lib
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


@contextlib.contextmanager
def using(lib):
    """`plant`'s calls go to `lib` inside the block."""
    from contactimplicitmpc.jl_amd import _lib
    mine = _lib.load()
    _lib._lib = lib
    try:
        yield
    finally:
        _lib._lib = mine


def timed(runs, turns):
    outs = {k: f() for k, f in runs.items()}      # warm-up, and the outputs side by side
    times = {k: [] for k in runs}
    for _ in range(turns):
        for k, f in runs.items():
            t0 = time.perf_counter(); f(); times[k].append((time.perf_counter() - t0) * 1e3)
    return outs, times


def leg(name, model, gait_file, B, T, turns, builds):
    from contactimplicitmpc.jl_amd import plant
    from plant_adjoint_ab import leg_inputs
    from plant_gradients_ab import summary
    import plant_gradient_cases as pgc
    import plant_riccati_cases as prc
    g, q1, v1, u = leg_inputs(model, gait_file, B, T)
    nq, nu = pgc.dims(model)[:2]
    n = 2 * nq
    rng = np.random.default_rng(0)
    Q, R, Qf = prc.weights(rng, n, nu)
    res = {"leg": name, "model": model, "B": B, "T": T}
    state = {}
    for tag, lib in builds.items():      # a nominal, its tape, cost terms and unlimited gains per build, each through its own library
        with using(lib):
            ok, q, ua, gamma, b, status, iters, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
            x = np.concatenate([q[:-1], q[1:]], axis=2)
            cost = plant.TrackingCost(Q, 0.01 * R, Qf, x_goal=x + 0.02 * np.random.default_rng(1).standard_normal(x.shape), u_goal=ua * 0.5)
            J, lq, lr = cost.evaluate(q, ua)
            gains = tape.lqr(Q, 0.01 * R, Qf, q=lq, r=lr, rho=1e-3)
            state[tag] = dict(tape=tape, q=q, ua=ua, cost=cost, J=J, lq=lq, lr=lr, gains=gains, fb=gains.feedback(q))
    R = 0.01 * R

    def existing(tag):
        s, lib = state[tag], builds[tag]

        def lqr():
            with using(lib):
                return s["tape"].lqr(Q, R, Qf, q=s["lq"], r=s["lr"], rho=1e-3)

        def closed():
            with using(lib):
                return plant.rollout(model, q1, v1, s["ua"] + 0.5 * s["gains"].k, g.h, g.mu, feedback=s["fb"])

        def search():
            with using(lib):
                ls = s["tape"].linesearch(s["gains"], s["q"], s["ua"], s["cost"], s["J"], (0.5,))
                ls.tape.close()
                return ls
        return {f"lqr[{tag}]": lqr, f"rollout_feedback[{tag}]": closed, f"linesearch[{tag}]": search}
    runs = {}
    for tag in builds:
        runs.update(existing(tag))
    # the new paths, this build only
    s = state["this"]
    tape, ua, gains = s["tape"], s["ua"], s["gains"]
    inf = np.full(nu, np.inf)
    bound = 0.5 * np.abs(ua + gains.k).max(axis=(0, 1))      # half of the largest control the unlimited full step asks for, per control
    lo, hi = np.minimum(-bound, ua.min(axis=(0, 1))), np.maximum(bound, ua.max(axis=(0, 1)))      # the nominal stays inside
    levels = 1e-3 * 10.0 ** (np.arange(B) % 3)

    def per_level():
        Kb, k, dV = np.zeros((T, B, n, nu)), np.zeros((T, B, nu)), np.zeros((B, 2))
        for val in np.unique(levels):
            rows = levels == val
            one = tape.lqr(Q, R, Qf, q=s["lq"], r=s["lr"], rho=float(val))
            Kb[:, rows], k[:, rows], dV[rows] = one.K_blocks[:, rows], one.k[:, rows], one.dV[rows]
        return Kb, k, dV
    limited_fb = dataclasses.replace(s["fb"], u_lo=lo, u_hi=hi)
    runs.update({"lqr_infinite_limits": lambda: tape.lqr(Q, R, Qf, q=s["lq"], r=s["lr"], rho=1e-3, u_lo=-inf, u_hi=inf, u_nom=ua),
                 "lqr_binding_limits": lambda: tape.lqr(Q, R, Qf, q=s["lq"], r=s["lr"], rho=1e-3, u_lo=lo, u_hi=hi, u_nom=ua),
                 "rollout_feedback_limited": lambda: plant.rollout(model, q1, v1, ua + 0.5 * gains.k, g.h, g.mu, feedback=limited_fb),
                 "backward_pass_three_rho_levels_one_launch": lambda: tape.lqr(Q, R, Qf, q=s["lq"], r=s["lr"], rho=levels),
                 "backward_pass_three_rho_levels_a_launch_each": per_level})
    outs, times = timed(runs, turns)
    for st in state.values():
        st["tape"].close()
    med = {k: summary(v)["median_ms"] for k, v in times.items()}
    res["time"] = {k: summary(v) for k, v in times.items()}
    same = lambda a, b: bool(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes())
    if "parent" in builds:
        res["existing_paths"] = {}
        for path in ("lqr", "rollout_feedback", "linesearch"):
            a, p = outs[f"{path}[this]"], outs[f"{path}[parent]"]
            eq = (same(a.K, p.K) and same(a.k, p.k) and same(a.P0, p.P0)) if path == "lqr" else (same(a[1], p[1]) and same(a[2], p[2])) if path == "rollout_feedback" \
                else (same(a.J, p.J) and same(a.q, p.q) and same(a.u_applied, p.u_applied))
            row = {"this_over_parent": round(med[f"{path}[this]"] / med[f"{path}[parent]"], 4), "outputs_equal_the_parents_bit_for_bit": eq}
            if "parent_copy" in builds:
                row["parent_copy_over_parent"] = round(med[f"{path}[parent_copy]"] / med[f"{path}[parent]"], 4)
            res["existing_paths"][path] = row
    full = outs["lqr_binding_limits"]
    res["new_paths"] = {
        "lqr_infinite_limits_over_lqr": round(med["lqr_infinite_limits"] / med["lqr[this]"], 4),
        "lqr_binding_limits_over_lqr": round(med["lqr_binding_limits"] / med["lqr[this]"], 4),
        "lqr_infinite_limits_equals_lqr_bit_for_bit": same(outs["lqr_infinite_limits"].K, outs["lqr[this]"].K) and same(outs["lqr_infinite_limits"].k, outs["lqr[this]"].k),
        "binding_limits_clamped_step_controls": int(sum(bin(int(v)).count("1") for v in full.clamped.ravel())), "of": T * B * nu,
        "binding_limits_robots_whose_chain_ended": int((full.status != 0).sum()),
        "rollout_feedback_limited_over_unlimited": round(med["rollout_feedback_limited"] / med["rollout_feedback[this]"], 4),
        "limited_closed_loop_controls_on_a_bound": int(((outs["rollout_feedback_limited"][2] == lo) | (outs["rollout_feedback_limited"][2] == hi)).sum()),
        "one_launch_over_a_launch_per_level": round(med["backward_pass_three_rho_levels_one_launch"] / med["backward_pass_three_rho_levels_a_launch_each"], 4),
        "one_launch_equals_the_merged_rows_bit_for_bit": same(outs["backward_pass_three_rho_levels_one_launch"].K_blocks, outs["backward_pass_three_rho_levels_a_launch_each"][0])}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, metavar="PATH", help="libcimpc_hip.so of the parent commit")
    ap.add_argument("--parent-copy", default=None, metavar="PATH", help="a copy of it, for the A/A spread")
    ap.add_argument("--resources", default=None, metavar="JSON", help="the table --compile-resources wrote")
    ap.add_argument("--compile-resources", default=None, metavar="OUT", help="write the compiler's resource table and stop (no device)")
    ap.add_argument("--figures-from", default=None, metavar="LOG", help="a `pytest -s` log of tests/test_gpu_plant_boxqp.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_boxqp.json"))
    a = ap.parse_args()
    if a.compile_resources:
        return compile_resources(a.compile_resources)
    import torch                                                    # the device comes up through torch first, as in the tests
    from contactimplicitmpc.jl_amd import _lib
    from plant_gradients_ab import LEGS
    assert torch.cuda.is_available(), "needs a GPU"
    builds = {"this": _lib.load()}
    if a.parent_lib:
        builds["parent"] = bound_library(a.parent_lib)
    if a.parent_copy:
        builds["parent_copy"] = bound_library(a.parent_copy)
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "date": time.strftime("%Y-%m-%d"),
           "method": "host clock around whole calls, medians of alternating turns after a warm call, one process",
           "legs": [leg(*l, a.turns, builds) for l in LEGS]}
    if a.resources:
        res["kernel_resources_gfx950"] = json.load(open(a.resources))
    if a.figures_from:
        keep = re.compile(r"clamped \[|on a bound|projected gradient|limited hoppers")
        res["figures_of_tests_test_gpu_plant_boxqp"] = [line.strip().lstrip(".") for line in open(a.figures_from) if keep.search(line)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
