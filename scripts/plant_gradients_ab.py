#!/usr/bin/env python3
"""What the step gradients cost: `plant.rollout(..., diff_sol=True)` (`cimpc_plant_rollout_grad`) against `plant.rollout` of this build
and of another build of the library (`--parent-lib PATH`, a build of the parent commit), and against the unfused composition - the
rollout, then `plant.linearize` at every step's (z, θ) with both Jacobians read back, the regularization and `numpy.linalg.solve` on
the host; the z comes from a `diff_sol=True` call made beforehand, since nothing else returns it.  One GPU, one process, warm calls,
alternating turns, a host clock around calls that end in the stream synchronize; medians over `--turns` turns (at least 20).

Legs: the open-loop replay of quadruped gait2 (B = 256 robots started at knots spread over the gait, T = 100) and of the centroidal
quadruped's in-place trot (B = 64, T = 60).  Also recorded: the parity figures of tests/test_gpu_plant_gradients.py (synthetic knots
and the rollout cases) with their bounds.
usage: python scripts/plant_gradients_ab.py [--turns 20] [--parent-lib PATH] [--out profiles/plant_gradients.json]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from contactimplicitmpc.jl_amd import _lib, gait_io, plant  # noqa: E402

GAITS = os.path.join(ROOT, "tests", "golden", "gaits")
LEGS = (("quadruped gait2 replay", "quadruped", "quadruped_gait2", 256, 100), ("centroidal in-place trot replay", "centroidal_quadruped", "centroidal_inplace_trot_v7", 64, 60))


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "turns": len(ms)}


def parent_rollout(lib, model, q1, v1, u, h, mu):
    """`cimpc_plant_rollout` of another build, with the arguments `plant.rollout` passes"""
    mid, nq, nu, nc, fd, nw = plant.model_dims(model)
    T, B = u.shape[0], q1.shape[0]
    q0 = np.ascontiguousarray(q1 - h * v1)
    q = np.zeros((T + 2, B, nq)); g = np.zeros((T, B, nc)); b = np.zeros((T, B, fd * nc))
    st = np.zeros((T, B), dtype=np.int32); it = np.zeros((T, B), dtype=np.int32)
    o = _lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS))
    mua = np.array([float(mu)])
    dp = lambda a: a.ctypes.data_as(_lib._dp)
    ip = lambda a: a.ctypes.data_as(_lib._ip)

    def call():
        rc = lib.cimpc_plant_rollout(mid, B, T, 0, 0, None, dp(q0), dp(q1), dp(u), u.shape[0], u.shape[1], 1, None, 1, 1, 1, dp(mua), 1, float(h),
                                     C.byref(o), dp(q), dp(g), dp(b), ip(st), ip(it))
        if rc != 0:
            raise _lib.CimpcError(f"cimpc_plant_rollout of the parent build failed ({rc})")
        return q, g, b, st, it
    return call


def leg(name, model, gait_file, B, T, turns, parent):
    import plant_gradient_cases as pgc
    g = gait_io.load_gait(os.path.join(GAITS, gait_file + ".jld2"))
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(model)
    k = np.arange(B) * g.H // B
    q1, v1 = np.ascontiguousarray(g.q[k + 1]), (g.q[k + 1] - g.q[k]) / g.h
    u = np.ascontiguousarray(np.stack([g.u[(k + t) % g.H] for t in range(T)]))
    n_cols = 2 * nq + nu
    plain = lambda: plant.rollout(model, q1, v1, u, g.h, g.mu)
    grad = lambda: plant.rollout(model, q1, v1, u, g.h, g.mu, diff_sol=True)
    ok, q, ua, gam, b, st, it, G = grad()
    Z = G.z.reshape(T * B, nz)

    def composition():
        """the gradients without the fused kernel, at the z of the earlier call: θ on the host, both Jacobians of every step read back
        from `plant.linearize`, then the definition in NumPy (LAPACK, batched)"""
        ok2, q2, ua2, *_ = plain()
        TH = np.concatenate([q2[:-2], q2[1:-1], ua2, np.zeros((T, B, nw)), np.full((T, B, 1), g.mu), np.full((T, B, 1), g.h)], axis=2).reshape(T * B, nth)
        _, rz, rth = plant.linearize(model, Z, TH, 0.0)
        ny, i = 2 * nc + nb, np.arange(2 * nc + nb)
        rz[:, nq + ny + i, nq + i] = np.maximum(Z[:, nq + ny + i], pgc.REG)
        rz[:, nq + ny + i, nq + ny + i] = np.maximum(Z[:, nq + i], pgc.REG)
        return np.linalg.solve(rz, -rth[:, :, :n_cols])[:, :nr].reshape(T, B, nr, n_cols)

    runs = {"rollout": plain, "rollout_diff_sol": grad, "composition": composition}
    if parent is not None:
        runs["rollout_parent_build"] = parent_rollout(parent, model, q1, v1, u, g.h, g.mu)
    outs = {n: f() for n, f in runs.items()}                        # warm-up, and the outputs side by side
    times = {n: [] for n in runs}
    for _ in range(turns):
        for n, f in runs.items():
            t0 = time.perf_counter(); f(); times[n].append((time.perf_counter() - t0) * 1e3)
    done = G.status == 1
    scale = np.abs(G.dz).max(axis=(2, 3))
    dev = np.abs(outs["composition"] - G.dz).max(axis=(2, 3)) / np.where(scale > 0, scale, 1.0)
    res = {"leg": name, "model": model, "B": B, "T": T, "n_cols": n_cols, "steps_converged": int(st.sum()), "steps_differentiated": int(done.sum()),
           "time": {n: summary(v) for n, v in times.items()},
           "rollout_unchanged_by_diff_sol": all(np.array_equal(x, y) for x, y in zip(outs["rollout"][1:], outs["rollout_diff_sol"][1:7])),
           "composition_vs_fused_max_rel_over_differentiated_steps": float(dev[done].max()) if done.any() else None,
           "composition_vs_fused_median_rel": float(np.median(dev[done])) if done.any() else None}
    med = lambda n: res["time"][n]["median_ms"]
    res["diff_sol_over_rollout_this_build"] = round(med("rollout_diff_sol") / med("rollout"), 4)
    res["composition_over_diff_sol"] = round(med("composition") / med("rollout_diff_sol"), 3)
    if parent is not None:
        res["rollout_identical_to_parent_build"] = all(np.array_equal(x, y) for x, y in zip(outs["rollout"][1:2] + outs["rollout"][3:], outs["rollout_parent_build"]))
        res["diff_sol_over_rollout_parent_build"] = round(med("rollout_diff_sol") / med("rollout_parent_build"), 4)
        res["rollout_this_over_parent_build"] = round(med("rollout") / med("rollout_parent_build"), 4)
    print(json.dumps(res), flush=True)
    return res


def parity():
    """the figures of tests/test_gpu_plant_gradients.py, tests 1 and 2: per case the worst device distance to the longdouble solve, the
    bound of the entry where it is closest to its bound, and the references' own worst distance"""
    import plant_gradient_cases as pgc
    import plant_linearize_cases as plc
    out = []

    def record(case, devs, refs):
        d = [pgc.rel(x, r["ld"]) for x, r in zip(devs, refs)]
        i = int(np.argmax([a / r["bound"] for a, r in zip(d, refs)]))
        out.append({"case": case, "entries": len(d), "worst_device": max(d), "closest_to_its_bound": {"device": d[i], "bound": refs[i]["bound"]},
                    "worst_reference": max(max(r["d_lapack"], r["d_order"]) for r in refs), "largest_cond_R": max(r["cond"] for r in refs),
                    "all_within_bound": all(a <= r["bound"] for a, r in zip(d, refs))})
    for reg in pgc.REGS:
        for name, mid in pgc.FLAT_CASES:
            z, th, refs = pgc.flat_case(mid, reg)
            dz, st = plant.sensitivity(name, z, th, reg, n_cols=th.shape[1])
            record(f"{name} reg={reg:g}", list(dz), refs)
        for model, mid, ter in plc.TERRAIN_CASES:
            z, th, refs = pgc.terrain_case(model, mid, ter, reg)
            dz, st = plant.sensitivity(model, z, th, reg, n_cols=th.shape[1], terrain=ter)
            record(f"{model} on {ter} reg={reg:g}", list(dz), refs)
    for which in pgc.ROLLOUTS:
        c = pgc.rollout_case(which)
        ok, q, ua, gam, b, st, it, G = plant.rollout(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], terrain=c["terrain"], diff_sol=True)
        T, B = st.shape
        TH = np.array([[pgc.step_theta(c, q, ua, t, r) for r in range(B)] for t in range(T)])
        refs = pgc.rollout_references(c, G.z, TH, pgc.REG, G.dz.shape[3])
        record(f"rollout {which} (T={T}, B={B})", list(G.dz.reshape(T * B, *G.dz.shape[2:])), list(refs.ravel()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, metavar="PATH", help="libcimpc_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_gradients.json"))
    a = ap.parse_args()
    assert a.turns >= 20, "medians of at least 20 turns"

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.cimpc_plant_rollout.restype, parent.cimpc_plant_rollout.argtypes = _lib.SIGNATURES["cimpc_plant_rollout"]
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "parent_build_measured": parent is not None,
           "legs": [leg(*l, a.turns, parent) for l in LEGS], "parity": parity()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
