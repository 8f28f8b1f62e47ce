#!/usr/bin/env python3
"""`plant.rollout` (T plant steps in one call) against the host loop of `plant.plant_step`, and `plant_step` itself against other
builds of the library, on one GPU in one process: alternating pairs, a host clock around calls that end in the stream synchronize.

Rollout legs: the open-loop replay of quadruped gait2 (mu 0.5, T = H steps) and of hopper_3D gait_in_place (T = H steps), every robot
from the gait's own start, B in {4, 64, 512}; per pair the loop's and the rollout's wall time per step, whose outputs are compared
bit for bit once per leg.  Step legs (`step_legs`): one `plant_step` call per leg, a table that reaches every kernel instantiation and
every residual of plant_model.h on flat ground and on terrain, this build against every `--step-lib NAME=PATH` (e.g. a build of the
parent commit, and a copy of it for the spread of a build against itself), alternating per pair; the small models (B = 16) are
compared only, not timed.  `--parent-step-us LEG=US` records a figure measured elsewhere next to them; `--legs TEXT ...` keeps the
step legs whose name contains one of the texts.  The rollout legs also run `rollout` on every `--step-lib`, timed and compared.
Kernel legs (`--kernels`, `kernel_legs`): the other plant-side entry points on every library - `linearize`, `sensitivity`, `reference_gains`,
`reference_gains_lin`, `tvlqr` and `rollout(diff_sol=True)` - compared with `np.array_equal` at small shapes (3 knots per model, a flat
knot inside every terrain batch, n_cols = 1 and nθ, the two smallest cases of tests/gains_cases.py) and, with `--pairs` > 0, timed at
the shapes of plant_linearize_ab.py, gains_ab.py and plant_gradients_ab.py.  With libraries named `parent` and `parent_copy` the
result ends with `ratios`: per timed leg this build over the parent and the parent's copy over the parent (medians).
usage: python scripts/plant_rollout_ab.py [--pairs 5] [--calls 100] [--step-lib NAME=PATH ...] [--parent-step-us LEG=US ...]
                                          [--legs TEXT ...] [--no-rollout] [--no-step] [--kernels] [--out profiles/plant_rollout_ab.json]"""
import argparse
import contextlib
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
from contactimplicitmpc.jl_amd import _lib, gains, gait_io, plant  # noqa: E402

GAITS = os.path.join(ROOT, "tests", "golden", "gaits")
BATCHES = (4, 64, 512)


def summary(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "pairs_us": [round(v, 2) for v in us]}


@contextlib.contextmanager
def bound(lib):
    """the Python wrappers (`plant`, `gains`) on another build: they take their library from `_lib.load()`"""
    keep, _lib._lib = _lib._lib, lib
    try:
        yield
    finally:
        _lib._lib = keep


def on(lib, fn, *args, **kw):
    with bound(lib):
        return fn(*args, **kw)


def same(x, y):
    """two results of one wrapper (an array, or a tuple of arrays and plain values) bit for bit"""
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same(a, b) for a, b in zip(x, y))
    if isinstance(x, plant.StepGradients):
        return same((x.dz, x.z, x.status), (y.dz, y.z, y.status))
    return bool(np.array_equal(np.asarray(x), np.asarray(y)))


def rollout_leg(name, model, q0, q1, u, h, mu, B, pairs, libs):
    """u (T, nu) shared by B identical robots: per pair, the loop of T `plant_step` calls and ONE `rollout`, us per step each; then ONE
    `rollout` per library and pair"""
    T = u.shape[0]
    q1b, v1b = np.tile(q1, (B, 1)), np.tile((q1 - q0) / h, (B, 1))
    ub = np.ascontiguousarray(np.broadcast_to(u[:, None, :], (T, B, u.shape[1])))

    def loop():
        q = [q1b - h * v1b, q1b]
        ok = True
        for t in range(T):
            q2, g, b, st, it = plant.plant_step(model, q[t], q[t + 1], ub[t], mu, h)
            ok = ok and bool(st.all())
            q.append(q2)
        return ok, np.array(q)

    roll = lambda: plant.rollout(model, q1b, v1b, u, h, mu)
    (ok_l, q_l), first = loop(), roll()                              # warm-up, and the outputs side by side
    ok_r, q_r = first[:2]
    t_loop, t_roll = [], []
    for _ in range(pairs):
        t0 = time.perf_counter(); loop(); t1 = time.perf_counter(); roll(); t2 = time.perf_counter()
        t_loop.append((t1 - t0) / T * 1e6); t_roll.append((t2 - t1) / T * 1e6)
    t_lib = {k: [] for k in libs}
    identical = {k: same(on(lib, roll), first) for k, lib in libs.items() if k != "this"}
    for _ in range(pairs if len(libs) > 1 else 0):                   # the rollout alone, alternating over the libraries
        for k, lib in libs.items():
            t0 = time.perf_counter(); on(lib, roll); t_lib[k].append((time.perf_counter() - t0) / T * 1e6)
    out = {"leg": name, "model": model, "B": B, "T": T, "all_steps_converged": bool(ok_l and ok_r), "identical_q": bool(np.array_equal(q_l, q_r)),
           "loop_per_step": summary(t_loop), "rollout_per_step": summary(t_roll), "rollout_per_step_on": {k: summary(v) for k, v in t_lib.items() if v},
           "identical_rollout_on": identical}
    out["rollout_over_loop"] = round(out["rollout_per_step"]["median_us"] / out["loop_per_step"]["median_us"], 4)
    print(json.dumps(out), flush=True)
    return out


def step_leg(name, model, q0, q1, u, h, mu, libs, pairs, calls, terrain=None):
    """one `cimpc_plant_step` call (`cimpc_plant_step_terrain` on a terrain name) on every library in turn, `calls` calls per turn,
    `pairs` turns: us per call; pairs = 0 only compares the outputs"""
    mid, nq, nu, nc, fd, nw = plant.model_dims(model)
    B = q0.shape[0]
    q0, q1, u = (np.ascontiguousarray(a, dtype=np.float64) for a in (q0, q1, u))
    q2 = np.zeros((B, nq)); g = np.zeros((B, nc)); b = np.zeros((B, fd * nc)); st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
    o = _lib.IpOpts(**dataclasses.asdict(plant.SIM_OPTS))
    dp = lambda a: a.ctypes.data_as(_lib._dp)
    ip = lambda a: a.ctypes.data_as(_lib._ip)
    ta, nt = (None, 0) if terrain is None else plant._terrain_array(terrain, B)

    def call(lib):
        out = (dp(q0), dp(q1), dp(u), None, float(mu), float(h), C.byref(o), dp(q2), dp(g), dp(b), ip(st), ip(it))
        rc = lib.cimpc_plant_step(mid, B, *out) if terrain is None else lib.cimpc_plant_step_terrain(mid, B, nt, ta, *out)
        if rc != 0:
            raise _lib.CimpcError(f"plant step of leg {name} failed ({rc})")

    results, outputs = {k: [] for k in libs}, {}
    for k, lib in libs.items():                                     # warm-up, and the outputs side by side
        for _ in range(3):
            call(lib)
        outputs[k] = (q2.copy(), g.copy(), b.copy(), st.copy(), it.copy())
    for _ in range(pairs):
        for k, lib in libs.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                call(lib)
            results[k].append((time.perf_counter() - t0) / calls * 1e6)
    first = outputs["this"]
    out = {"leg": name, "model": model, "terrain": terrain, "B": B, "calls_per_turn": calls, "ip_iterations_per_robot": round(float(first[4].mean()), 2),
           "all_converged": bool(first[3].all()), "per_call": {k: summary(v) for k, v in results.items()} if pairs else None,
           "identical_outputs": {k: all(np.array_equal(x, y) for x, y in zip(first, v)) for k, v in outputs.items() if k != "this"}}
    print(json.dumps(out), flush=True)
    return out


def walled_inputs(model, B, h, seed=0):
    """pushbot / walledcartpole around their walls, as tests/walled_ref.py draws them: θ ~ U(-0.4, 0.4) with the arm's tip at
    x ~ U(-0.52, 0.52), or θ ~ U(-0.7, 0.7), x ~ U(-0.1, 0.1), wall offsets ~ U(-0.01, 0.01); v, u ~ U(-1, 1), q0 = q1 - h v"""
    rng = np.random.default_rng(seed)
    if model == "pushbot":
        th, x = rng.uniform(-0.4, 0.4, B), rng.uniform(-0.52, 0.52, B)
        q1 = np.stack([th, (x + np.sin(th)) / np.cos(th)], -1)
    else:
        q1 = np.stack([rng.uniform(-0.7, 0.7, B), rng.uniform(-0.1, 0.1, B), rng.uniform(-0.01, 0.01, B), rng.uniform(-0.01, 0.01, B)], -1)
    v = rng.uniform(-1.0, 1.0, q1.shape)
    return q1 - h * v, q1, rng.uniform(-1.0, 1.0, (B, plant.model_dims(model)[2]))


def step_legs(libs, pairs, calls, only=()):
    """quadruped, centroidal, box and wall at B = 256 and hopper_3D at B = 512, at knots spread over their gaits; the quadruped on
    terrain as tests/test_gpu_terrain.py places it (x over [0, 2.5], lifted by the height under the hip, h / 5), hopper_3D on the
    sine as tests/test_gpu_hopper_3d.py does; the small models at B = 16 with the inputs of the terrain tests, outputs only; pushbot
    and walledcartpole at B = 512 and 8192 around their walls (`walled_inputs`)"""
    from contactimplicitmpc.jl_amd import terrain
    gait = lambda f: gait_io.load_gait(os.path.join(GAITS, f + ".jld2"))
    knots = lambda g, B: np.arange(B) * g.H // B
    def leg(name, model, q0, q1, u, h, mu, n=calls, ter=None, timed=True):
        if only and not any(t in name for t in only):
            return None
        return step_leg(name, model, q0, q1, u, h, mu, libs, pairs if timed else 0, n, ter)
    out = []
    for model, mu in (("pushbot", 0.5), ("walledcartpole", 0.1)):
        for B in (512, 8192):
            out.append(leg(f"{model}{B}", model, *walled_inputs(model, B, 0.02), 0.02, mu, calls if B == 512 else max(10, calls // 5)))
    fwd = gait_io.load_joint_traj(os.path.join(GAITS, "hopper_3D_gait_forward.jld2"))
    k = knots(fwd, 512)
    out.append(leg("hopper512", "hopper_3D", fwd.q[k], fwd.q[k + 1], fwd.u[k], 0.01, 1.5))
    shift = np.zeros((512, 7)); shift[:, 0] = 0.13 * k; shift[:, 2] = 0.075
    out.append(leg("hopper512 sine2", "hopper_3D", fwd.q[k] + shift, fwd.q[k + 1] + shift, fwd.u[k], 0.01, 1.5, ter="sine2_3D_lc"))
    quad = gait("quadruped_gait2")
    k = knots(quad, 256)
    out.append(leg("quadruped256", "quadruped", quad.q[k], quad.q[k + 1], quad.u[k], quad.h, 0.5, max(10, calls // 5)))
    for name in ("sine1_2D_lc", "piecewise1_2D_lc"):
        q0, q1 = quad.q[k].copy(), quad.q[k + 1].copy()
        for q in (q0, q1):
            q[:, 0] += np.linspace(0.0, 2.5, 256)
            q[:, 1] += terrain.get(name).surface(q[:, 0])
        out.append(leg("quadruped256 " + name, "quadruped", q0, q1, quad.u[k], quad.h / 5, 1.0, max(10, calls // 10), ter=name))
    for model, f in (("centroidal_quadruped", "centroidal_inplace_trot_v7"), ("centroidal_quadruped_box", "step_over_box_v0"),
                     ("centroidal_quadruped_wall", "wall_stand_FL_4")):
        g = gait(f)
        k = knots(g, 256)
        out.append(leg(model.replace("_quadruped", "") + "256", model, g.q[k], g.q[k + 1], g.u[k], g.h, g.mu, max(10, calls // 5)))
    fl = gait("flamingo_gait_forward_36_4")
    k = np.arange(16)
    out.append(leg("flamingo16", "flamingo", fl.q[k], fl.q[k + 1], fl.u[k], fl.h, 0.9, timed=False))
    rng = np.random.default_rng(7)
    for model, name, nq in (("hopper_2D", "slope1_2D_lc", 4), ("particle", "quadratic_bowl_3D_lc", 3), ("particle_2D", "slope1_2D_lc", 2)):
        T, q1 = terrain.get(name), np.zeros((16, nq))
        q1[:, 0] = rng.uniform(-1.0, 1.0, 16) if model == "particle" else np.linspace(-0.2, 2.3, 16)
        if model == "particle":
            q1[:, 1] = rng.uniform(-1.0, 1.0, 16)
            q1[:, 2] = T.surface(q1[:, 0], q1[:, 1]) + rng.uniform(-0.01, 0.02, 16)
        elif model == "hopper_2D":
            q1[:, 2] = rng.uniform(-0.2, 0.2, 16); q1[:, 3] = 0.5
            q1[:, 1] = T.surface(q1[:, 0] + 0.5 * np.sin(q1[:, 2])) + 0.5 * np.cos(q1[:, 2]) + rng.uniform(-0.01, 0.02, 16)
        else:
            q1[:, 1] = T.surface(q1[:, 0]) + rng.uniform(-0.01, 0.02, 16)
        u = rng.uniform(-1.0, 1.0, (16, plant.model_dims(model)[2]))
        if model == "hopper_2D":
            u[:, 1] += 3.3 * 9.81 * 0.2
        out.append(leg(model + "16 " + name, model, q1 - 0.01 * rng.uniform(-0.5, 0.5, (16, nq)), q1, u, 0.01, 0.8 if model == "hopper_2D" else 0.5,
                       ter=name, timed=False))
    return [o for o in out if o is not None]


def kernel_legs(libs, pairs):
    """`compare`: every library's result of one wrapper call against this build's, bit for bit; `timed`: the same call, alternating"""
    import gains_cases as gc
    import gains_ref
    import plant_gradient_cases as pgc
    import plant_linearize_cases as plc
    from contactimplicitmpc.jl_amd import terrain
    compare, timed = [], []

    def leg(name, fn, *args, calls=0, **kw):
        first = on(libs["this"], fn, *args, **kw)
        out = {"leg": name, "identical_outputs": {k: same(first, on(lib, fn, *args, **kw)) for k, lib in libs.items() if k != "this"}}
        if calls and pairs:
            t = {k: [] for k in libs}
            for _ in range(pairs):
                for k, lib in libs.items():
                    with bound(lib):
                        t0 = time.perf_counter()
                        for _ in range(calls):
                            fn(*args, **kw)
                        t[k].append((time.perf_counter() - t0) / calls * 1e6)
            out.update(calls_per_turn=calls, per_call={k: summary(v) for k, v in t.items()})
        (timed if calls else compare).append(out)
        print(json.dumps(out), flush=True)
        return first

    def knots3(model, seed, x=None):
        nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(model)
        z, th = plc.inputs(seed, nz, nth, 3)
        if x is not None:
            z[:, 0] = x
        return z, th, nth

    def lin_and_sens(what, model, z, th, nth, ter=None):
        leg(f"linearize {what}", plant.linearize, model, z, th, plc.KAPPA, terrain=ter)
        for n_cols in (1, nth):
            for reg in pgc.REGS:
                leg(f"sensitivity {what} n_cols={n_cols} reg={reg:g}", plant.sensitivity, model, z, th, reg, n_cols=n_cols, terrain=ter)

    for mid, model in sorted(plc.TORCH_MODELS.items()):
        lin_and_sens(model, model, *knots3(model, mid))
    for model, mid, name in plc.TERRAIN_CASES:                      # knot 1 of 3 stands on the flat terrain of the same family
        flat = "flat_3D_lc" if model in ("particle", "hopper_3D") else "flat_2D_lc"
        rng = np.random.default_rng(200 + mid)
        x = rng.uniform(-1.0, 1.0, 3) if model in ("particle", "hopper_3D") else rng.uniform(-0.5, 2.5, 3)
        z, th, nth = knots3(model, 100 + mid, x)
        lin_and_sens(f"{model} on [{name}, {flat}, {name}]", model, z, th, nth, [terrain.get(name), terrain.get(flat), terrain.get(name)])
        lin_and_sens(f"{model} on {name} (shared)", model, z, th, nth, name)

    def gains_inputs(case, whole):
        model_name, file, kind, n, N = gc.CASES[case]
        model, z, th = gc.knots(model_name, file, kind)
        n, N = (z.shape[0], 10) if whole or n is None else (n, N)      # whole: every knot of the gait and N = 10, as gains_ab.py
        return model_name, model, np.ascontiguousarray(z[:n]), np.ascontiguousarray(th[:n]), gc.hopper_weights() if model_name == "hopper_3D" else gc.centroidal_weights(), N

    def gains_legs(case, calls=0, whole=False):
        name, model, z, th, w, N = gains_inputs(case, whole)
        tag = f" ({z.shape[0]} knots, N = {N})" if whole else ""
        leg(f"reference_gains {case}{tag}", gains.reference_gains, name, z, th, *w, N=N, return_P1=True, calls=calls)
        _, rz0, rth0 = plant.linearize(name, z, th, 0.0)
        leg(f"reference_gains_lin {case}{tag}", gains.reference_gains_lin, model.nq, model.nu, rz0, rth0, *w, N=N, return_P1=True, calls=calls)
        AB = [gains_ref.dynamics(model.nq, model.nu, rz0[t], rth0[t]) for t in range(z.shape[0])]
        Q, R = gains_ref.weights(*w)
        leg(f"tvlqr {case}{tag}", gains.tvlqr, np.stack([a for a, _ in AB]), np.stack([b for _, b in AB]), Q[None], np.tile(R[None], (N * z.shape[0], 1, 1)),
            n_keep=z.shape[0], calls=calls)

    for case in ("hopper_3D in place, knots 1-5, N = 3", "box step-over, knots 1-3, N = 2"):      # nz 19 and 66, the fewest knots
        gains_legs(case)
    for which in ("hopper_2D", "particle"):                         # the two short rollout cases of tests/plant_gradient_cases.py, one on a terrain
        c = pgc.rollout_case(which)
        leg(f"rollout diff_sol {which}", plant.rollout, c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], terrain=c["terrain"], diff_sol=True)

    if pairs:
        for case, model in (("quadruped gait2", "quadruped"), ("wall_stand_FL_4", "centroidal_quadruped_wall")):
            _, z, th = gc.knots(model, {"quadruped": "quadruped_gait2.jld2"}.get(model, "wall_stand_FL_4.jld2"), "gait")
            nq, nu = pgc.dims(model)[:2]
            leg(f"linearize {case}, {z.shape[0]} knots", plant.linearize, model, z, th, 1e-3, calls=10)
            leg(f"sensitivity {case}, {z.shape[0]} knots, n_cols=2nq+nu", plant.sensitivity, model, z, th, pgc.REG, n_cols=2 * nq + nu, calls=10)
        gains_legs("centroidal trot, all knots, N = 10", calls=3)
        gains_legs("wall stand, knots 1-3, N = 2", calls=3, whole=True)
        for name, model, f, B, T in (("quadruped gait2 replay", "quadruped", "quadruped_gait2", 256, 100),
                                     ("centroidal in-place trot replay", "centroidal_quadruped", "centroidal_inplace_trot_v7", 64, 60)):      # the legs of plant_gradients_ab.py
            g = gait_io.load_gait(os.path.join(GAITS, f + ".jld2"))
            k = np.arange(B) * g.H // B
            q1, v1 = np.ascontiguousarray(g.q[k + 1]), (g.q[k + 1] - g.q[k]) / g.h
            u = np.ascontiguousarray(np.stack([g.u[(k + t) % g.H] for t in range(T)]))
            leg(f"rollout {name} B={B} T={T}", plant.rollout, model, q1, v1, u, g.h, g.mu, calls=1)
            leg(f"rollout diff_sol {name} B={B} T={T}", plant.rollout, model, q1, v1, u, g.h, g.mu, diff_sol=True, calls=1)
    return {"compare": compare, "timed": timed}


def ratios(res):
    """per timed leg: this build over `parent` and `parent_copy` over `parent`, medians; `slower_than_spread`: the first is above 1 by more than the second is away
    from 1"""
    out = []
    def add(name, t):
        if t and all(k in t for k in ("this", "parent", "parent_copy")):
            m = {k: t[k]["median_us"] for k in t}
            a, b = m["this"] / m["parent"], m["parent_copy"] / m["parent"]
            out.append({"leg": name, "this_over_parent": round(a, 4), "parent_copy_over_parent": round(b, 4), "slower_than_spread": bool(a - 1.0 > abs(b - 1.0))})
    for o in res["plant_step"]:
        add("plant_step " + o["leg"], o["per_call"])
    for o in res["rollout"]:
        add(f"rollout {o['leg']} B={o['B']}", o["rollout_per_step_on"])
    for o in res.get("kernels", {}).get("timed", []):
        add(o["leg"], o.get("per_call"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--step-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--parent-step-us", action="append", default=[], metavar="LEG=US")
    ap.add_argument("--legs", nargs="*", default=[], metavar="TEXT", help="only the step legs whose name contains one of these")
    ap.add_argument("--no-rollout", action="store_true", help="the step legs only")
    ap.add_argument("--no-step", action="store_true", help="no step legs")
    ap.add_argument("--kernels", action="store_true", help="the kernel legs: linearize, sensitivity, the gains, rollout gradients")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_rollout_ab.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    libs = {"this": _lib.load()}
    for spec in a.step_lib:
        name, path = spec.split("=", 1)
        lib = C.CDLL(os.path.abspath(path))
        for f, (restype, argtypes) in _lib.SIGNATURES.items():
            getattr(lib, f).restype, getattr(lib, f).argtypes = restype, argtypes
        libs[name] = lib

    res = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "rollout": [], "plant_step": [] if a.no_step else step_legs(libs, a.pairs, a.calls, a.legs),
           "parent_step_us_from_the_command_line": dict(s.split("=", 1) for s in a.parent_step_us)}
    if not a.no_rollout:
        quad = gait_io.load_gait(os.path.join(GAITS, "quadruped_gait2.jld2"))
        hop = gait_io.load_joint_traj(os.path.join(GAITS, "hopper_3D_gait_in_place.jld2"))
        for B in BATCHES:
            res["rollout"].append(rollout_leg("hopper_3D gait_in_place replay", "hopper_3D", hop.q[0], hop.q[1], np.asarray(hop.u), hop.h, 1.5, B, a.pairs, libs))
            res["rollout"].append(rollout_leg("quadruped gait2 replay", "quadruped", quad.q[0], quad.q[1], np.asarray(quad.u), quad.h, 0.5, B, a.pairs, libs))
    if a.kernels:
        res["kernels"] = kernel_legs(libs, a.pairs)
    res["ratios"] = ratios(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
