#!/usr/bin/env python3
"""What forward tangents through a device rollout cost, on the two legs of scripts/plant_gradients_ab.py, on ONE tape made beforehand:

  (a) `RolloutTape.jvp` of one direction in (q1, v1, u): the whole trajectory tangent;
  (b) `RolloutTape.transition()`: the 2nq unit directions of [dq0; dq1] in ONE launch, each block read once per group of directions;
  (c) the same 2nq directions as 2nq launches of one direction each (what (b) replaces), equal to (b) bit for bit;
  (d) `RolloutTape.vjp` on the same tape, for scale;
  (e) the host route: `plant.rollout(diff_sol=True)` - every block read back and transposed - and the forward chain in NumPy (batched
      over the robots with `@`), for one direction and for the 2nq; the NumPy chains are also timed alone on blocks already on the host.
(a) and (d) are timed a second time back to back, behind the alternating turns, and the ratios against `vjp` are taken there: in the
alternation the quadruped leg's `vjp` scattered between 3.5 and 24 ms in three runs, where back to back it takes its recorded 0.9-1.0 ms.

One GPU, one process, a warm call, then alternating turns, a host clock around whole calls; medians over `--turns` turns (at least
20).  Recorded, not asserted.  `--figures-from LOG` adds the figures a `pytest -s` run of tests/test_gpu_plant_tangent.py printed
(distance from tangent_ld per case, the adjoint identity, the flight finite differences), as they stand.
usage: python scripts/plant_tangent_ab.py [--turns 20] [--figures-from LOG] [--out profiles/plant_tangent.json]"""
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
from contactimplicitmpc.jl_amd import plant  # noqa: E402
from plant_adjoint_ab import leg_inputs  # noqa: E402
from plant_gradients_ab import LEGS, summary  # noqa: E402


def host_tangents(D, dq0, dq1, du_step, nq):
    """The forward chain in float64 NumPy over StepGradients.dz (T, B, nr, n_cols), batched over the robots and the directions:
    dq0, dq1 (n_dir, B, nq), du_step (n_dir, T, B, nu) or None -> δq (n_dir, T + 2, B, nq)."""
    T, B = D.shape[:2]
    n_dir = dq0.shape[0]
    nu = D.shape[3] - 2 * nq
    q = np.zeros((n_dir, T + 2, B, nq))
    q[:, 0], q[:, 1] = dq0, dq1
    zero = np.zeros((n_dir, B, nu))
    for t in range(T):
        x = np.concatenate([q[:, t], q[:, t + 1], zero if du_step is None else du_step[:, t]], axis=2)      # (n_dir, B, n_cols)
        q[:, t + 2] = np.einsum("brc,dbc->dbr", D[t, :, :nq], x)
    return q


def leg(name, model, gait_file, B, T, turns):
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    g, q1, v1, u = leg_inputs(model, gait_file, B, T)
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(model)
    rng = np.random.default_rng(0)
    gq, gg, gb = pac.random_cotangents(rng, T, B, nq, nc, nb)
    dq1, dv1, du = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal(u.shape)
    units0, units1 = np.zeros((2 * nq, B, nq)), np.zeros((2 * nq, B, nq))
    for i in range(nq):
        units0[i, :, i] = 1.0
        units1[nq + i, :, i] = 1.0
    *_, tape = plant.rollout_tape(model, q1, v1, u, g.h, g.mu)
    *_, G = plant.rollout(model, q1, v1, u, g.h, g.mu, diff_sol=True)
    one0, one1 = np.ascontiguousarray((dq1 - g.h * dv1)[None]), np.ascontiguousarray(dq1[None])

    def separate():
        return np.concatenate([tape._jvp_steps(1, units0[d:d + 1], units1[d:d + 1], rows=False)[0] for d in range(2 * nq)])

    def host_route(n):
        *_, G2 = plant.rollout(model, q1, v1, u, g.h, g.mu, diff_sol=True)
        return host_tangents(G2.dz, one0, one1, du[None], nq) if n == 1 else host_tangents(G2.dz, units0, units1, None, nq)

    runs = {"jvp_one_direction": lambda: tape.jvp(dq1=dq1, dv1=dv1, du=du),
            "transition_2nq_directions_one_launch": tape.transition,
            "transition_2nq_directions_2nq_launches": separate,
            "vjp": lambda: tape.vjp(gq, gg, gb),
            "rollout_diff_sol_and_host_chain_one_direction": lambda: host_route(1),
            "rollout_diff_sol_and_host_chain_2nq_directions": lambda: host_route(2 * nq),
            "host_chain_alone_one_direction": lambda: host_tangents(G.dz, one0, one1, du[None], nq),
            "host_chain_alone_2nq_directions": lambda: host_tangents(G.dz, units0, units1, None, nq)}
    outs = {n: f() for n, f in runs.items()}                        # warm-up, and the outputs side by side
    times = {n: [] for n in runs}
    for _ in range(turns):
        for n, f in runs.items():
            t0 = time.perf_counter(); f(); times[n].append((time.perf_counter() - t0) * 1e3)
    for n in ("jvp_one_direction", "vjp"):                          # and each of the two alone, back to back, after the alternating turns
        times[n + "_back_to_back"] = []
        for _ in range(turns):
            t0 = time.perf_counter(); runs[n](); times[n + "_back_to_back"].append((time.perf_counter() - t0) * 1e3)
    tape.close()
    grouped, apart = outs["transition_2nq_directions_one_launch"], outs["transition_2nq_directions_2nq_launches"]
    apart_phi = np.concatenate([apart[:, T], apart[:, T + 1]], axis=2).transpose(1, 2, 0)
    res = {"leg": name, "model": model, "B": B, "T": T, "n_cols": 2 * nq + nu, "directions_of_a_transition": 2 * nq, "directions_per_workgroup": int(
               plant.tangent_group(model, 2 * nq + nu)), "tape_bytes": T * B * nr * (2 * nq + nu) * 8,
           "n_cut_total": int(outs["jvp_one_direction"].n_cut.sum()), "time": {n: summary(v) for n, v in times.items()},
           "grouped_equals_separate_launches_bit_for_bit": bool(grouped.tobytes() == np.ascontiguousarray(apart_phi).tobytes()),
           "device_vs_host_chain_max_rel": pac.distance(outs["jvp_one_direction"].q, outs["host_chain_alone_one_direction"][0])}
    med = lambda n: res["time"][n]["median_ms"]
    res["separate_launches_over_one_grouped_launch"] = round(med("transition_2nq_directions_2nq_launches") / med("transition_2nq_directions_one_launch"), 3)
    res["grouped_launch_over_vjp_back_to_back"] = round(med("transition_2nq_directions_one_launch") / med("vjp_back_to_back"), 3)
    res["jvp_one_direction_over_vjp_both_back_to_back"] = round(med("jvp_one_direction_back_to_back") / med("vjp_back_to_back"), 3)
    res["host_route_over_transition"] = round(med("rollout_diff_sol_and_host_chain_2nq_directions") / med("transition_2nq_directions_one_launch"), 3)
    res["host_chain_alone_over_transition"] = round(med("host_chain_alone_2nq_directions") / med("transition_2nq_directions_one_launch"), 3)
    print(json.dumps(res), flush=True)
    return res


def figures(path):
    """The lines of a `pytest -s` log of tests/test_gpu_plant_tangent.py that state a measured figure, as they stand."""
    keep = re.compile(r"at most .* from tangent_ld|<g, jvp\(d\)>|central differences of the device rollout|from the longdouble product")
    with open(path) as f:
        return [line.strip().lstrip(".") for line in f if keep.search(line)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=20)
    ap.add_argument("--figures-from", default=None, metavar="LOG", help="a `pytest -s` log of tests/test_gpu_plant_tangent.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_tangent.json"))
    a = ap.parse_args()

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.turns >= 20, "medians of at least 20 turns"
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "legs": [leg(*l, a.turns) for l in LEGS]}
    if a.figures_from:
        res["figures_of_tests_test_gpu_plant_tangent"] = figures(a.figures_from)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
