#!/usr/bin/env python3
"""What the clamp's derivative costs, on the two legs of scripts/plant_tangent_ab.py (quadruped B 256 T 100,
centroidal_quadruped B 64 T 60), in ONE process, a host clock around whole calls (each ends in a stream synchronize), a warm call each, then
alternating turns; medians, minima and maxima.  Recorded, not asserted.

  the chains     `vjp`, one `jvp` direction and `transition()` on four tapes of the same closed-loop rollout call (the per-robot gains and
                 gait reference of scripts/plant_feedback_ab.py): (a) the unlimited tape of this build, (a') a second one, its A/A twin,
                 (c) the LIMITED tape (`clamp_grad=True`; even controls capped at the median of what the unlimited loop applied to them, odd
                 ones given limits one unit outside it), which launches the third instantiation of the two chain kernels, and with
                 `--parent-lib PATH` (p) the unlimited tape of a build of the parent commit.  (a) and (p) are compared bit for bit.
  the tape call  `rollout_tape` unlimited, its twin, and limited (the LOOP = 2 step kernel, the mask kernel and one more read-back)
  the compiler   `--resources JSON`, made without a device by `--compile-resources` (hipcc -Rpass-analysis=kernel-resource-usage over
                 plant_adjoint.hip, plant_tangent.hip and plant_kernel.hip; with `--parent-asm DIR`, the `--cuda-device-only -S` texts
                 plant_kernel.s, plant_adjoint.s and plant_tangent.s of the parent commit, also the number of assembly lines in which each
                 instantiation the parent has differs from it, resource directives included), is copied in as it stands

usage: python scripts/plant_clamp_ab.py [--turns 20] [--parent-lib PATH] [--resources JSON] [--figures-from LOG] [--out profiles/plant_clamp.json]
       python scripts/plant_clamp_ab.py --compile-resources OUT.json [--parent-asm DIR]        (no device)"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CSRC = os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc")
KEPT = ("plant_adjoint_kernel", "plant_tangent_kernel", "plant_clamp_mask_kernel", "plant_step_kernel")
HIPCC = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "--cuda-device-only", "-S"]


def demangled(name):
    return re.sub(r"\(.*", "", subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()).replace("void ", "").replace("cimpc::", "")


def kernel_texts(path):
    """{demangled kernel: its assembly lines} of a `--cuda-device-only -S` file: from the kernel's label to its .Lfunc_end, comments, blank
    lines, the kernel's own mangled name and the function number inside branch labels taken out."""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[demangled(name)] = cur
                cur = None
                continue
            text = line.split(";")[0].strip().replace(name, "KERNEL")
            text = re.sub(r"\.LBB\d+_", ".LBB_", text)              # a branch label carries its function's number in the file
            if text:
                cur.append(text)
    return out


def compile_resources(out, parent_asm):
    """VGPRs, AGPRs, scratch, LDS, occupancy and spills of every instantiation of the chain kernels, the mask kernel and the step kernel, as the
    compiler reports them; with the parent's assembly, how many lines of each instantiation the parent has differ from it."""
    table, res = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ("plant_adjoint.hip", "plant_tangent.hip", "plant_kernel.hip"):
            asm = os.path.join(tmp, unit + ".s")
            run = subprocess.run(HIPCC + ["-o", asm, "-Rpass-analysis=kernel-resource-usage", unit], cwd=CSRC, capture_output=True, text=True, check=True)
            cur = None
            for line in run.stderr.splitlines():
                m = re.search(r"remark: \s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
                if not m:
                    continue
                key, val = m.group(1).strip(), m.group(2)
                if key == "Function Name":
                    cur = demangled(val)
                    cur = cur if cur.startswith(KEPT) else None
                    if cur:
                        table[cur] = {}
                elif cur and key in ("VGPRs", "AGPRs", "SGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size"):
                    table[cur][key] = int(val)
            old_asm = os.path.join(parent_asm, unit.replace(".hip", ".s")) if parent_asm else None
            if old_asm and os.path.exists(old_asm):
                new, old = kernel_texts(asm), kernel_texts(old_asm)
                for k in sorted(k for k in new if k.startswith(KEPT)):
                    was = k if k in old else k.replace("<0>", "<false>").replace("<1>", "<true>")      # the chain kernels' FB was a bool
                    if was not in old:
                        continue
                    lines = [(b, a) for a, b in zip(new[k], old[was]) if a != b]
                    entry = {"lines": len(old[was]), "differing": len(lines) + abs(len(new[k]) - len(old[was]))}
                    if lines and len(lines) <= 4:
                        entry["they_are"] = [f"{b} -> {a}" for b, a in lines]
                    res.setdefault("assembly_lines_differing_from_the_parent_commit", {})[k] = entry
    res["kernel_resources_gfx950"] = table
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def leg(name, model, gait_file, B, T, turns, parent):
    from contactimplicitmpc.jl_amd import gait_io, plant
    from plant_boxqp_ab import timed, using
    from plant_feedback_ab import GAIN_SCALE, leg_inputs
    from plant_gradients_ab import summary
    import plant_adjoint_cases as pac
    import plant_gradient_cases as pgc
    g, q1, v1, u, x_ref = leg_inputs(gait_io, gait_file, B, T)
    nq, nu, nc, nb = pgc.dims(model)[:4]
    rng = np.random.default_rng(0)
    K = GAIN_SCALE[model] * rng.standard_normal((T, B, nu, 2 * nq))
    gq, gg, gb = pac.random_cotangents(rng, T, B, nq, nc, nb)
    dq1, dv1, du = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal(u.shape)
    args = (model, q1, v1, u, g.h, g.mu)
    fb = lambda **lim: plant.Feedback(K, x_ref, **lim)
    ua0 = plant.rollout(*args, feedback=fb())[2]
    u_lo, u_hi = np.full((B, nu), -np.inf), np.full((B, nu), np.inf)
    u_hi[:, 0::2] = np.median(ua0[:, :, 0::2], axis=0)
    u_lo[:, 1::2], u_hi[:, 1::2] = ua0[:, :, 1::2].min(axis=0) - 1.0, ua0[:, :, 1::2].max(axis=0) + 1.0
    limited = fb(u_lo=u_lo, u_hi=u_hi, clamp_grad=True)

    def tape_of(feedback):
        *_, tape, _ = plant.rollout_tape(*args, feedback=feedback)
        return tape

    def make_and_drop(feedback):
        tape_of(feedback).close()

    tapes = {"a_unlimited": tape_of(fb()), "a_twin": tape_of(fb()), "c_limited": tape_of(limited)}
    if parent is not None:
        with using(parent):
            tapes["p_parent_unlimited"] = tape_of(fb())

    def on(key, f):
        if key.startswith("p_"):
            def run():
                with using(parent):
                    return f(tapes[key])
            return run
        return lambda: f(tapes[key])

    ops = {"vjp": lambda t: t.vjp(gq, gg, gb), "jvp_one_direction": lambda t: t.jvp(dq1=dq1, dv1=dv1, du=du), "transition": lambda t: t.transition()}
    mask = tapes["c_limited"].clamped
    res = {"leg": name, "model": model, "B": B, "T": T, "n_cols": 2 * nq + nu, "directions_of_a_transition": 2 * nq,
           "clamped_controls": int(sum(((mask >> i) & 1).sum() for i in range(nu))), "of": int(mask.size * nu), "time": {}, "ratios_of_medians": {}}
    for op, f in ops.items():
        outs, times = timed({k: on(k, f) for k in tapes}, turns)
        res["time"][op] = {k: summary(v) for k, v in times.items()}
        med = {k: res["time"][op][k]["median_ms"] for k in tapes}
        r = {"twin_over_unlimited": round(med["a_twin"] / med["a_unlimited"], 4), "limited_over_unlimited": round(med["c_limited"] / med["a_unlimited"], 4)}
        if parent is not None:
            r["unlimited_over_parent"] = round(med["a_unlimited"] / med["p_parent_unlimited"], 4)
            r["limited_over_parent"] = round(med["c_limited"] / med["p_parent_unlimited"], 4)
            a, p = outs["a_unlimited"], outs["p_parent_unlimited"]
            keys = ("g_q0", "g_q1", "u_step", "xref_step") if op == "vjp" else ("q", "gamma", "b", "u_applied") if op == "jvp_one_direction" else None
            same = np.array_equal(a, p) if keys is None else all(np.array_equal(getattr(a, k), getattr(p, k)) for k in keys)
            res.setdefault("unlimited_equals_parent_bit_for_bit", {})[op] = bool(same)
        res["ratios_of_medians"][op] = r
    _, times = timed({"a_unlimited": lambda: make_and_drop(fb()), "a_twin": lambda: make_and_drop(fb()), "c_limited": lambda: make_and_drop(limited)}, max(3, turns // 4))
    res["time"]["rollout_tape"] = {k: summary(v) for k, v in times.items()}
    med = {k: v["median_ms"] for k, v in res["time"]["rollout_tape"].items()}
    res["ratios_of_medians"]["rollout_tape"] = {"twin_over_unlimited": round(med["a_twin"] / med["a_unlimited"], 4),
                                                "limited_over_unlimited": round(med["c_limited"] / med["a_unlimited"], 4)}
    for key, tape in tapes.items():
        if key.startswith("p_"):
            with using(parent):
                tape.close()
        else:
            tape.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, metavar="PATH", help="libcimpc_hip.so of a build of the parent commit")
    ap.add_argument("--resources", default=None, metavar="JSON", help="the output of --compile-resources")
    ap.add_argument("--figures-from", default=None, metavar="LOG", help="a `pytest -s` log of tests/test_gpu_plant_clamp.py")
    ap.add_argument("--compile-resources", default=None, metavar="OUT.json")
    ap.add_argument("--parent-asm", default=None, metavar="DIR", help="with --compile-resources: the parent's plant_kernel.s, plant_adjoint.s, plant_tangent.s (--cuda-device-only -S)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_clamp.json"))
    a = ap.parse_args()
    if a.compile_resources:
        return compile_resources(a.compile_resources, a.parent_asm)
    for path in (a.parent_lib, a.resources, a.figures_from):      # before anything is measured
        assert path is None or os.path.exists(path), f"{path} not found"

    import torch                                                    # the device comes up through torch first, as in the tests
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.turns >= 3, "medians of at least 3 turns"
    from plant_boxqp_ab import bound_library
    from plant_gradients_ab import LEGS
    parent = bound_library(a.parent_lib) if a.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "turns": a.turns, "parent_build_measured": parent is not None,
           "legs": [leg(*l, a.turns, parent) for l in reversed(LEGS)]}
    if a.resources:
        res.update(json.load(open(a.resources)))
    if a.figures_from:
        keep = re.compile(r"controls clamped|from chain_ld|from tangent_ld|<g, jvp|caller's arguments|central differences")
        res["figures_of_tests_test_gpu_plant_clamp"] = [re.sub(r"^\.+", "", line.strip()) for line in open(a.figures_from) if keep.search(line)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
