"""The rollout calls share one grow-only workspace per device, and every call takes its regions from `plant_rollout_layout`
(csrc/plant_rollout_call.h): a call that follows a larger one of another kind lands in buffers that are bigger than it asks for and
hold the other call's data.  In one process, in this order:

    A   the closed-loop tape rollout of hopper_2D: the case of tests/plant_feedback_cases.py with its per-robot schedule, the first
        two robots and the first three steps (B = 2, T = 3), every column of θ, z kept
    B   `rollout(diff_sol=True)` of pushbot, B = 3, T = 5, with per-robot w and mu: the case of tests/plant_feedback_cases.py, its third
        robot robot 0 again under robot 1's controls, a w of a few 1e-3 per robot and step and a friction coefficient per robot
    A'  A again, with one `vjp`

Every array of A', the `vjp` outputs included, equals A's bit for bit (`array_equal`; A makes the same `vjp`), and every array of B
equals the same call made first in a fresh child process.  Nothing here is a tolerance: a wrong offset or a region that shrank
between the calls changes bits.  A and A' run prefixes of rollouts that tests/test_plant_feedback.py shows to converge on the CPU; B's
comparison does not depend on convergence.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import plant_feedback_cases as pfc
import plant_gradient_cases as pgc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call_a():
    """A: dict of every array the tape rollout and one `vjp` of gq = 1, ggamma = 1 return."""
    from contactimplicitmpc.jl_amd import plant
    c, f = pfc.base_case("hopper_2D"), pfc.feedback("hopper_2D", "per_robot")
    B, T = 2, 3
    fb = plant.Feedback(f["K"][:T, :B], f["x_ref"][:T, :B], hold=f["hold"], n_sample=f["n_sample"])
    ok, q, ua, g, b, st, it, tape, fb_err = plant.rollout_tape(c["model"], c["q1"][:B], c["v1"][:B], c["u"][:T, :B], c["h"], c["mu"][:B],
                                                               steps_per_launch=pfc.STEPS_PER_LAUNCH, grad_cols=pgc.dims(c["model"])[6], keep_z=True,
                                                               feedback=fb)
    with tape:
        cot = tape.vjp(gq=np.ones(q.shape), ggamma=np.ones(g.shape))
        out = dict(q=q, u_applied=ua, gamma=g, b=b, status=st, iters=it, fb_err=fb_err, z=tape.z, grad_status=tape.grad_status)
        for k in ("q1", "v1", "u", "u_step", "w_step", "g_mu", "g_h", "n_cut", "g_q0", "g_q1", "K", "x_ref", "xref_step"):
            out["vjp_" + k] = np.asarray(getattr(cot, k))
    return out


def _call_b():
    """B: dict of every array `rollout(diff_sol=True)` returns."""
    from contactimplicitmpc.jl_amd import plant
    c = pfc.base_case("pushbot")
    pick = [0, 1, 0]
    B, T, nw = 3, c["T"], pgc.dims("pushbot")[4]
    u = c["u"][:, [0, 1, 1]]
    w = 1e-3 * (1.0 + np.arange(T * B * nw, dtype=np.float64).reshape(T, B, nw))
    ok, q, ua, g, b, st, it, G = plant.rollout(c["model"], c["q1"][pick], c["v1"][pick], u, c["h"], np.array([0.5, 0.5, 0.4]), w=w,
                                               steps_per_launch=pfc.STEPS_PER_LAUNCH, diff_sol=True, grad_cols=pgc.dims("pushbot")[6])
    assert q.shape == (T + 2, B, 2) and w.shape == (T, B, nw)
    return dict(q=q, u_applied=ua, gamma=g, b=b, status=st, iters=it, dz=G.dz, z=G.z, grad_status=G.status)


@pytest.mark.gpu
def test_a_call_after_a_larger_call_of_another_kind_returns_the_same_bits(tmp_path):
    alone = str(tmp_path / "b_alone.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    child = subprocess.run([sys.executable, os.path.abspath(__file__), alone], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert child.returncode == 0, child.stderr[-3000:]
    a, b, a2 = _call_a(), _call_b(), _call_a()
    assert a["status"].shape == (3, 2) and b["status"].shape == (5, 3)
    for k in a:
        assert a2[k].shape == a[k].shape and a2[k].tobytes() == a[k].tobytes(), f"A' differs from A in {k}"
    with np.load(alone) as first:
        assert sorted(first.files) == sorted(b)
        for k in b:
            assert first[k].shape == b[k].shape and first[k].tobytes() == b[k].tobytes(), f"B after A differs from B alone in {k}"
    assert a["vjp_xref_step"].any() and b["dz"].any(), "the compared arrays are not all zeros"


if __name__ == "__main__":      # the child: B alone, as the first call of a fresh process
    import torch
    assert torch.cuda.is_available()
    np.savez(sys.argv[1], **_call_b())
