"""Two pins of what a handle remembers between calls (csrc/handle_state.h), on the device.  Both describe behaviour the library had
before the state moved into that header; the failure paths are tested on the CPU (test_handle_state.py), never by making a HIP
call fail.

* After `mpc_advance` the window lives on the device only: an `mpc_solve` that brings the window of the step before again must
  upload and re-key it, exactly as the separate `set_window` / `set_reference` / `newton_solve` calls do.
* `gain_latch` runs between a Newton solve and the next move of the window or the reference, whichever call moves them.  (The
  policy-level cadence - latch, feedback, advance - is in test_gpu_gains.py.)
"""
import numpy as np
import pytest

from contactimplicitmpc.jl_amd import CimpcError
from oracle import synth

from common import make_case, make_solver

pytestmark = pytest.mark.gpu

H, H_REF, B = 6, 8, 2
FIELDS = ("q", "u", "gamma", "b", "nu")


@pytest.fixture(scope="module")
def case():
    d, prob, tabs, rollouts = make_case("hopper", 0, H_ref=H_REF, H=H, B=B, seed=6, perturb=1e-2)
    W = np.stack([w for (w, _, _, _) in rollouts]) + 1
    R = {f: np.stack([getattr(r, f) for (_, r, _, _) in rollouts]) for f in ("q", "u", "w", "gamma", "b", "theta")}
    q0 = np.stack([r[2] for r in rollouts]); q1 = np.stack([r[3] for r in rollouts])
    return d, prob, rollouts, W, R, q0, q1


def _solver(case):
    d, prob, rollouts = case[:3]
    return make_solver(d, prob, rollouts, H, obj=synth.make_objective(d, H))


def _one_step_later(case):
    """window and reference of the same rollouts one MPC step on"""
    d, prob, rollouts = case[:3]
    sh = [synth.make_rollout(d, prob, H, phase=(int(w[0]) + 1) % H_REF, seed=1000 + k, perturb=0.0)[:2] for k, (w, _, _, _) in enumerate(rollouts)]
    return np.stack([w for w, _ in sh]) + 1, {f: np.stack([getattr(r, f) for _, r in sh]) for f in ("q", "u", "w", "gamma", "b", "theta")}


def test_mpc_solve_uploads_its_window_again_after_a_device_side_move(case):
    d, _, _, W, R, q0, q1 = case
    stride = np.zeros(d.nq); stride[0] = 0.05
    a, b = _solver(case), _solver(case)
    try:
        for warm in (False, True):
            if warm:
                a.mpc_advance(stride)
                b.mpc_advance(stride)
            u1a, ita, rna, ta = a.mpc_solve(q0, q1, window=W, reference=R, warm_start=warm, which=FIELDS)
            b.set_window(W)
            b.set_reference(R["q"], R["u"], R["w"], R["gamma"], R["b"], R["theta"])
            u1b, itb, rnb = b.newton_solve(q0, q1, warm_start=warm)
            tb = b.trajectory()
            assert np.array_equal(u1a, u1b) and np.array_equal(ita, itb) and np.array_equal(rna, rnb), warm
            for f in FIELDS:
                assert np.array_equal(ta[f], tb[f]), (warm, f)
        assert np.array_equal(a.reference()["window"], W)
        assert np.array_equal(b.reference()["window"], W)
    finally:
        a.close(); b.close()


def test_gain_latch_runs_between_a_solve_and_the_next_move(case):
    d, _, _, W, R, q0, q1 = case
    W2, R2 = _one_step_later(case)
    assert not np.array_equal(W2, W)
    stride = np.zeros(d.nq); stride[0] = 0.05
    s = _solver(case)
    try:
        s.set_gains(np.random.default_rng(2).standard_normal((H_REF, d.nu, 2 * d.nq)))
        s.newton_solve(q0, q1)
        s.gain_latch()
        s.set_window(W)                      # the same window: still a move as far as the latch is concerned
        with pytest.raises(CimpcError):
            s.gain_latch()
        s.mpc_solve(q0, q1, window=W2, reference=R2, which=())
        s.gain_latch()
        s.mpc_advance(stride)
        with pytest.raises(CimpcError):
            s.gain_latch()
    finally:
        s.close()
