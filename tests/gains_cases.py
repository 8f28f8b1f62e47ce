"""Inputs of the feedback-gain parity checks, shared by tests/test_gpu_gains.py and scripts/gains_parity.py: knots of the shipped gaits of
the 3-D cone models with the objective of examples/centroidal_quadruped/continuous_wall.jl:41-45 (its `relative_state_cost` Q is dense),
their torch linearization (`ContactModel.linearize_batch`) and the NumPy restatement's K, P1 (tests/gains_ref.py), each computed once.

The cases are the smallest shapes at which the kernels can still go wrong: nz = 66 is one column past a wavefront, n = 36 no multiple of
16, m = 12; nz = 114 the multi-wavefront, large-LDS case; nz = 19, n = 14, m = 3 the small one; one full chain of 710 steps; and the box
quadruped (plant id 7) stepping over its box.  The shapes no model has are in tests/gains_edge_cases.py."""
import functools
import os

import numpy as np

from contactimplicitmpc.jl_amd import gait_io, lcp_models
import gains_ref

GAIT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaits")
KAPPA = 2e-4      # does not enter the derivatives
TOL = 1e-9        # of max|K_ref| (and of max|P1_ref|): >= 150 x the movement of the restatement under last-place noise on its inputs

# name -> (model, gait file, kind, knots, N)
CASES = {
    "centroidal trot, knots 1-4, N = 2": ("centroidal_quadruped", "centroidal_inplace_trot_v7.jld2", "gait", 4, 2),
    "wall stand, knots 1-3, N = 2": ("centroidal_quadruped_wall", "wall_stand_FL_4.jld2", "gait", 3, 2),
    "hopper_3D in place, knots 1-5, N = 3": ("hopper_3D", "hopper_3D_gait_in_place.jld2", "traj", 5, 3),
    "centroidal trot, all knots, N = 10": ("centroidal_quadruped", "centroidal_inplace_trot_v7.jld2", "gait", None, 10),
    "box step-over, knots 1-3, N = 2": ("centroidal_quadruped_box", "step_over_box_v0.jld2", "gait", 3, 2),
}


def centroidal_weights():
    """obj.q[1], obj.v[1], obj.u[1] of continuous_wall.jl:41-45."""
    oq = lcp_models.relative_state_cost(1.0 * np.array([1e-2, 1e-2, 1.0]), 0.3 * np.ones(3), 1.0 * np.array([0.1, 0.1, 1.0]))
    ov = np.diag(1e-3 * np.concatenate([np.ones(3), 1e3 * np.ones(3), np.ones(12)]))
    ou = np.diag(3e-3 * np.ones(12))
    return oq, ov, ou


def hopper_weights():
    """No hopper example of the reference turns the gains on, so these weights are chosen here: positions, orientation, leg length."""
    return np.diag([1.0, 1.0, 1.0, 0.3, 0.3, 0.3, 0.1]), np.diag(1e-3 * np.ones(7)), np.diag([1e-2, 1e-2, 1e-1])


@functools.lru_cache(maxsize=None)
def knots(model_name, file, kind):
    """(model, z, theta) of every knot of a shipped gait."""
    model = lcp_models.MODELS[model_name]()
    path = os.path.join(GAIT_DIR, file)
    if kind == "gait":
        P = lcp_models.reference_problem(model, gait_io.load_gait(path), KAPPA, tables=False)
        return model, P.z, P.theta
    t = gait_io.load_joint_traj(path)
    return model, t.z, t.theta


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(model, z, theta, rz0, rth0, weights, N, K, P1): inputs and the restatement's answer; read-only by agreement."""
    model_name, file, kind, n, N = CASES[name]
    model, z, th = knots(model_name, file, kind)
    n = z.shape[0] if n is None else n
    z, th = np.ascontiguousarray(z[:n]), np.ascontiguousarray(th[:n])
    _, rz0, rth0 = model.linearize_batch(z, th, KAPPA)
    rz0, rth0 = np.asarray(rz0, dtype=np.float64), np.asarray(rth0, dtype=np.float64)
    w = hopper_weights() if model_name == "hopper_3D" else centroidal_weights()
    K, P1 = gains_ref.reference_gains(model.nq, model.nu, rz0, rth0, *w, N=N, return_P1=True)
    out = dict(model=model, z=z, theta=th, rz0=rz0, rth0=rth0, weights=w, N=N, K=K, P1=P1)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
