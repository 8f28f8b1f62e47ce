"""`plant.rollout` (`cimpc_plant_rollout`: T plant steps in one call, every intermediate state on the device) against the host loop of
`plant.plant_step` that `plant.simulate` makes.  A rollout step IS the plant step - one kernel, the `n = 1` launch of it - so every
comparison with the loop is `assert_array_equal` on q, gamma, b, status and iters.  The shapes are the smallest at which the step loop
can go wrong: more than one robot, more steps than one launch, a launch of one step, both wavefront counts, every ground."""
import dataclasses
import functools
import os

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import gait_io
from oracle import plant as pl
from real_problems import real_problem

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GAIT_DIR = os.path.join(HERE, "golden", "gaits")


def _loop(model, q1, v1, u_applied, h, mu, w=None, opts=None, terrain=None):
    """What `simulate` does with these controls: one `plant_step` call per step (per robot too where friction or terrain is per robot).
    u_applied (T, B, nu), w None or (T, B, nw) -> q (T + 2, B, nq), gamma, b, status, iters."""
    from contactimplicitmpc.jl_amd import plant
    kw = {} if opts is None else {"opts": opts}
    B = q1.shape[0]
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,))
    per_robot = len(set(mu)) > 1 or (terrain is not None and not isinstance(terrain, str))
    groups = [[i] for i in range(B)] if per_robot else [list(range(B))]
    q = [q1 - h * v1, q1.copy()]
    out = [[], [], [], []]
    for t in range(u_applied.shape[0]):
        parts = [plant.plant_step(model, q[t][g], q[t + 1][g], u_applied[t][g], mu[g[0]], h, w=None if w is None else w[t][g],
                                  terrain=(terrain[g[0]] if per_robot and terrain is not None else terrain), **kw) for g in groups]
        q2, *rest = (np.concatenate([p[k] for p in parts]) for k in range(5))
        q.append(q2)
        for o, r in zip(out, rest):
            o.append(r)
    return (np.array(q), *(np.array(o) for o in out))


def _same(roll, loop):
    """(ok, q, u_applied, gamma, b, status, iters) of `rollout` against (q, gamma, b, status, iters) of `_loop`, bit for bit"""
    ok, q, ua, g, b, st, it = roll
    for name, x, y in zip(("q", "gamma", "b", "status", "iters"), (q, g, b, st, it), loop):
        np.testing.assert_array_equal(x, y, err_msg=name)
    assert ok == bool(loop[3].all())


def _policy_controls(u, N_sample, T, B):
    """`OpenLoopPolicy` called for t = 1 .. T: (T, B, nu)"""
    from contactimplicitmpc.jl_amd import plant
    pol = plant.OpenLoopPolicy(list(u), N_sample=N_sample)
    return np.array([np.broadcast_to(pol(t + 1), (B, u.shape[-1])) for t in range(T)])


# ---- hopper_2D at gait knots: B = 3, K = 4 controls held N_sample = 2 steps, 7 steps -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hopper(shared):
    tr = gait_io.load_joint_traj(os.path.join(GAIT_DIR, "hopper_gait_forward.jld2"))
    knots = np.array([0, 9, 20])
    q1, v1 = tr.q[knots + 1], (tr.q[knots + 1] - tr.q[knots]) / tr.h
    u = tr.u[:4] if shared else np.stack([tr.u[knots + k] for k in range(4)])          # (4, nu) | (4, 3, nu)
    h, mu = tr.h / 2, pl.HopperPlant().mu_world
    return q1, v1, u, h, mu, _loop("hopper_2D", q1, v1, _policy_controls(u, 2, 7, 3), h, mu)


@pytest.mark.parametrize("shared,steps_per_launch", [(False, 0), (True, 0), (False, 3), (False, 1), (True, 3)])
def test_hopper_rollout_is_the_plant_step_loop(shared, steps_per_launch):
    """per-robot and shared controls; launches of 7, of 3 + 3 + 1 and of 1 step"""
    from contactimplicitmpc.jl_amd import plant
    q1, v1, u, h, mu, loop = _hopper(shared)
    roll = plant.rollout("hopper_2D", q1, v1, u, h, mu, N_sample=2, steps=7, steps_per_launch=steps_per_launch)
    _same(roll, loop)
    assert roll[0] and roll[1].shape == (9, 3, 4) and roll[3].shape == (7, 3, 1) and roll[4].shape == (7, 3, 2) and roll[5].shape == (7, 3)
    np.testing.assert_array_equal(roll[2], _policy_controls(u, 2, 7, 3))
    np.testing.assert_array_equal(roll[1][0], q1 - h * v1)
    np.testing.assert_array_equal(roll[1][1], q1)
    assert np.abs(roll[1][8] - roll[1][1]).max() > 1e-6 and np.all(roll[6] > 0)          # it moved, and every step iterated


def test_one_step_is_one_plant_step_and_one_robot_is_a_batch_of_one():
    from contactimplicitmpc.jl_amd import plant
    q1, v1, u, h, mu, loop = _hopper(False)
    ok, q, ua, g, b, st, it = plant.rollout("hopper_2D", q1, v1, u[:1], h, mu, N_sample=2, steps=1)
    q2, g1, b1, st1, it1 = plant.plant_step("hopper_2D", q1 - h * v1, q1, u[0] / 2, mu, h)
    for x, y in ((q[2], q2), (g[0], g1), (b[0], b1), (st[0], st1), (it[0], it1)):
        np.testing.assert_array_equal(x, y)
    assert q.shape == (3, 3, 4)
    for r in range(3):                                                 # B = 1: robot r alone, with its own column of the controls
        one = plant.rollout("hopper_2D", q1[r], v1[r], u[:, r], h, mu, N_sample=2, steps=7, steps_per_launch=4)
        _same(one, tuple(x[:, r:r + 1] for x in loop))


def test_steps_that_do_not_converge_are_reported_and_the_rollout_goes_on():
    from contactimplicitmpc.jl_amd import plant
    q1, v1, u, h, mu, _ = _hopper(False)
    q1, v1, u = q1[:2], v1[:2], u[:, :2]
    opts = dataclasses.replace(plant.SIM_OPTS, max_iter=1)
    roll = plant.rollout("hopper_2D", q1, v1, u, h, mu, N_sample=2, steps=3, opts=opts, steps_per_launch=2)
    assert roll[0] is False and not roll[5].any() and np.all(roll[6] == 1)
    _same(roll, _loop("hopper_2D", q1, v1, _policy_controls(u, 2, 3, 2), h, mu, opts=opts))
    assert np.abs(roll[1][4] - roll[1][3]).max() > 0.0                  # the state still advances


# ---- the two ENV instantiations: the wall on two wavefronts, the box --------------------------------------------------------------------
@pytest.mark.parametrize("name,gait", [("centroidal_quadruped_wall", "wall_stand_FL_4"), ("centroidal_quadruped_box", "step_over_box_v0")])
def test_wall_and_box_rollout_is_the_plant_step_loop(name, gait):
    from contactimplicitmpc.jl_amd import plant
    g = gait_io.load_gait(os.path.join(GAIT_DIR, gait + ".jld2"))
    knots = np.arange(2) * g.H // 2
    q1, v1 = g.q[knots + 1], (g.q[knots + 1] - g.q[knots]) / g.h
    u = np.stack([g.u[knots + k] for k in range(3)])
    w = np.random.default_rng(2).uniform(-5.0, 5.0, (3, 2, 3)) * g.h                     # a payload force on the body, per step and robot
    roll = plant.rollout(name, q1, v1, u, g.h, g.mu, w=w, steps_per_launch=2)
    _same(roll, _loop(name, q1, v1, u, g.h, g.mu, w=w))
    assert roll[0] and roll[1].shape == (5, 2, 18)


# ---- TERRAIN: per-robot terrains (one flat), hopper_3D on its own instantiation ------------------------------------------------------------
def test_quadruped_on_per_robot_terrains():
    from contactimplicitmpc.jl_amd import plant, terrain
    d, P, *_ = real_problem("quadruped", 2e-4, False, 0)
    names = ["flat_2D_lc", "sine1_2D_lc"]
    knots = np.array([0, 4])
    Pq, Pu = np.asarray(P.q), np.asarray(P.u)
    q0, q1 = Pq[knots].copy(), Pq[knots + 1].copy()
    for k, n in enumerate(names):
        q0[k, 0] += 0.3 + k; q1[k, 0] += 0.3 + k
        s = terrain.get(n).surface(q1[k, 0])
        q0[k, 1] += s; q1[k, 1] += s
    h, v1 = P.h / 5, (q1 - q0) / P.h
    u = np.stack([Pu[knots + k] for k in range(4)]) / 5
    roll = plant.rollout("quadruped", q1, v1, u, h, 1.0, terrain=names, steps_per_launch=3)
    _same(roll, _loop("quadruped", q1, v1, u, h, 1.0, terrain=names))
    flat = plant.rollout("quadruped", q1, v1, u, h, 1.0)
    np.testing.assert_array_equal(roll[1][:, 0], flat[1][:, 0])          # the flat robot of a rough batch makes the flat step
    assert np.abs(roll[1][-1, 1] - flat[1][-1, 1]).max() > 1e-6          # and the other one stands on its sine


def test_hopper_3d_on_the_sine_terrain():
    from contactimplicitmpc.jl_amd import plant
    t = gait_io.load_joint_traj(os.path.join(GAIT_DIR, "hopper_3D_gait_forward.jld2"))
    knots = np.array([3, 12])
    shift = np.zeros((2, 7)); shift[:, 0] = 0.13 * knots; shift[:, 2] = 0.075      # as tests/test_gpu_hopper_3d.py puts the gait on the sine
    q1, v1 = t.q[knots + 1] + shift, (t.q[knots + 1] - t.q[knots]) / t.h
    u = np.stack([t.u[knots + k] for k in range(3)])
    roll = plant.rollout("hopper_3D", q1, v1, u, t.h, 1.5, terrain="sine2_3D_lc", steps_per_launch=2)
    _same(roll, _loop("hopper_3D", q1, v1, u, t.h, 1.5, terrain="sine2_3D_lc"))
    assert roll[1].shape == (5, 2, 7)


# ---- per-robot friction and a disturbance schedule ------------------------------------------------------------------------------------------
def test_particle_with_per_robot_friction_and_an_impulse():
    from contactimplicitmpc.jl_amd import plant
    q1 = np.array([[0.0, 0.0, 0.002], [0.1, 0.0, 0.0]]); v1 = np.array([[1.0, 2.0, 0.0], [1.0, 2.0, 0.0]])
    mu, h, T = np.array([1.0, 0.1]), 0.01, 6
    u = np.zeros((1, 3))
    w = np.zeros((T, 2, 3)); w[2, 1] = [0.02, -0.01, 0.03]                  # simulator step 3 (1-based), robot 1 only
    roll = plant.rollout("particle", q1, v1, u, h, mu, w=w, steps=T, steps_per_launch=4)
    ua = np.zeros((T, 2, 3))
    _same(roll, _loop("particle", q1, v1, ua, h, mu, w=w))
    calm = plant.rollout("particle", q1, v1, u, h, mu, steps=T)
    _same(calm, _loop("particle", q1, v1, ua, h, mu))
    np.testing.assert_array_equal(roll[1][:4], calm[1][:4])                # rows before step 3's outcome
    np.testing.assert_array_equal(roll[1][:, 0], calm[1][:, 0])             # robot 0 is never pushed
    assert np.all(np.abs(roll[1][4:, 1] - calm[1][4:, 1]).max(axis=1) > 1e-6)
    same_mu = plant.rollout("particle", q1, v1, u, h, 1.0, steps=T)
    np.testing.assert_array_equal(same_mu[1][:, 0], calm[1][:, 0])
    assert np.abs(same_mu[1][-1, 1] - calm[1][-1, 1]).max() > 1e-6          # friction is the robot's own
    held = plant.rollout("particle", q1, v1, u, h, mu, w=w[:3], w_hold=2, steps=T)      # rows 0 0 1 1 2 2: the impulse at steps 5 and 6
    np.testing.assert_array_equal(held[1][:6], calm[1][:6])
    assert np.abs(held[1][6, 1] - calm[1][6, 1]).max() > 1e-6


# ---- the reference's simulator tests, each in one call ---------------------------------------------------------------------------------------
def test_reference_simulator_test_quadruped_open_loop_in_one_call():
    """test/simulator/quadruped.jl:22-35: gait2's own controls (mu_world = 0.5) over T = H steps end within 0.025 of the reference's
    final base configuration; two robots side by side are identical, and the call equals the `simulate`-based replay of
    tests/test_gpu_plant.py."""
    from contactimplicitmpc.jl_amd import plant
    d, P, prob, tabs = real_problem("quadruped", 2e-4, True)
    q1 = np.stack([P.q[1], P.q[1]])
    v1 = np.stack([(P.q[1] - P.q[0]) / P.h] * 2)
    ok, q, ua, g, b, st, it = plant.rollout("quadruped", q1, v1, np.asarray(P.u), P.h, 0.5)
    assert ok and q.shape == (P.H + 2, 2, d.nq)
    assert np.abs(P.q[-1][:3] - q[-1, 0, :3]).max() < 0.025
    np.testing.assert_array_equal(q[:, 0], q[:, 1])
    pol = plant.OpenLoopPolicy(list(P.u))
    step = [0]
    def policy(qq):
        step[0] += 1
        return np.tile(pol(step[0]), (qq.shape[0], 1))
    ok_s, q_s, u_s, g_s, b_s = plant.simulate("quadruped", policy, q1, v1, P.H, P.h, mu=0.5)
    assert ok_s
    for x, y in ((q, q_s), (ua, u_s), (g, g_s), (b, b_s)):
        np.testing.assert_array_equal(x, y)


def test_reference_simulator_test_particle_in_one_call():
    """test/simulator/particle.jl:1-30: DROP and SLIDE side by side, 100 steps (two launches)"""
    from contactimplicitmpc.jl_amd import plant
    h, T = 0.01, 100
    q1 = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]); v1 = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.0]])
    ok, q, *_ = plant.rollout("particle", q1, v1, np.zeros((1, 3)), h, 1.0, steps=T)
    assert ok and q.shape == (T + 2, 2, 3)
    assert np.all(np.abs(q[-1, 0]) < 1e-6)                                               # dropped: at rest at the origin
    assert abs(q[-1, 1, 2]) < 1e-6 and np.all(np.abs((q[-1, 1] - q[-2, 1]) / h) < 1e-6)   # slid: on the ground, stopped
    okc, qc, *_ = pl.simulate(pl.ParticlePlant(), lambda qq, t: np.zeros(3), q1[1], v1[1], T, h)
    np.testing.assert_allclose(q[:, 1], qc, rtol=0, atol=1e-7)                          # and the same path as the CPU restatement
