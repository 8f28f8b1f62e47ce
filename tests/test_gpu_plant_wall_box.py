"""Device plant step of centroidal_quadruped_box and centroidal_quadruped_wall (CIMPC_PLANT_CENTROIDAL_BOX / _WALL) against the
Newton solve of the NumPy restatement (tests/centroidal_wall_box_ref.py) at the knots of the shipped gaits."""
import os

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import gait_io
from oracle import plant as pl
import centroidal_wall_box_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GAITS = {"centroidal_quadruped_wall": os.path.join(HERE, "golden", "gaits", "wall_stand_FL_4.jld2"),
         "centroidal_quadruped_box": os.path.join(HERE, "golden", "gaits", "step_over_box_v0.jld2")}
B = 32


def _batch(name, knots, payload):
    g = gait_io.load_gait(GAITS[name])
    t = np.asarray(knots)
    rng = np.random.default_rng(len(t))
    w = rng.uniform(-5.0, 5.0, (len(t), 3)) * g.h if payload else None      # a payload force on the body, as an impulse per step
    return g, g.q[t], g.q[t + 1], g.u[t], w


def _cpu(P, q0, q1, u, w, mu, h):
    out = [pl.plant_step(P, q0[i], q1[i], u[i], np.zeros(3) if w is None else w[i], mu, h, pl.SIM_OPTS) for i in range(len(q0))]
    return (np.array([o[0] for o in out]), np.array([o[2] for o in out]), np.array([o[3] for o in out]), np.array([o[4] for o in out]))


@pytest.mark.parametrize("payload", [False, True])
@pytest.mark.parametrize("name", sorted(GAITS))
def test_device_step_matches_the_cpu_newton_solve_at_the_gait_knots(name, payload):
    from contactimplicitmpc.jl_amd import plant
    H = gait_io.load_gait(GAITS[name]).H
    g, q0, q1, u, w = _batch(name, np.arange(B) * H // B, payload)
    q2, gam, b, st, it = plant.plant_step(name, q0, q1, u, g.mu, g.h, w=w)
    ok, cq2, cg, cb = _cpu(ref.PLANTS[name](), q0, q1, u, w, g.mu, g.h)
    np.testing.assert_array_equal(st.astype(bool), ok)
    assert ok.all() and np.all(it > 0)
    np.testing.assert_allclose(q2, cq2, rtol=0, atol=1e-7)
    np.testing.assert_allclose(gam, cg, rtol=0, atol=1e-5)


def test_box_far_from_the_step_is_the_centroidal_step_with_the_box_feet():
    """Every foot at x < 0.05, where e(x) = e'(x) = 0 in fp64: the box residual IS the centroidal residual with 0.5 kg feet
    (bit for bit on the CPU, tests/test_centroidal_wall_box.py).  The device box step equals the CPU Newton solve of that
    centroidal model to 1e-7 - not CIMPC_PLANT_CENTROIDAL, whose feet weigh 0.2 kg (centroidal_quadruped_box/model.jl:219)."""
    from contactimplicitmpc.jl_amd import plant
    g, q0, q1, u, w = _batch("centroidal_quadruped_box", np.arange(B), True)
    shift = np.zeros(18)
    shift[0::3] = -(max(q0[:, 6::3].max(), q1[:, 6::3].max()) + 0.1)              # x of the body and of every foot
    q0, q1 = q0 + shift, q1 + shift
    q2, gam, b, st, it = plant.plant_step("centroidal_quadruped_box", q0, q1, u, g.mu, g.h, w=w)
    assert q2[:, 6::3].max() < 0.05
    C = pl.CentroidalPlant(damped=True)
    C.mass_foot = 0.5
    ok, cq2, cg, cb = _cpu(C, q0, q1, u, w, g.mu, g.h)
    assert st.all() and ok.all()
    np.testing.assert_allclose(q2, cq2, rtol=0, atol=1e-7)


def test_wall_without_wall_contact_is_the_centroidal_plant():
    """Feet >= 0.08 m from the plane (the wall gait's first knots).  Each idle wall contact still carries gamma ~ kappa / phi:
    at convergence gamma phi < kappa_tol = 1e-8, so gamma < 1e-8 / 0.08 = 1.25e-7 N and sum b <= mu gamma.  Over one step that
    force moves a 0.2 kg foot by at most h^2 / m_f (1 + mu) gamma = 0.0125 * 1.3 * 1.25e-7 = 2e-9 m; each of the two solves is
    itself only converged to r_tol = 1e-8 on the momentum rows (h / m_f r_tol = 2.5e-9 m).  Bound: 1e-8."""
    from contactimplicitmpc.jl_amd import plant
    g, q0, q1, u, w = _batch("centroidal_quadruped_wall", np.arange(B) % 10, True)
    assert max(q0[:, 6::3].max(), q1[:, 6::3].max()) <= 0.25 - 0.08 + 1e-12
    q2w, gw, bw, stw, _ = plant.plant_step("centroidal_quadruped_wall", q0, q1, u, g.mu, g.h, w=w)
    q2c, gc, bc, stc, _ = plant.plant_step("centroidal_quadruped", q0, q1, u, g.mu, g.h, w=w)
    assert stw.all() and stc.all()
    assert gw[:, 4:].max() < 1e-8 / 0.08 * 1.01
    d = np.abs(q2w - q2c).max()
    print(f"wall without wall contact vs centroidal: max |dq2| = {d:.3e}, max idle wall gamma = {gw[:, 4:].max():.3e}")
    assert d < 1e-8
    np.testing.assert_allclose(gw[:, :4], gc, rtol=0, atol=1e-5)


def test_open_loop_replay_of_the_wall_gait_matches_the_cpu():
    """The wall gait's controls replayed from (q[0], q[1]) through the device plant (test/simulator/quadruped.jl does this for
    the quadruped), 4 robots with payloads 0, 1, 2, 3 kg: every step converges, the device trajectory equals the CPU Newton
    solve's step by step to 1e-7 at the end state, and the unloaded robot's body stays up.  A payload the open-loop controls do
    not carry sinks the body (nothing but u holds it; measured: 0.23 / -1.1 / -2.5 / -3.8 m after 2.5 s for 0 / 1 / 2 / 3 kg)."""
    from contactimplicitmpc.jl_amd import plant
    g = gait_io.load_gait(GAITS["centroidal_quadruped_wall"])
    P = ref.WallPlant()
    nr = 4
    w = np.zeros((nr, 3)); w[:, 2] = -9.81 * np.arange(nr) * g.h                 # payload weight as an impulse per step
    qa, qb = np.repeat(g.q[0:1], nr, 0), np.repeat(g.q[1:2], nr, 0)
    ca, cb = qa.copy(), qb.copy()
    for t in range(g.H):
        u = np.repeat(g.u[t:t + 1], nr, 0)
        q2, gam, b, st, it = plant.plant_step("centroidal_quadruped_wall", qa, qb, u, g.mu, g.h, w=w)
        ok, cq2, _, _ = _cpu(P, ca, cb, u, w, g.mu, g.h)
        assert st.all() and ok.all(), t
        qa, qb, ca, cb = qb, q2, cb, cq2
    d = np.abs(qb - cb).max()
    print(f"open-loop wall replay, {g.H} steps: max |q_dev - q_cpu| at the end = {d:.3e}; body z = {qb[:, 2]}")
    assert d < 1e-7
    assert qb[0, 2] > 0.2 and np.all(np.diff(qb[:, 2]) < 0.0)


@pytest.mark.parametrize("name", sorted(GAITS))
def test_terrain_entry_takes_flat_only_and_runs_the_same_step(name):
    from contactimplicitmpc.jl_amd import _lib, plant
    g, q0, q1, u, w = _batch(name, np.arange(4), False)
    a = plant.plant_step(name, q0, q1, u, g.mu, g.h)
    f = plant.plant_step(name, q0, q1, u, g.mu, g.h, terrain="flat_3D_lc")
    for x, y in zip(a, f):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(_lib.CimpcError):
        plant.plant_step(name, q0, q1, u, g.mu, g.h, terrain="sine1_2D_lc")


def test_wall_stand_closed_loop_with_policy_and_plant_on_the_device():
    """examples/centroidal_quadruped/continuous_wall.jl (H_mpc 5, N_sample 5, TrackingVelocityObjective of :41-51) without the
    example's `gains = true`: the discrete CIMPCPolicy on the wall model plus the device wall plant, 250 plant steps (the
    example's H_sim), 4 robots carrying 0 / 5 / 10 / 20 N.  Sized from one measured run: every plant step
    converges; Newton stops within its 5 iterations at a residual norm <= 2.0e-3; height drift <= 0.030 m; |orientation| <= 0.436
    rad (the gait pitches to 0.314); the front-left foot reaches the wall and pushes on it while the gait has it there."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("closed_loop_wall", os.path.join(os.path.dirname(HERE), "scripts", "closed_loop_wall.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ok, out = mod.run(250, (0.0, -5.0, -10.0, -20.0), verbose=True)
    assert ok
    for o in out:
        assert o["newton_iters_max"] <= 5 and o["newton_rnorm_max"] < 5e-3
        assert o["height_drift_max"] < 0.05 and o["orientation_max"] < 0.5
        assert abs(o["fl_x_max"] - 0.25) < 1e-3
        assert o["fl_wall_gamma_max_on_wall"] > 0.1                   # measured 0.267 - 0.292
