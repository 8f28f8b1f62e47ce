"""Device plant step of hopper_3D (CIMPC_PLANT_HOPPER_3D) against the Newton solve of the NumPy restatement (tests/hopper_3d_ref.py)
at the knots of the reference's gaits, the reference's simulator test on the device, terrain, and the controller on the model's real
problem tables.  Tolerances are the plant tests' existing ones (tests/test_gpu_plant_wall_box.py, tests/test_gpu_terrain.py)."""
import functools
import os

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import gait_io
from oracle import plant as pl
import hopper_3d_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B = 32
MU, H_STEP = 1.5, 0.01


@functools.lru_cache(maxsize=None)
def _gait(name):
    t = gait_io.load_joint_traj(os.path.join(HERE, "golden", "gaits", f"hopper_3D_{name}.jld2"))
    assert (t.theta[0, -2], t.theta[0, -1], t.h) == (MU, H_STEP, H_STEP)
    return t


def _cpu(P, q0, q1, u, w):
    out = [pl.plant_step(P, q0[i], q1[i], u[i], np.zeros(3) if w is None else w[i], MU, H_STEP, pl.SIM_OPTS) for i in range(len(q0))]
    return (np.array([o[0] for o in out]), np.array([o[2] for o in out]), np.array([o[3] for o in out]), np.array([o[1] for o in out]))


@functools.lru_cache(maxsize=None)
def _cpu_replay():
    """The in-place gait's controls replayed from (q[0], q[1]) by the CPU Newton solve: (all converged, q (H + 2, 7))."""
    t = _gait("gait_in_place")
    P = ref.Hopper3DPlant()
    q, ok = [t.q[0], t.q[1]], True
    for k in range(t.H):
        st, _, q2, _, _ = pl.plant_step(P, q[k], q[k + 1], t.u[k], np.zeros(3), MU, H_STEP, pl.SIM_OPTS)
        ok = ok and st
        q.append(q2)
    return ok, np.array(q)


@pytest.mark.parametrize("impulse", [False, True])
@pytest.mark.parametrize("name", ["gait_forward", "gait_in_place"])
def test_device_step_matches_the_cpu_newton_solve_at_the_gait_knots(name, impulse):
    from contactimplicitmpc.jl_amd import plant
    t = _gait(name)
    k = np.arange(B) * t.H // B
    w = np.random.default_rng(B).uniform(-5.0, 5.0, (B, 3)) * H_STEP if impulse else None
    q0, q1, u = t.q[k], t.q[k + 1], t.u[k]
    q2, gam, b, st, it = plant.plant_step("hopper_3D", q0, q1, u, MU, H_STEP, w=w)
    ok, cq2, cg, _ = _cpu(ref.Hopper3DPlant(), q0, q1, u, w)
    np.testing.assert_array_equal(st.astype(bool), ok)
    assert ok.all() and np.all(it > 0)
    np.testing.assert_allclose(q2, cq2, rtol=0, atol=1e-7)
    np.testing.assert_allclose(gam, cg, rtol=0, atol=1e-5)


def test_reference_simulator_test_on_the_device():
    """test/simulator/hopper_3D.jl: from (q[0], q[1]) of gait_in_place, T = 92 steps with no policy; `@test status`.  The body falls
    and the leg coordinate runs negative with it (the reference's behaviour): only the status is asserted, as there."""
    from contactimplicitmpc.jl_amd import plant
    t = _gait("gait_in_place")
    ok, q, u, g, b = plant.simulate("hopper_3D", lambda q: np.zeros((1, 3)), t.q[1:2], (t.q[1:2] - t.q[0:1]) / t.h, t.H, t.h, mu=MU)
    assert ok and q.shape == (t.H + 2, 1, 7)


def test_open_loop_replay_of_the_in_place_gait():
    """The in-place gait's own controls through the device plant: every step converges, the end state equals the CPU replay's to 1e-7
    and the gait's own q[H + 1] to 1e-5, the tolerance the gait was solved to (the CPU replay lands 4.6e-7 from it)."""
    from contactimplicitmpc.jl_amd import plant
    t = _gait("gait_in_place")
    cok, cq = _cpu_replay()
    qa, qb = t.q[0:1], t.q[1:2]
    for k in range(t.H):
        q2, gam, b, st, it = plant.plant_step("hopper_3D", qa, qb, t.u[k:k + 1], MU, H_STEP)
        assert st.all(), k
        qa, qb = qb, q2
    d_cpu, d_gait, c_gait = np.abs(qb[0] - cq[-1]).max(), np.abs(qb[0] - t.q[-1]).max(), np.abs(cq[-1] - t.q[-1]).max()
    print(f"open-loop in-place replay, {t.H} steps: |q_dev - q_cpu| = {d_cpu:.3e}, |q_dev - q_gait| = {d_gait:.3e}, |q_cpu - q_gait| = {c_gait:.3e}")
    assert cok
    assert d_cpu < 1e-7
    assert d_gait < 1e-5


def _sine_batch():
    """Every third knot of gait_forward, body x shifted by 0.13 t (the foot meets the sine at every phase) and z lifted by the
    sine's amplitude 0.075."""
    t = _gait("gait_forward")
    k = np.arange(0, t.H, 3)
    shift = np.zeros((len(k), 7)); shift[:, 0] = 0.13 * k; shift[:, 2] = 0.075
    return t.q[k] + shift, t.q[k + 1] + shift, t.u[k]


def test_step_on_the_sine_terrain_matches_the_cpu_newton_solve():
    from contactimplicitmpc.jl_amd import plant
    q0, q1, u = _sine_batch()
    assert len(q0) == 31
    q2, gam, b, st, it = plant.plant_step("hopper_3D", q0, q1, u, MU, H_STEP, terrain="sine2_3D_lc")
    ok, cq2, cg, cit = _cpu(ref.Hopper3DPlant("sine2_3D_lc"), q0, q1, u, None)
    print(f"sine2_3D_lc: CPU iterations max {cit.max()}, device max {it.max()}; max |dq2| = {np.abs(q2 - cq2).max():.3e}")
    np.testing.assert_array_equal(st.astype(bool), ok)
    assert ok.all() and np.all(it > 0)
    np.testing.assert_allclose(q2, cq2, rtol=0, atol=1e-7)
    np.testing.assert_allclose(gam, cg, rtol=0, atol=1e-5)


def test_one_terrain_per_robot_equals_single_calls():
    """Eight knots of gait_forward, each robot lifted onto its own terrain under its foot."""
    from contactimplicitmpc.jl_amd import plant, terrain
    names = ["flat_3D_lc", "sine2_3D_lc", "sine3_3D_lc", "flat_3D_lc", "quadratic_bowl_3D_lc", "sine2_3D_lc", "flat_3D_lc", "sine3_3D_lc"]
    t = _gait("gait_forward")
    k = np.arange(len(names)) * 11
    q0, q1, u = t.q[k].copy(), t.q[k + 1].copy(), t.u[k]
    q0[:, 0] += 0.13 * k; q1[:, 0] += 0.13 * k
    foot = ref.Hopper3DPlant().foot(q1)
    for i, name in enumerate(names):
        s = terrain.get(name).surface(foot[i, 0], foot[i, 1])
        q0[i, 2] += s; q1[i, 2] += s
    many = plant.plant_step("hopper_3D", q0, q1, u, MU, H_STEP, terrain=names)
    assert many[3].all()
    for i, name in enumerate(names):
        one = plant.plant_step("hopper_3D", q0[i:i + 1], q1[i:i + 1], u[i:i + 1], MU, H_STEP, terrain=name)
        for x, y in zip(many, one):
            np.testing.assert_array_equal(x[i:i + 1], y)
    # a robot's terrain matters: robot 1 on flat ground lands elsewhere
    flat1 = plant.plant_step("hopper_3D", q0[1:2], q1[1:2], u[1:2], MU, H_STEP)
    assert np.abs(flat1[0] - many[0][1:2]).max() > 1e-6


def test_flat_terrain_is_the_flat_entry_and_planar_terrains_are_refused():
    from contactimplicitmpc.jl_amd import _lib, plant
    t = _gait("gait_forward")
    q0, q1, u = t.q[0:4], t.q[1:5], t.u[0:4]
    a = plant.plant_step("hopper_3D", q0, q1, u, MU, H_STEP)
    f = plant.plant_step("hopper_3D", q0, q1, u, MU, H_STEP, terrain="flat_3D_lc")
    for x, y in zip(a, f):
        np.testing.assert_array_equal(x, y)
    for name in ("sine1_2D_lc", "slope1_2D_lc"):
        with pytest.raises(_lib.CimpcError):
            plant.plant_step("hopper_3D", q0, q1, u, MU, H_STEP, terrain=name)


def test_newton_solve_on_the_in_place_problem():
    """newton_solve on the tables of gait_in_place (H 20, B 4, κ 1e-4, the objective and options of examples/hopper/3D_flat.jl,
    perturb 0.02) against oracle.newton on the same inputs, under the acceptance rule of test_newton_solve_on_real_problems: equal
    Newton iterations, at least half of the rollouts on the oracle's exact path (1e-6), all within its amplification band."""
    from common import make_solver
    from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, lcp_models
    from oracle import ip as oip, lcp, newton as onewton, synth
    from oracle.dims import Dims
    from real_problems import real_rollout
    kappa, H, nB = 1e-4, 20, 4
    m = lcp_models.Hopper3D()
    P = lcp_models.reference_problem_from_traj(m, _gait("gait_in_place"), kappa)
    d = Dims(nq=m.nq, nu=m.nu, nw=m.nw, nc=m.nc, nb=m.nb, mode=0)
    prob = dict(z0=P.z, th0=P.theta, r0=P.r0, rz0=P.rz0, rth0=P.rth0, kappa=kappa, P=P)
    tabs = [lcp.LinTable(d, P.z[t], P.theta[t], P.r0[t], P.rz0[t], P.rth0[t]) for t in range(P.H)]
    rng = np.random.default_rng(4)
    rollouts = [real_rollout(d, prob, H, int(rng.integers(0, P.H)), seed=10 + b, perturb=0.02) for b in range(nB)]
    obj = synth.make_objective(d, H)
    obj.q = np.tile(np.diag(0.1 * np.array([3.0, 3.0, 0.1, 50.0, 50.0, 50.0, 10.0]))[None], (H, 1, 1))
    obj.u = np.tile(np.diag([0.1, 0.1, 10.0])[None], (H, 1, 1))
    obj.__post_init__()
    s = make_solver(d, prob, rollouts, H, obj=obj, ip_opts=InteriorPointOptions(kappa_tol=kappa, r_tol=1e-4),
                    newton_opts=NewtonOptions(kappa=kappa, r_tol=3e-4, max_iter=5))
    u1, it, rn = s.newton_solve(np.stack([r[2] for r in rollouts]), np.stack([r[3] for r in rollouts]))
    traj = s.trajectory()
    tight = 0
    for b, (window, rf, q0, q1) in enumerate(rollouts):
        core = onewton.Newton(d, H, obj, onewton.NewtonOptions(r_tol=3e-4, max_iter=5, solver="condensed"),
                              oip.IPOptions(kappa_tol=kappa, r_tol=1e-4), kappa, rf)
        st = onewton.newton_solve(core, q0, q1, window, tabs, rf)
        dq = np.abs(traj["q"][b] - core.traj.q).max()
        du = np.abs(traj["u"][b] - core.traj.u).max() / max(1.0, np.abs(core.traj.u).max())
        print(f"rollout {b}: Newton iterations {it[b]} / {st.iters}, max |dq| = {dq:.3e}, |du| = {du:.3e}")
        assert it[b] == st.iters, (b, it[b], st.iters)
        assert dq < 1e-2 and du < 5e-2, (b, dq, du)
        tight += int(dq < 1e-6)
    assert tight >= nB // 2, (tight, nB)
    assert it.max() >= 1


def test_closed_loop_with_policy_and_plant_on_the_device():
    """examples/hopper/3D_flat.jl, 4 robots, 300 plant steps: every plant step converges, Newton stays within its 5 iterations, and
    the physical conditions hold - no penetration (ϕ >= -1e-6), |p| < 0.2 (under 45°), the body more than 0.2 m above its foot.
    Then 3D_sine.jl's terrain: every plant step converges; the rest is recorded."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("closed_loop_hopper3d", os.path.join(os.path.dirname(HERE), "scripts", "closed_loop_hopper3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ok, out = mod.run("flat", robots=4, steps=300, verbose=True)
    assert ok
    for o in out:
        assert o["plant_converged"]
        assert o["newton_iters_max"] <= 5
        assert o["phi_min"] >= -1e-6
        assert o["mrp_norm_max"] < 0.2
        assert o["body_above_foot_min"] > 0.2
    ok, out = mod.run("sine2", robots=4, steps=300, verbose=True)
    assert ok
