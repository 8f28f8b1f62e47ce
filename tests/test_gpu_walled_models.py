"""Device plant step of pushbot and walledcartpole (CIMPC_PLANT_PUSHBOT / CIMPC_PLANT_WALLEDCARTPOLE) against the Newton solve of the
NumPy restatement (tests/walled_ref.py) on states around both walls, the three entry points, the controller on pushbot's real problem
tables and the two examples in closed loop with policy and plant on the device.  Tolerances are the plant tests' existing ones
(tests/test_gpu_plant_wall_box.py, tests/test_gpu_hopper_3d.py); the CPU sides are solved once per process (walled_ref.cpu_step_case)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import walled_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ("pushbot", "walledcartpole")
H_STEP = ref.H_STEP


@pytest.mark.parametrize("disturbed", [False, True])
@pytest.mark.parametrize("name", MODELS)
def test_device_step_matches_the_cpu_newton_solve(name, disturbed):
    """64 states per model, some starting 2 cm inside a wall, with and without a disturbance on every coordinate (four on the
    cart-pole): status equal to the CPU's and all converged, q2 to 1e-7, γ to 1e-5, and at least 8 robots end in contact, on both walls."""
    from contactimplicitmpc.jl_amd import plant
    mu = ref.PLANTS[name].mu_world
    q0, q1, u, w = ref.step_inputs(name, 0, 64, H_STEP, disturbed)
    assert w is None or w.shape == (64, plant.model_dims(name)[5])
    q2, gam, b, st, it = plant.plant_step(name, q0, q1, u, mu, H_STEP, w=w)
    ok, cq2, cg, cb, cit = ref.cpu_step_case(name, disturbed)
    touching = gam > 1e-3
    print(f"{name} (w {'on' if disturbed else 'off'}): iterations max {it.max()} (CPU {cit.max()}), in contact {touching.any(axis=1).sum()}, "
          f"max |dq2| = {np.abs(q2 - cq2).max():.3e}, max |dγ| = {np.abs(gam - cg).max():.3e}")
    np.testing.assert_array_equal(st.astype(bool), ok)
    assert ok.all() and np.all(it > 0)
    np.testing.assert_allclose(q2, cq2, rtol=0, atol=1e-7)
    np.testing.assert_allclose(gam, cg, rtol=0, atol=1e-5)
    assert touching.any(axis=1).sum() >= 8 and touching[:, 0].any() and touching[:, 1].any()


@pytest.mark.parametrize("name", MODELS)
def test_flat_terrain_is_the_flat_entry_and_every_other_terrain_is_refused(name):
    from contactimplicitmpc.jl_amd import _lib, plant
    mu = ref.PLANTS[name].mu_world
    q0, q1, u, w = ref.step_inputs(name, 0, 64, H_STEP, True)
    a = plant.plant_step(name, q0, q1, u, mu, H_STEP, w=w)
    f = plant.plant_step(name, q0, q1, u, mu, H_STEP, w=w, terrain="flat_2D_lc")
    assert a[3].all()
    for x, y in zip(a, f):
        np.testing.assert_array_equal(x, y)
    for terrain in ("sine1_2D_lc", "slope1_2D_lc", "sine2_3D_lc"):
        with pytest.raises(_lib.CimpcError):
            plant.plant_step(name, q0, q1, u, mu, H_STEP, w=w, terrain=terrain)


@pytest.mark.parametrize("name", MODELS)
def test_rollout_equals_the_loop_of_steps(name):
    """B = 8, T = 12 in chunks of 5 (two chunk boundaries), a per-robot u schedule held for N_sample = 2 steps, a w schedule whose
    fourth row pushes every robot's point towards a wall (some reach it), per-robot μ: bit for bit the loop of plant_step."""
    from contactimplicitmpc.jl_amd import plant
    _, nq, nu, nc, fd, nw = plant.model_dims(name)
    B, T, N = 8, 12, 2
    rng = np.random.default_rng(7)
    _, q1, _, _ = ref.step_inputs(name, 1, B, H_STEP)
    v1 = rng.uniform(-1.0, 1.0, (B, nq))
    u = rng.uniform(-1.0, 1.0, (T // N, B, nu))
    w = np.zeros((T, B, nw))
    w[3, :, 0] = np.linspace(-1.0, 1.0, B) * (2.0 if name == "pushbot" else 0.3)      # an impulse on θ, both signs
    mu = rng.uniform(0.1, 0.6, B)
    ok, q, ua, g, b, st, it = plant.rollout(name, q1, v1, u, H_STEP, mu, N_sample=N, w=w, steps_per_launch=5)
    assert ok and q.shape == (T + 2, B, nq) and (g.max(axis=(0, 2)) > 1e-3).any()
    qa, qb = q1 - H_STEP * v1, q1
    for t in range(T):
        assert np.array_equal(ua[t], u[t // N] / N)
        for r in range(B):                                                             # plant_step takes one μ: robot by robot
            one = plant.plant_step(name, qa[r:r + 1], qb[r:r + 1], ua[t, r:r + 1], mu[r], H_STEP, w=w[t, r:r + 1])
            for x, y in zip(one, (q[t + 2, r:r + 1], g[t, r:r + 1], b[t, r:r + 1], st[t, r:r + 1], it[t, r:r + 1])):
                np.testing.assert_array_equal(x, y)
        qa, qb = qb, q[t + 2]


def test_newton_solve_on_the_pushbot_problem():
    """newton_solve on the tables of examples/pushbot/push_recovery.jl (H 10, B 4, κ 1e-4, :configurationforce, the example's "fast
    recovery" velocity objective and Newton options, perturb 0.02) against oracle.newton on the same inputs, under the acceptance rule
    of test_newton_solve_on_real_problems: equal Newton iterations, at least half of the rollouts on the oracle's exact path (1e-6),
    all within its amplification band."""
    from common import make_solver
    from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, lcp_models
    from oracle import ip as oip, lcp, newton as onewton
    from oracle.dims import Dims
    from real_problems import real_rollout
    kappa, H, nB, h = 1e-4, 10, 4, 0.04
    m = lcp_models.PushBot()
    P = lcp_models.reference_problem(m, lcp_models.constant_reference(m, np.zeros(2), 100, h), kappa)
    d = Dims(nq=m.nq, nu=m.nu, nw=m.nw, nc=m.nc, nb=m.nb, mode=1)
    prob = dict(z0=P.z, th0=P.theta, r0=P.r0, rz0=P.rz0, rth0=P.rth0, kappa=kappa, P=P)
    tabs = [lcp.LinTable(d, P.z[t], P.theta[t], P.r0[t], P.rz0[t], P.rth0[t]) for t in range(P.H)]
    rng = np.random.default_rng(4)
    rollouts = [real_rollout(d, prob, H, int(rng.integers(0, P.H)), seed=10 + b, perturb=0.02) for b in range(nB)]
    tile = lambda rows: np.stack([np.diag(np.asarray(r, dtype=float)) for r in rows])
    obj = onewton.Objective(q=tile([[12.0 * ((t + 1) / H) ** 2] * 2 for t in range(H)]), u=tile([[100.0, 1.0]] * H),
                            gamma=tile([[1e-100] * 2] * H), b=tile([[1e-100] * 4] * H), v=tile([[1.0 / h ** 2, 0.01 / h ** 2]] * H))
    s = make_solver(d, prob, rollouts, H, obj=obj, ip_opts=InteriorPointOptions(kappa_tol=kappa, r_tol=1e-8),
                    newton_opts=NewtonOptions(kappa=kappa, r_tol=3e-4, max_iter=10))
    u1, it, rn = s.newton_solve(np.stack([r[2] for r in rollouts]), np.stack([r[3] for r in rollouts]))
    traj = s.trajectory()
    tight = 0
    for b, (window, rf, q0, q1) in enumerate(rollouts):
        core = onewton.Newton(d, H, obj, onewton.NewtonOptions(r_tol=3e-4, max_iter=10, solver="lu"),
                              oip.IPOptions(kappa_tol=kappa, r_tol=1e-8), kappa, rf)
        st = onewton.newton_solve(core, q0, q1, window, tabs, rf)
        dq = np.abs(traj["q"][b] - core.traj.q).max()
        du = np.abs(traj["u"][b] - core.traj.u).max() / max(1.0, np.abs(core.traj.u).max())
        print(f"rollout {b}: Newton iterations {it[b]} / {st.iters}, max |dq| = {dq:.3e}, |du| = {du:.3e}")
        assert it[b] == st.iters, (b, it[b], st.iters)
        assert dq < 1e-2 and du < 5e-2, (b, dq, du)
        tight += int(dq < 1e-6)
    assert tight >= nB // 2, (tight, nB)
    assert it.max() >= 1


@functools.lru_cache(maxsize=None)
def _closed_loop_module():
    spec = importlib.util.spec_from_file_location("closed_loop_pushbot", os.path.join(os.path.dirname(HERE), "scripts", "closed_loop_pushbot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("example", ["pushbot", "cartpole"])
def test_closed_loop_with_policy_and_plant_on_the_device(example):
    """examples/pushbot/push_recovery.jl and examples/cartpole/cartpole.jl, 4 robots, 400 plant steps (three impulses): every plant step
    converges, Newton stays within the example's iteration cap, no penetration (ϕ >= -1e-6).  Recovery is held to the reference
    algorithm's own: every robot stays within 1.5 x the max |θ| and the max |θ| over the last 50 steps of ITS CPU loop (oracle policy,
    walled_ref plant, the same impulses; tests/golden/make_walled_closed_loop.py), recorded in tests/golden/walled_closed_loop.json.
    The CPU loops recover between the impulses (pushbot: |θ| 0.011 at step 200, before the second push; cart-pole: 0.002), and the last
    50 steps follow the third impulse.  Measured on the device: the four robots' figures equal their CPU loops' to four digits
    (pushbot max |θ| 0.1976 / 0.3126 / 0.1952 / 0.2638, cart-pole 0.4810 / 0.4702 / 0.4613 / 0.4592)."""
    mod = _closed_loop_module()
    gold = json.load(open(os.path.join(HERE, "golden", "walled_closed_loop.json")))[example]
    S = mod.example_settings(example)
    assert gold["steps"] == 400 and len(gold["robots"]) == 4 and all(g["plant_converged"] for g in gold["robots"])
    assert all(np.array_equal(np.asarray(gold["settings"][k]), np.asarray(S[k])) for k in gold["settings"])
    ok, out = mod.run(example, robots=4, steps=400, verbose=True)
    assert ok
    for o, g in zip(out, gold["robots"]):
        print(f"{example} robot {g['robot']}: max |theta| {o['theta_abs_max']:.4f} (CPU loop {g['theta_abs_max']:.4f}), "
              f"last 50 steps {o['theta_abs_last50']:.4f} ({g['theta_abs_last50']:.4f})")
        assert o["plant_converged"]
        assert o["newton_iters_max"] <= S["newton_max_iter"]
        assert o["phi_min"] >= -1e-6
        assert o["theta_abs_max"] <= 1.5 * g["theta_abs_max"]
        assert o["theta_abs_last50"] <= 1.5 * g["theta_abs_last50"]
