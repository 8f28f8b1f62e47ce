"""-m gpu: the device plant step on terrain (`cimpc_plant_step_terrain`) against the CPU restatement of
tests/terrain_ref.py, its flat path against `cimpc_plant_step`, the reference's two terrain simulator tests and the closed loop
with the altitude update."""
import numpy as np
import pytest

from oracle import ip as oip
from oracle import plant as pl, synth
from real_problems import real_problem
import terrain_ref

pytestmark = pytest.mark.gpu

O_CPU = oip.IPOptions(r_tol=1e-8, kappa_tol=1e-8, undercut=np.inf, gamma_reg=0.1, eps_min=0.25, max_iter=100, max_ls=25)


def _check_against_cpu(model, name, q0, q1, u, mu, h):
    from contactimplicitmpc.jl_amd import plant
    q2, g, b, st, it = plant.plant_step(model, q0, q1, u, mu, h, terrain=name)
    assert st.all()
    cpu = terrain_ref.plant(model, name)
    for k in range(q0.shape[0]):
        s_, i_, q2c, gc, bc = pl.plant_step(cpu, q0[k], q1[k], u[k], np.zeros(cpu.nw), mu, h, O_CPU)
        assert s_ and abs(int(it[k]) - i_) <= 1, (k, int(it[k]), i_)
        np.testing.assert_allclose(q2[k], q2c, rtol=0, atol=1e-7)
        np.testing.assert_allclose(g[k], gc, rtol=0, atol=1e-5 * max(1.0, np.abs(gc).max()))
        np.testing.assert_allclose(b[k], bc, rtol=0, atol=1e-5 * max(1.0, np.abs(bc).max()))


def _on_terrain(name, q):
    """Lift gait configurations by the terrain height under the hip, so the feet meet the terrain."""
    from contactimplicitmpc.jl_amd import terrain
    q = q.copy()
    q[:, 1] += terrain.get(name).surface(q[:, 0])
    return q


@pytest.mark.parametrize("model,which,mu,name", [("quadruped", "quadruped", 1.0, "sine1_2D_lc"),
                                                 ("quadruped", "quadruped", 1.0, "piecewise1_2D_lc"),
                                                 ("quadruped", "quadruped", 1.0, "slope_smooth_2D_lc"),
                                                 ("flamingo", "flamingo", 0.9, "sine3_2D_lc")])
def test_terrain_step_of_the_chains_matches_the_cpu_restatement(gpu_required, model, which, mu, name):
    d, P, prob, tabs = real_problem(which, 2e-4, False, 0)
    knots = [0, 7, 19, 33, 48, 57]
    rng = np.random.default_rng(3)
    shift = np.array([0.0, 0.35, 0.7, 1.05, 1.4, 1.95])           # spread the robots over the terrain's features
    q0 = np.stack([P.q[t] for t in knots]); q1 = np.stack([P.q[t + 1] for t in knots]) + 1e-3 * rng.standard_normal((len(knots), d.nq))
    q0[:, 0] += shift; q1[:, 0] += shift
    q0, q1 = _on_terrain(name, q0), _on_terrain(name, q1)
    u = np.stack([P.u[t] for t in knots])
    _check_against_cpu(model, name, q0, q1, u, mu, P.h / 5)


@pytest.mark.parametrize("model,name,nq,nu", [("hopper_2D", "sine2_2D_lc", 4, 2), ("hopper_2D", "piecewise2_2D_lc", 4, 2),
                                              ("particle_2D", "slope1_2D_lc", 2, 2), ("particle_2D", "stairs3_2D_lc", 2, 2),
                                              ("particle", "quadratic_bowl_3D_lc", 3, 3), ("particle", "sine3_3D_lc", 3, 3),
                                              ("particle", "sine1_3D_lc", 3, 3)])
def test_terrain_step_of_the_small_models_matches_the_cpu_restatement(gpu_required, model, name, nq, nu):
    from contactimplicitmpc.jl_amd import terrain
    T = terrain.get(name)
    rng = np.random.default_rng(7)
    n, h = 6, 0.01
    q1 = np.zeros((n, nq))
    q1[:, 0] = np.linspace(-0.2, 2.3, n) if model != "particle" else rng.uniform(-1.0, 1.0, n)
    if model == "particle":
        q1[:, 1] = rng.uniform(-1.0, 1.0, n)
        q1[:, 2] = T.surface(q1[:, 0], q1[:, 1]) + rng.uniform(-0.01, 0.02, n)
    elif model == "hopper_2D":
        q1[:, 2] = rng.uniform(-0.2, 0.2, n); q1[:, 3] = 0.5
        q1[:, 1] = T.surface(q1[:, 0] + 0.5 * np.sin(q1[:, 2])) + 0.5 * np.cos(q1[:, 2]) + rng.uniform(-0.01, 0.02, n)
    else:
        q1[:, 1] = T.surface(q1[:, 0]) + rng.uniform(-0.01, 0.02, n)
    v = rng.uniform(-0.5, 0.5, (n, nq))
    q0 = q1 - h * v
    u = rng.uniform(-1.0, 1.0, (n, nu))
    if model == "hopper_2D":
        u[:, 1] += 3.3 * 9.81 * 0.2
    _check_against_cpu(model, name, q0, q1, u, 0.8 if model == "hopper_2D" else 0.5, h)


@pytest.mark.parametrize("model", ["quadruped", "flamingo", "hopper_2D", "centroidal_quadruped", "centroidal_quadruped_undamped", "particle"])
def test_flat_terrain_through_the_new_entry_is_bit_identical(gpu_required, model):
    from contactimplicitmpc.jl_amd import plant
    mid, nq, nu, nc, fd, nw = plant.MODELS[model]
    rng = np.random.default_rng(11)
    B = 8
    if model in ("quadruped", "flamingo"):
        d, P, *_ = real_problem(model, 2e-4, False, 0)
        q0 = np.stack([P.q[t] for t in range(B)]); q1 = np.stack([P.q[t + 1] for t in range(B)]) + 1e-3 * rng.standard_normal((B, nq))
        u = np.stack([P.u[t] for t in range(B)]); h = P.h
    else:
        q1 = rng.uniform(-0.1, 0.1, (B, nq)); h = 0.01
        if model == "hopper_2D":
            q1[:, 1] += 0.5; q1[:, 3] = 0.5
        if model == "particle":
            q1[:, 2] = rng.uniform(-0.01, 0.02, B)
        if model.startswith("centroidal"):
            d, P, *_ = real_problem("centroidal", 1e-3, False, 0)
            q1 = np.stack([P.q[t + 1] for t in range(B)]) + 1e-3 * rng.standard_normal((B, nq)); h = P.h
        q0 = q1 - h * rng.uniform(-0.3, 0.3, (B, nq))
        u = rng.uniform(-0.5, 0.5, (B, nu))
    w = rng.uniform(-0.5, 0.5, (B, nw))
    ref = plant.plant_step(model, q0, q1, u, 0.7, h, w=w)
    flat = "flat_3D_lc" if model in ("particle", "centroidal_quadruped", "centroidal_quadruped_undamped") else "flat_2D_lc"
    for ter in (flat, [flat] * B):
        got = plant.plant_step(model, q0, q1, u, 0.7, h, w=w, terrain=ter)
        for a, b in zip(ref, got):
            np.testing.assert_array_equal(a, b)
    assert ref[3].all()


def test_one_terrain_per_robot_equals_single_calls(gpu_required):
    from contactimplicitmpc.jl_amd import plant, terrain
    d, P, *_ = real_problem("quadruped", 2e-4, False, 0)
    names = ["flat_2D_lc", "sine1_2D_lc", "piecewise1_2D_lc", "sine3_2D_lc", "piecewise2_2D_lc", "slope_smooth_2D_lc"]
    B = len(names)
    rng = np.random.default_rng(5)
    q0 = np.stack([P.q[4 * t] for t in range(B)]); q1 = np.stack([P.q[4 * t + 1] for t in range(B)]) + 1e-3 * rng.standard_normal((B, d.nq))
    shift = np.linspace(0.3, 2.0, B)
    q0[:, 0] += shift; q1[:, 0] += shift
    for k, n in enumerate(names):
        s = terrain.get(n).surface(q1[k, 0])
        q0[k, 1] += s; q1[k, 1] += s
    u = np.stack([P.u[4 * t] for t in range(B)])
    many = plant.plant_step("quadruped", q0, q1, u, 1.0, P.h / 5, terrain=names)
    assert many[3].all()
    for k, n in enumerate(names):
        one = plant.plant_step("quadruped", q0[k:k + 1], q1[k:k + 1], u[k:k + 1], 1.0, P.h / 5, terrain=n)
        for a, b in zip(many, one):
            np.testing.assert_array_equal(a[k:k + 1], b)
    # a robot's terrain matters: robot 1 on flat ground lands elsewhere
    flat1 = plant.plant_step("quadruped", q0[1:2], q1[1:2], u[1:2], 1.0, P.h / 5)
    assert np.abs(flat1[0] - many[0][1:2]).max() > 1e-6


def test_refusals(gpu_required):
    import ctypes as C
    from contactimplicitmpc.jl_amd import _lib, plant, terrain
    z = lambda n: np.zeros(n)
    q = np.zeros((2, 18)); u = np.zeros((2, 12))
    with pytest.raises(_lib.CimpcError):                         # centroidal ignores the environment in the reference
        plant.plant_step("centroidal_quadruped", q, q, u, 0.3, 0.01, terrain="sine1_2D_lc")
    with pytest.raises(_lib.CimpcError):
        plant.plant_step("centroidal_quadruped", q, q, u, 0.3, 0.01, terrain="quadratic_bowl_3D_lc")
    with pytest.raises(_lib.CimpcError):                         # a 3-D surface under a planar model
        plant.plant_step("quadruped", np.zeros((1, 11)), np.zeros((1, 11)), np.zeros((1, 8)), 1.0, 0.01, terrain="sine1_3D_lc")
    lib = _lib.load()
    opts = _lib.IpOpts(**__import__("dataclasses").asdict(plant.SIM_OPTS))
    B, nq, nu = 3, 11, 8
    q0, q1, uu = z(B * nq), z(B * nq), z(B * nu)
    q2, g, b, st, it = z(B * nq), z(B * 4), z(B * 8), np.zeros(B, np.int32), np.zeros(B, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    def call(ts, n):
        arr = (_lib.Terrain * max(len(ts), 1))(*ts)
        return lib.cimpc_plant_step_terrain(0, B, n, arr, dp(q0), dp(q1), dp(uu), None, 1.0, 0.01, C.byref(opts), dp(q2), dp(g), dp(b), ip(st), ip(it))
    good = terrain.get("sine1_2D_lc").to_c()
    assert call([good], 1) == 0 and call([good] * 3, 3) == 0
    assert call([good, good], 2) == -1                           # CIMPC_ERR_INVALID: neither 1 nor B terrains
    assert call([good], 0) == -1
    bad = terrain.get("sine1_2D_lc").to_c(); bad.kind = 42
    assert call([bad], 1) == -1
    nan = terrain.get("sine1_2D_lc").to_c(); nan.p[0] = float("nan")
    assert call([nan], 1) == -1
    pw = terrain.get("piecewise1_2D_lc").to_c(); pw.n_pieces = 9
    assert call([pw], 1) == -1
    assert lib.cimpc_plant_step_terrain(0, B, 1, None, dp(q0), dp(q1), dp(uu), None, 1.0, 0.01, C.byref(opts), dp(q2), dp(g), dp(b),
                                        ip(st), ip(it)) == -1
    # the flat entry does not take particle_2D
    assert lib.cimpc_plant_step(6, 1, dp(z(2)), dp(z(2)), dp(z(2)), None, 1.0, 0.01, C.byref(opts), dp(z(2)), dp(z(1)), dp(z(2)),
                                ip(np.zeros(1, np.int32)), ip(np.zeros(1, np.int32))) == -1


def test_reference_particle_in_quadratic_bowl(gpu_required):
    """test/simulator/particle.jl:129-209: particle in quadratic_bowl_3D_lc, μ 0.1, h 0.01, T 1000, q1 (1, 0.5, 2); v1 (0.1, 0, 0)
    and the DROP (v1 = 0) side by side: it settles at the bottom."""
    from contactimplicitmpc.jl_amd import plant
    q1 = np.array([[1.0, 0.5, 2.0], [1.0, 0.5, 2.0]]); v1 = np.array([[0.1, 0.0, 0.0], [0.0, 0.0, 0.0]])
    ok, q, *_ = plant.simulate("particle", lambda qq: np.zeros((2, 3)), q1, v1, 1000, 0.01, mu=0.1, terrain="quadratic_bowl_3D_lc")
    assert ok
    assert np.all(np.abs(q[-1, :, 0]) < 0.05) and np.all(np.abs(q[-1, :, 1]) < 0.05) and np.all(np.abs(q[-1, :, 2]) < 1e-3)


def test_reference_particle_2d_on_slope(gpu_required):
    """test/simulator/particle.jl:246-268: particle_2D on slope1_2D_lc, μ 0.1, h 0.01, T 100, q1 (0, 1): it slides down the slope;
    and the first 100 steps agree with the CPU restatement."""
    from contactimplicitmpc.jl_amd import plant
    q1 = np.array([[0.0, 1.0]]); v1 = np.zeros((1, 2))
    ok, q, *_ = plant.simulate("particle_2D", lambda qq: np.zeros((1, 2)), q1, v1, 100, 0.01, mu=0.1, terrain="slope1_2D_lc")
    assert ok and q[-1, 0, 0] < 0.0 and q[-1, 0, 1] < 0.0
    okc, qc, *_ = pl.simulate(terrain_ref.plant("particle_2D", "slope1_2D_lc"), lambda qq, t: np.zeros(2), q1[0], v1[0], 100, 0.01, mu=0.1)
    assert okc
    np.testing.assert_allclose(q[:, 0], qc, rtol=0, atol=1e-7)


def test_closed_loop_on_sine_terrain_with_the_altitude_update(gpu_required, monkeypatch):
    """examples/quadruped/sine.jl with policy and plant on the device: gait2 and the flat controller (H_mpc 10, N_sample 5, κ_mpc 1e-4,
    altitude_update with threshold 0.05) while the plant steps on sine1_2D_lc; two robots, the second 1 cm higher with its joints
    0.02 rad off.  Every plant step converges; after every impact the policy's altitude for that contact is the terrain height
    under the foot; the robots walk forward and stay up (bounds from the first measured run)."""
    import torch
    from contactimplicitmpc.jl_amd import InteriorPointOptions, NewtonOptions, plant, terrain
    from contactimplicitmpc.jl_amd import policy as policy_mod
    KAPPA, H_MPC, N_SAMPLE, H_sim = 1e-4, 10, 5, 300
    T = terrain.get("sine1_2D_lc")
    d, P, prob, tabs = real_problem("quadruped", KAPPA, True)
    hits = []
    orig = policy_mod.update_altitude

    def recording_update(model, alt, gamma_hist, q_hist, threshold=1.0):
        out = orig(model, alt, gamma_hist, q_hist, threshold)
        for i in range(model.nc):
            j = int(np.argmax(gamma_hist[:, i]))                # first maximum, as the reference's strict `>` picks
            if gamma_hist[j, i] > threshold:
                foot_x = float(model.kinematics(torch.as_tensor(q_hist[j]))[2 * i])
                hits.append((float(alt[i]), float(T.surface(foot_x))))
        return out
    monkeypatch.setattr(policy_mod, "update_altitude", recording_update)
    obj = synth.make_objective(d, H_MPC, kind="quadruped")
    pol = policy_mod.CIMPCPolicy(P, obj.q, obj.u, H_mpc=H_MPC, N_sample=N_SAMPLE, kappa_mpc=KAPPA, B=2,
                                 n_opts=NewtonOptions(kappa=KAPPA, r_tol=3e-4, max_iter=5), ip_opts=InteriorPointOptions(kappa_tol=KAPPA, r_tol=1e-8),
                                 altitude_update=True, altitude_impact_threshold=0.05)
    q1 = np.stack([P.q[1], P.q[1]]); v1 = np.stack([(P.q[1] - P.q[0]) / P.h] * 2)
    q1[1, 1] += 0.01; q1[1, 3:] += 0.02
    q1[:, 1] += T.surface(q1[:, 0])
    ok, q, u, g, b = plant.simulate("quadruped", pol, q1, v1, H_sim, P.h / N_SAMPLE, mu=1.0, terrain=T)
    pol.close()
    assert ok
    # bounds from the first measured run (243 impacts, altitude error 1.4e-10, progress 0.181 / 0.169 m, clearance 0.275 m,
    # pitch 0.083 rad)
    assert len(hits) >= 200
    err = max(abs(a - s) for a, s in hits)
    progress = q[-1, :, 0] - q[1, :, 0]
    clearance = (q[:, :, 1] - T.surface(q[:, :, 0])).min()
    pitch = np.abs(q[:, :, 2] - P.q[0][2]).max()
    print("impacts %d, altitude error %.2e, progress %s, min clearance %.4f, max pitch %.4f" % (len(hits), err, progress, clearance, pitch))
    assert err <= 2e-3
    assert np.all(progress > 0.15)
    assert clearance > 0.25
    assert pitch < 0.15
