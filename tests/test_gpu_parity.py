"""-m gpu: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Tolerances (fp64): the kernels use the reference's algorithm (Schur complement + MGS-QR,
same association in rlin!), but reductions run in a different order (DPP trees), divisions
by the QR diagonal are multiplications by a reciprocal, and the triangular solve runs
column-oriented.  The Schur matrix reaches cond ~1e6..1e8 near convergence (y2/y1 on the
diagonal), so iterates agree to ~cond*eps:  converged z to 1e-6 absolute (values O(1)), d to 1e-7, sensitivities
to 1e-6 relative, identical iteration counts and status flags."""
import numpy as np
import pytest

from oracle import ip as oip
from oracle import newton as onewton, synth

from common import make_case, make_solver, oracle_sweep

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model,mode,B,H,H_ref", [
    ("quadruped", 0, 5, 6, 12),
    ("hopper", 0, 4, 8, 10),
    ("pushbot", 1, 3, 5, 8),
    ("quadruped", 1, 3, 4, 8),
    ("centroidal", 0, 3, 4, 6),
    ("flamingo", 1, 3, 5, 8),
    ("hopper3d", 0, 4, 6, 8),            # the reference's remaining models (src/dynamics/*/model.jl): dimension sets without
    ("walledcartpole", 1, 3, 5, 8),      # a single-launch kernel - lock-step rounds only
    ("particle", 0, 3, 5, 8),
    ("particle2d", 1, 3, 4, 6),
    ("anydims", 0, 3, 5, 8),             # no compiled set: the runtime-dimension kernel (ip_generic.hip)
    ("anydims", 1, 3, 5, 8),
    ("centroidal_wall", 0, 2, 4, 6),     # ny = 48 > 32 lanes: the compiled 64-lane sweep (round 6; rounds 2-5: runtime-dimension kernel)
    ("centroidal_wall", 1, 2, 4, 6),     # ... whose :configurationforce mode keeps the runtime-dimension kernel
])
def test_implicit_dynamics_matches_oracle(gpu_required, model, mode, B, H, H_ref):
    d, prob, tabs, rollouts = make_case(model, mode, H_ref=H_ref, H=H, B=B, seed=3)
    opts = oip.IPOptions(kappa_tol=prob["kappa"])
    s = make_solver(d, prob, rollouts, H)
    ref = oracle_sweep(d, tabs, rollouts, opts)
    q = np.stack([tr.q for tr, _ in ref]); th = np.stack([tr.theta for tr, _ in ref])
    g = np.stack([tr.gamma for tr, _ in ref]); bb = np.stack([tr.b for tr, _ in ref])
    out = s.implicit_dynamics(q, th, g, bb, want_z=True)
    n = agree = 0
    for b, (tr, o) in enumerate(ref):
        # a borderline solve may flip one discrete IP decision (iteration count) under roundoff:
        # r_tol = 1e-8 sits at the cond*eps noise floor of the Schur solve
        same = (out["status"][b] == o["status"]) & (out["iters"][b] == o["iters"])
        n += same.size
        agree += int(same.sum())
        ok = same & (o["status"] == 1)
        np.testing.assert_allclose(out["z"][b][ok], o["z"][ok], rtol=0, atol=1e-6)
        np.testing.assert_allclose(out["d"][b][ok], o["d"][ok], rtol=0, atol=1e-7)
        for k in ("dq0", "dq1", "du1"):
            scale = np.abs(o[k]).max()
            np.testing.assert_allclose(out[k][b][ok], o[k][ok], rtol=0, atol=1e-6 * max(scale, 1.0))
    assert agree >= 0.9 * n, (agree, n)


def _newton_case(perturb, r_tol, max_iter, seed, B=6, H=10, H_ref=16, model="quadruped", dense_q=False):
    d, prob, tabs, rollouts = make_case(model, 0, H_ref=H_ref, H=H, B=B, seed=seed, perturb=perturb)
    from contactimplicitmpc.jl_amd import NewtonOptions
    obj = synth.make_objective(d, H, kind=model, dense_q=dense_q)
    s = make_solver(d, prob, rollouts, H, obj=obj,
                    newton_opts=NewtonOptions(kappa=prob["kappa"], r_tol=r_tol, max_iter=max_iter))
    u1, it, rn = s.newton_solve(np.stack([r[2] for r in rollouts]), np.stack([r[3] for r in rollouts]))
    traj = s.trajectory()
    cnt = s.rollout_counters()
    res = []
    for b, (window, ref, q0, q1) in enumerate(rollouts):
        core = onewton.Newton(d, H, obj, onewton.NewtonOptions(r_tol=r_tol, max_iter=max_iter, solver="lu"),
                              oip.IPOptions(kappa_tol=prob["kappa"]), prob["kappa"], ref)
        st = onewton.newton_solve(core, q0, q1, window, tabs, ref)
        res.append((core, st))
    return u1, it, rn, traj, cnt, res


def test_newton_solve_matches_oracle(gpu_required):
    """newton_solve! against the oracle running the reference-default dense-LU KKT backend.
    Moderate perturbation: every rollout converges with mostly full steps."""
    u1, it, rn, traj, cnt, res = _newton_case(perturb=1e-2, r_tol=1e-5, max_iter=5, seed=11)
    for b, (core, st) in enumerate(res):
        assert it[b] == st.iters
        assert cnt["sweeps"][b] == st.sweeps
        assert cnt["ip_iters"][b] == st.ip_iters
        np.testing.assert_allclose(rn[b], st.r_norm / core.lay.N, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(traj["q"][b], core.traj.q, rtol=0, atol=1e-8)
        np.testing.assert_allclose(traj["u"][b], core.traj.u, rtol=0, atol=1e-8)
        np.testing.assert_allclose(traj["nu"][b], core.nu, rtol=0, atol=1e-8)
        np.testing.assert_allclose(u1[b], core.traj.u[0], rtol=0, atol=1e-8)


@pytest.mark.parametrize("model,H,H_ref,dense_q", [
    ("hopper", 20, 24, False),       # BASELINE configs[1]: hopper flat, H = 20
    ("centroidal", 6, 8, True),      # nq = 18 > 16: 24 x 24 KKT tiles, dense Q (relative_state_cost)
    ("hopper3d", 10, 12, False),     # (nq, nu) = (7, 3): hopper_3D
    ("walledcartpole", 8, 10, False),    # (4, 1)
    ("particle", 8, 10, True),       # (3, 3)
    ("anydims", 8, 10, False),       # runtime dimensions end to end: generic sweep + runtime residual kernel + banded LDL^T / dense LU
    ("centroidal_wall", 5, 6, True),
])
def test_newton_solve_other_models(gpu_required, model, H, H_ref, dense_q):
    u1, it, rn, traj, cnt, res = _newton_case(perturb=5e-3, r_tol=1e-5, max_iter=4, seed=23, B=4, H=H, H_ref=H_ref,
                                              model=model, dense_q=dense_q)
    # One rollout of the batch may leave the oracle's discrete path: a decision inside an interior-point solve
    # that flips under ~cond*eps roundoff moves the residual of the trial point by per cent, and a residual that close to r_tol then
    # ends the Newton loop one iteration earlier or later (hopper3d, rollout 1: 1.011e-5 against r_tol = 1e-5 after the first
    # iteration; the sensitivities themselves agree to 1e-9, scripts/dbg/sens_err.py).  Such a rollout must still end converged.
    same = 0
    for b, (core, st) in enumerate(res):
        if it[b] == st.iters and cnt["ip_iters"][b] == st.ip_iters and cnt["sweeps"][b] == st.sweeps:
            same += 1
            np.testing.assert_allclose(traj["q"][b], core.traj.q, rtol=0, atol=1e-7)
            np.testing.assert_allclose(traj["u"][b], core.traj.u, rtol=0, atol=1e-6)
        else:
            # (the relaxed branch is bounded - it is the round-off flip described above and nothing else: one iteration
            #  apart, the shorter run ended within 5 % of r_tol (the coin toss), both ends converged, and the two final iterates are
            #  the same trajectory at the level one extra Newton step moves it; a real regression on a rollout fails one of these)
            assert abs(int(it[b]) - st.iters) <= 1
            assert rn[b] < 1e-5 or it[b] == 4
            r_short = rn[b] if it[b] < st.iters else st.r_norm / core.lay.N
            assert it[b] == st.iters or 0.95e-5 < r_short < 1e-5, (b, it[b], st.iters, r_short)
            np.testing.assert_allclose(traj["q"][b], core.traj.q, rtol=0, atol=1e-5)
            np.testing.assert_allclose(traj["u"][b], core.traj.u, rtol=0, atol=1e-5 * max(1.0, np.abs(core.traj.u).max()))
    assert same >= len(res) - 1


def test_newton_solve_backtracking_regime(gpu_required):
    """Large perturbation: heavy backtracking, residual at the IP-termination noise floor.
    Every discrete decision inside an IP solve (iteration count, regularisation switch,
    line-search back-off) can flip under ~cond*eps roundoff at such candidates, after which a
    rollout legitimately follows a different path.  Required: identical Newton iteration
    counts everywhere, and at least half of the rollouts on the oracle's path to 1e-7."""
    u1, it, rn, traj, cnt, res = _newton_case(perturb=3e-2, r_tol=1e-6, max_iter=4, seed=11)
    same = 0
    for b, (core, st) in enumerate(res):
        assert it[b] == st.iters
        if np.abs(traj["q"][b] - core.traj.q).max() < 1e-7 and np.abs(traj["u"][b] - core.traj.u).max() < 1e-7:
            same += 1
    assert same >= len(res) // 2


def test_implicit_dynamics_stress(gpu_required):
    """Hard interior-point instances (large parameter perturbations): exercises the
    regularisation switch, the residual line search and failing solves.  Flags and
    iteration counts must agree on >= 95 % of the solves, and those agree to 1e-6."""
    from oracle.newton import Traj
    B, H, H_ref = 16, 8, 10
    d, prob, tabs, rollouts = make_case("quadruped", 0, H_ref=H_ref, H=H, B=B, seed=21, perturb=0.15)
    rng = np.random.default_rng(5)
    hard = []
    for (window, ref, q0, q1) in rollouts:          # perturb the whole trajectory, not only (q0, q1)
        tr = ref.copy()
        tr.q += rng.uniform(-0.05, 0.05, tr.q.shape)
        tr.u += rng.uniform(-0.5, 0.5, tr.u.shape)
        tr.update_theta(d)
        hard.append((window, tr, tr.q[0].copy(), tr.q[1].copy()))
    opts = oip.IPOptions(kappa_tol=prob["kappa"])
    s = make_solver(d, prob, hard, H)
    ref = oracle_sweep(d, tabs, hard, opts)
    q = np.stack([tr.q for tr, _ in ref]); th = np.stack([tr.theta for tr, _ in ref])
    out = s.implicit_dynamics(q, th, want_z=True)
    n = agree = 0
    for b, (tr, o) in enumerate(ref):
        for i in range(H):
            n += 1
            if out["status"][b, i] == o["status"][i] and out["iters"][b, i] == o["iters"][i]:
                agree += 1
                if o["status"][i]:
                    np.testing.assert_allclose(out["z"][b, i], o["z"][i], rtol=0, atol=1e-6)
                    np.testing.assert_allclose(out["d"][b, i], o["d"][i], rtol=0, atol=1e-6)
    assert agree >= 0.95 * n, (agree, n)
    its = np.concatenate([o["iters"] for _, o in ref])
    assert its.max() >= 9          # the instances really are harder than the nominal 5-6 iterations


@pytest.mark.parametrize("model,H,H_ref", [
    ("quadruped", 8, 10),           # 16 x 16 MFMA tiles
    ("centroidal", 8, 10),          # nq = 18: 24 x 24 tiles (2 x 2 masked MFMA blocks), readlane Cholesky
    ("centroidal", 60, 71),         # BASELINE configs[4] horizon: the backward pass's staging at H = 60
])
def test_kkt_solve_matches_dense_lu(gpu_required, model, H, H_ref):
    """B1 seam: the condensed device solve against numpy's dense LU of the assembled R
    (the reference default :lu_solver)."""
    B = 4 if H <= 8 else 2
    d, prob, tabs, rollouts = make_case(model, 0, H_ref=H_ref, H=H, B=B, seed=5)
    obj = synth.make_objective(d, H, dense_q=True)
    s = make_solver(d, prob, rollouts, H, obj=obj)
    q = np.stack([r.q for (_, r, _, _) in rollouts]); th = np.stack([r.theta for (_, r, _, _) in rollouts])
    out = s.implicit_dynamics(q, th)    # leaves the sensitivities resident on the device
    assert out["status"].all()
    lay = onewton.Layout(d, H)
    rng = np.random.default_rng(0)
    r = rng.standard_normal((B, lay.N))
    for beta in (1e-5, 10.0):
        delta = s.kkt_solve(r, beta)
        for b in range(B):
            # R from the DEVICE's own sensitivities: isolates the linear solve from the interior-point parity
            im = {k: out[k][b] for k in ("d", "dq0", "dq1", "du1")}
            R = onewton.jacobian(lay, obj, im, beta, prob["kappa"])
            x = np.linalg.solve(R, r[b])
            np.testing.assert_allclose(delta[b], x, rtol=0, atol=1e-7 * max(1.0, np.abs(x).max()))


@pytest.mark.parametrize("model,mode,velocity,backend", [
    ("quadruped", 0, False, 1),     # :configuration through the reference-default backend
    ("pushbot", 1, False, 1),       # BASELINE configs[0] dimensions, :configurationforce (policy.jl:46 default), dense LU
    ("hopper", 1, True, 1),         # :configurationforce + TrackingVelocityObjective, dense LU
    ("pushbot", 1, False, 0),       # ... and as the library solves them by default: gamma / b eliminated (weights 1e-100),
    ("hopper", 1, True, 0),         #     the rest through the condensed MFMA solve / the banded LDL^T
    ("quadruped", 1, False, 0),
    ("hopper", 0, True, 1),         # velocity objective in :configuration mode (v_target terms), dense LU on request
    ("hopper", 0, True, 0),         # ... and through the backend the library picks for it: banded LDL^T
    ("quadruped", 0, True, 0),      # banded LDL^T, w = 81
    ("quadruped", 0, False, 2),     # banded LDL^T on request for a TrackingObjective
    ("centroidal", 0, True, 0),     # banded LDL^T, w = 131 (139 KB window in LDS)
])
def test_kkt_dense_lu_backend(gpu_required, model, mode, velocity, backend):
    """B1 seam through kkt_dense.hip: dense jacobian! + LU with partial pivoting (the reference default
    :lu_solver) against numpy's solve of the oracle's jacobian!, for the modes / objectives the condensed
    solve does not cover."""
    from contactimplicitmpc.jl_amd import NewtonOptions
    H, H_ref, B = 6, 8, 3
    d, prob, tabs, rollouts = make_case(model, mode, H_ref=H_ref, H=H, B=B, seed=9)
    obj = synth.make_objective(d, H, kind=model, velocity=velocity)
    if velocity:
        obj.v = obj.v * 1e3                      # make the velocity blocks numerically visible
        obj.v_target = 0.01 * np.random.default_rng(3).standard_normal((H, d.nq))
        obj.q_target = None
        obj.__post_init__()
    s = make_solver(d, prob, rollouts, H, obj=obj, newton_opts=NewtonOptions(kappa=prob["kappa"], kkt_backend=backend))
    opts = oip.IPOptions(kappa_tol=prob["kappa"])
    ref = oracle_sweep(d, tabs, rollouts, opts)
    q = np.stack([tr.q for tr, _ in ref]); th = np.stack([tr.theta for tr, _ in ref])
    g = np.stack([tr.gamma for tr, _ in ref]); bb = np.stack([tr.b for tr, _ in ref])
    out = s.implicit_dynamics(q, th, g, bb)       # leaves the sensitivities resident on the device
    lay = onewton.Layout(d, H)
    r = np.random.default_rng(0).standard_normal((B, lay.N))
    for beta in (1e-5, 10.0):
        delta = s.kkt_solve(r, beta)
        for b in range(B):
            # R from the DEVICE's own sensitivities: isolates the assembly + LU from the interior-point parity
            im = {k: out[k][b] for k in ("d", "dq0", "dq1", "du1")}
            R = onewton.jacobian(lay, obj, im, beta, prob["kappa"])
            x = np.linalg.solve(R, r[b])
            back = np.abs(R @ delta[b] - r[b]).max() / (np.abs(R).sum(axis=1).max() * np.abs(delta[b]).max() + np.abs(r[b]).max())
            # dense LU with partial pivoting: backward stable; the banded LDL^T runs WITHOUT pivoting (quasi-definite
            # matrix, interleaved order): its backward error carries the growth of L (1e2 .. 1e4 here) - both far
            # inside the 1e-10 residual lu.jl's own test asks for
            banded = mode == 0 and backend != 1 and (velocity or backend == 2)
            reduced = mode == 1 and backend != 1        # cf mode eliminated onto the :configuration solvers
            tol = 1e-9 if reduced else 1e-11 if banded else 1e-13
            assert back < tol, back
            atol = tol * np.linalg.cond(R) * max(1.0, np.abs(x).max())
            if reduced:     # condensed MFMA solve behind the reduction: its own bar (test_kkt_solve_matches_dense_lu)
                atol = 1e-7 * max(1.0, np.abs(x).max())
            np.testing.assert_allclose(delta[b], x, rtol=0, atol=atol)


def test_cf_mode_with_real_contact_weights_keeps_the_dense_lu(gpu_required):
    """The elimination of (gamma, b) is only taken for weights below fp64 resolution; a :configurationforce problem that
    really penalises contact impulses goes through the dense LU and still matches numpy."""
    from contactimplicitmpc.jl_amd import NewtonOptions
    H, H_ref, B = 5, 7, 2
    d, prob, tabs, rollouts = make_case("pushbot", 1, H_ref=H_ref, H=H, B=B, seed=4)
    obj = synth.make_objective(d, H, kind="pushbot")
    obj.gamma = np.tile((3e-2 * np.eye(d.nc))[None], (H, 1, 1))
    obj.b = np.tile((2e-2 * np.eye(d.nb))[None], (H, 1, 1))
    s = make_solver(d, prob, rollouts, H, obj=obj, newton_opts=NewtonOptions(kappa=prob["kappa"]))
    ref = oracle_sweep(d, tabs, rollouts, oip.IPOptions(kappa_tol=prob["kappa"]))
    q = np.stack([tr.q for tr, _ in ref]); th = np.stack([tr.theta for tr, _ in ref])
    g = np.stack([tr.gamma for tr, _ in ref]); bb = np.stack([tr.b for tr, _ in ref])
    out = s.implicit_dynamics(q, th, g, bb)
    lay = onewton.Layout(d, H)
    r = np.random.default_rng(0).standard_normal((B, lay.N))
    delta = s.kkt_solve(r, 1e-3)
    for b in range(B):
        im = {k: out[k][b] for k in ("d", "dq0", "dq1", "du1")}
        R = onewton.jacobian(lay, obj, im, 1e-3, prob["kappa"])
        x = np.linalg.solve(R, r[b])
        np.testing.assert_allclose(delta[b], x, rtol=0, atol=1e-12 * np.linalg.cond(R) * max(1.0, np.abs(x).max()))


@pytest.mark.parametrize("model,mode,velocity", [("hopper", 1, False), ("quadruped", 1, False), ("hopper", 0, True)])
def test_newton_solve_configurationforce_and_velocity(gpu_required, model, mode, velocity):
    """newton_solve! in :configurationforce mode / with a TrackingVelocityObjective (dense LU KKT) against
    the oracle running the reference-default dense-LU backend."""
    from contactimplicitmpc.jl_amd import NewtonOptions
    H, H_ref, B = 8, 12, 4
    d, prob, tabs, rollouts = make_case(model, mode, H_ref=H_ref, H=H, B=B, seed=31, perturb=5e-3)
    obj = synth.make_objective(d, H, kind=model, velocity=velocity)
    if velocity:
        obj.v = obj.v * 1e3
    s = make_solver(d, prob, rollouts, H, obj=obj, newton_opts=NewtonOptions(kappa=prob["kappa"], r_tol=1e-5, max_iter=4))
    u1, it, rn = s.newton_solve(np.stack([r[2] for r in rollouts]), np.stack([r[3] for r in rollouts]))
    traj = s.trajectory(); cnt = s.rollout_counters()
    same = 0
    for b, (window, ref, q0, q1) in enumerate(rollouts):
        core = onewton.Newton(d, H, obj, onewton.NewtonOptions(r_tol=1e-5, max_iter=4, solver="lu"),
                              oip.IPOptions(kappa_tol=prob["kappa"]), prob["kappa"], ref)
        st = onewton.newton_solve(core, q0, q1, window, tabs, ref)
        if it[b] == st.iters and cnt["sweeps"][b] == st.sweeps and cnt["ip_iters"][b] == st.ip_iters:
            # equal TOTALS do not exclude two interior-point solves flipping one iteration in opposite directions (DESIGN.md section 2,
            # round 4): such a rollout agrees like an off-path one (1e-4) and does not count as "same"
            if np.abs(traj["q"][b] - core.traj.q).max() > 1e-7 or np.abs(traj["u"][b] - core.traj.u).max() > 1e-7:
                np.testing.assert_allclose(traj["q"][b], core.traj.q, rtol=0, atol=1e-4)
                continue
            same += 1       # same discrete path (see DESIGN.md section 2 on roundoff-level flips)
            # (|r|_1 / N of a converged solve: it moves by |dr/dx| |dx| with the |dx| <= 1e-7 asserted above - 3e-9 was seen on a 7e-7 norm
            #  when the sweep's dot products went from four partial sums to the reference loop's running sum)
            np.testing.assert_allclose(rn[b], st.r_norm / core.lay.N, rtol=1e-3, atol=1e-8)
    assert same >= B - 1


@pytest.mark.parametrize("mode,B,tail", [("1", 24, None), ("2", 160, "120")])
def test_async_single_launch_matches_lockstep(gpu_required, monkeypatch, mode, B, tail):
    """The single-launch asynchronous solve (CIMPC_ASYNC=1, newton_async_impl.h) and the hybrid schedule
    (auto mode: lock-step rounds, then the asynchronous kernel for the last `tail` active rollouts, solves
    parked by the rounds included) run the same per-rollout arithmetic as the lock-step rounds alone:
    identical iteration counts, counters and trajectories."""
    from contactimplicitmpc.jl_amd import NewtonOptions
    d, prob, tabs, rollouts = make_case("quadruped", 0, H_ref=16, H=10, B=B, seed=5, perturb=3e-2)
    obj = synth.make_objective(d, 10, kind="quadruped")
    q0 = np.stack([r[2] for r in rollouts]); q1 = np.stack([r[3] for r in rollouts])
    if tail is not None:
        monkeypatch.setenv("CIMPC_ASYNC_TAIL", tail)
    # (same arithmetic on both sides: the lock-step rounds of a small batch would take the twisted KKT solve of round 5, the
    #  asynchronous kernel's KKT job is the one-ended pipeline - tests/test_gpu_round5.py compares the two solves)
    monkeypatch.setenv("CIMPC_KKT_TWISTED", "0")
    outs = []
    for flag in ("0", mode):
        monkeypatch.setenv("CIMPC_ASYNC", flag)
        s = make_solver(d, prob, rollouts, 10, obj=obj,
                        newton_opts=NewtonOptions(kappa=prob["kappa"], r_tol=1e-5, max_iter=5))
        u1, it, rn = s.newton_solve(q0, q1)
        outs.append((u1, it, rn, s.trajectory(), s.rollout_counters(), s.stats()))
    a, b = outs
    assert b[5]["rounds"] < a[5]["rounds"]          # the second solver really left the lock-step rounds
    if mode == "1":
        assert b[5]["rounds"] == 1
    else:
        assert b[5]["rounds"] > 2                    # ... after running some of them (hybrid)
    np.testing.assert_array_equal(a[1], b[1])
    for k in ("sweeps", "ip_iters", "ip_failures"):
        np.testing.assert_array_equal(a[4][k], b[4][k])
    # (the 1-norm reductions run with different workgroup sizes: last-bit differences only)
    np.testing.assert_allclose(a[0], b[0], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-12, atol=0)
    for k in ("q", "u", "nu"):
        np.testing.assert_allclose(a[3][k], b[3][k], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("model", ["pushbot", "hopper", "flamingo", "centroidal"])
def test_async_single_launch_other_models(gpu_required, monkeypatch, model):
    """Every other row of model_table.h with a single-launch instantiation reaches ITS persistent kernel (one round), and that kernel
    runs the arithmetic of the lock-step rounds: the case of test_newton_solve_other_models, compared as the quadruped is above."""
    from contactimplicitmpc.jl_amd import NewtonOptions
    B, H, H_ref = 4, 6, 8
    d, prob, tabs, rollouts = make_case(model, 0, H_ref=H_ref, H=H, B=B, seed=23, perturb=5e-3)
    obj = synth.make_objective(d, H, kind=model, dense_q=model == "centroidal")
    q0 = np.stack([r[2] for r in rollouts]); q1 = np.stack([r[3] for r in rollouts])
    monkeypatch.setenv("CIMPC_KKT_TWISTED", "0")
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("CIMPC_ASYNC", flag)
        s = make_solver(d, prob, rollouts, H, obj=obj, newton_opts=NewtonOptions(kappa=prob["kappa"], r_tol=1e-5, max_iter=4))
        u1, it, rn = s.newton_solve(q0, q1)
        outs.append((u1, it, s.trajectory(), s.rollout_counters(), s.stats()))
    a, b = outs
    assert b[4]["rounds"] == 1
    np.testing.assert_array_equal(a[1], b[1])
    for k in ("sweeps", "ip_iters", "ip_failures"):
        np.testing.assert_array_equal(a[3][k], b[3][k])
    np.testing.assert_allclose(a[0], b[0], rtol=1e-12, atol=1e-14)
    for k in ("q", "u", "nu"):
        np.testing.assert_allclose(a[2][k], b[2][k], rtol=1e-12, atol=1e-14)


def test_full_size_schedules_agree(gpu_required, monkeypatch):
    """BASELINE.json's full-size workload (quadruped, H = 40, H_ref = 60, 512 rollouts, cold start): the hybrid
    schedule (rounds + asynchronous tail, packed KKT) and the plain lock-step rounds must produce the same
    iteration counts, reference-equivalent counters and trajectories - a size-independent property that needs
    no oracle run (the oracle takes minutes at this size)."""
    import bench
    from contactimplicitmpc.jl_amd import CIMPCSolver, InteriorPointOptions, NewtonOptions
    H, H_ref, B = 40, 60, 512
    d, prob, obj, ro = bench.build_inputs(B, H, H_ref, seed=1234, perturb=0.05)
    q0 = np.stack([r[2] for r in ro]); q1 = np.stack([r[3] for r in ro])
    outs = []
    # (round 6: the rounds' KKT stage may take the duo kernel - the two-ended elimination, equal to the one-ended kernels to 1e-12 but not
    #  to the bit - in rounds the asynchronous tail replaces with its own one-ended KKT job.  The property tested here is that the
    #  SCHEDULE does not change the iterates: both runs use the one-ended kernels; test_gpu_round6.py compares the kernels.)
    monkeypatch.setenv("CIMPC_KKT_DUO", "0")
    for flag in ("0", "2"):
        monkeypatch.setenv("CIMPC_ASYNC", flag)
        s = CIMPCSolver(d.nq, d.nu, d.nw, d.nc, d.nb, H_ref, H, B=B, mode=0, ip_opts=InteriorPointOptions(kappa_tol=prob["kappa"]),
                        newton_opts=NewtonOptions(kappa=prob["kappa"], r_tol=3e-4, max_iter=5))
        for t in range(H_ref):
            s.set_linearization(t + 1, prob["z0"][t], prob["th0"][t], prob["r0"][t], prob["rz0"][t], prob["rth0"][t])
        s.set_objective(obj.q, obj.u)
        s.set_window(np.stack([w for (w, _, _, _) in ro]) + 1)
        s.set_reference(np.stack([r.q for (_, r, _, _) in ro]), np.stack([r.u for (_, r, _, _) in ro]), np.stack([r.w for (_, r, _, _) in ro]),
                        np.stack([r.gamma for (_, r, _, _) in ro]), np.stack([r.b for (_, r, _, _) in ro]), np.stack([r.theta for (_, r, _, _) in ro]))
        u1, it, rn = s.newton_solve(q0, q1)
        outs.append((u1, it, rn, s.trajectory(), s.rollout_counters(), s.stats()))
        s.close()
    a, b = outs
    assert b[5]["rounds"] < a[5]["rounds"]               # the hybrid run handed its tail over
    np.testing.assert_array_equal(a[1], b[1])
    for k in ("sweeps", "ip_iters", "ip_failures"):
        np.testing.assert_array_equal(a[4][k], b[4][k])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    for k in ("q", "u", "nu"):
        np.testing.assert_array_equal(a[3][k], b[3][k])
    assert np.isfinite(a[3]["q"]).all() and (a[1] <= 5).all()
