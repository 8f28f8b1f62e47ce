"""Closed-loop device rollouts under linear state feedback (`plant.rollout(..., feedback=)`, `rollout_tape`, `RolloutTape.vjp`,
`rollout_torch`; csrc/plant_feedback.h in plant_step_kernel and plant_adjoint_kernel) against the restatements of
tests/plant_feedback_cases.py, on the seven cases there (every step instance of csrc/plant_ground.h), each with a shared schedule at
n_sample = 1 and a per-robot one at n_sample = 4 (hopper_2D also with K_f = 2 rows held for 2 steps), steps_per_launch = 2:

    the law, the replay of u_applied through the open-loop rollout, K = 0, the host loop, the step gradients and the reverse chain
    are held bit for bit (`array_equal`); the chain is also held within 100 x max(d(chain_np, chain_ld), 2.2e-16) of the longdouble
    restatement, the bound of tests/plant_adjoint_cases.py built from the restatements alone; the adjoint identity within what those
    bounds allow an inner product; finite differences in flight within 1e-4, the tolerance of
    test_chain_matches_finite_differences_of_the_device_rollout_in_flight (tests/test_gpu_plant_adjoint.py).

Measured on one MI355X: every bit-for-bit comparison holds on every case and variant; the chain is at most 1.6e-14 from chain_ld
(particle, g_mu; bounds from 2.2e-14 to 7.8e-13).  Adjoint identity: hopper_2D 2.2e-13 of 49.4 (allowed 1.6e-9), quadruped 1.9e-13 of 194
(7.8e-10).  Flight finite differences of the closed-loop device rollout: d/dK 1.6e-6 (robot 0) and 5.3e-6 (robot 2), d/dx_ref 3.7e-6 and
4.3e-6.  Timings: scripts/plant_feedback_ab.py, profiles/plant_feedback.json.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import plant_adjoint_cases as pac
import plant_feedback_cases as pfc
import plant_gradient_cases as pgc

pytestmark = pytest.mark.gpu

PAIRS = [(w, v) for w in pfc.CASES for v in pfc.variants(w)]
IDS = [f"{w}-{v}" for w, v in PAIRS]
PLAIN = ("q", "gamma", "b", "status", "iters")


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def _fb(which, variant, **over):
    from contactimplicitmpc.jl_amd import plant
    f = dict(pfc.feedback(which, variant))
    f.update(over)
    return plant.Feedback(f["K"], f["x_ref"], hold=f["hold"], n_sample=f["n_sample"])


def _ubar(c):
    """The open-loop controls per step and robot, (T, B, nu): N_sample = 1."""
    return np.broadcast_to(c["u"], (c["T"], c["q1"].shape[0], c["u"].shape[2]))


@functools.lru_cache(maxsize=None)
def _closed(which, variant):
    """The closed-loop rollout of a case with every column of θ differentiated, once per process:
    dict(ok, q, u_applied, gamma, b, status, iters, G, fb_err)."""
    from contactimplicitmpc.jl_amd import plant
    c = pfc.base_case(which)
    out = plant.rollout(*_args(c), terrain=c["terrain"], steps_per_launch=pfc.STEPS_PER_LAUNCH, diff_sol=True,
                        grad_cols=pgc.dims(c["model"])[6], feedback=_fb(which, variant))
    assert len(out) == 9
    for a in out[1:7] + (out[8],):
        a.setflags(write=False)
    return dict(zip(("ok", "q", "u_applied", "gamma", "b", "status", "iters", "G", "fb_err"), out))


def _tape(which, variant, **kw):
    from contactimplicitmpc.jl_amd import plant
    c = pfc.base_case(which)
    kw.setdefault("grad_cols", pgc.dims(c["model"])[6])
    kw.setdefault("feedback", _fb(which, variant))
    *plain, tape, fb_err = plant.rollout_tape(*_args(c), terrain=c["terrain"], steps_per_launch=pfc.STEPS_PER_LAUNCH, **kw)
    return plain, tape, fb_err


# ---- 1. the law ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,variant", PAIRS, ids=IDS)
def test_applied_controls_and_errors_are_the_law_on_the_returned_trajectory(which, variant):
    c, r = pfc.base_case(which), _closed(which, variant)
    assert r["ok"] and r["status"].all(), "every step of every case converges"
    u, e = pfc.law_on(r["q"], _ubar(c), pfc.feedback(which, variant))
    np.testing.assert_array_equal(r["u_applied"], u)
    np.testing.assert_array_equal(r["fb_err"], e)
    assert np.abs(r["u_applied"] - _ubar(c)).max() > 1e-4      # the loop is closed


# ---- 2. the closed-loop step is the open-loop step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,variant", PAIRS, ids=IDS)
def test_replaying_the_applied_controls_open_loop_returns_the_same_rollout(which, variant):
    """u_applied as a per-robot schedule with K_u = T, N_sample = 1, in chunks of 2 steps and in one launch."""
    from contactimplicitmpc.jl_amd import plant
    c, r = pfc.base_case(which), _closed(which, variant)
    for spl in (pfc.STEPS_PER_LAUNCH, 0):
        ok, q, ua, g, b, st, it = plant.rollout(c["model"], c["q1"], c["v1"], r["u_applied"], c["h"], c["mu"], N_sample=1, terrain=c["terrain"],
                                                steps_per_launch=spl)
        for name, a in zip(PLAIN, (q, g, b, st, it)):
            np.testing.assert_array_equal(a, r[name], err_msg=f"{name}, steps_per_launch {spl}")
        np.testing.assert_array_equal(ua, r["u_applied"])


# ---- 3. zero gains ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pfc.CASES)
def test_zero_gains_return_the_open_loop_rollout(which):
    from contactimplicitmpc.jl_amd import plant
    c = pfc.base_case(which)
    f = pfc.feedback(which, "per_robot")
    plain = plant.rollout(*_args(c), terrain=c["terrain"], steps_per_launch=pfc.STEPS_PER_LAUNCH)
    got = plant.rollout(*_args(c), terrain=c["terrain"], steps_per_launch=pfc.STEPS_PER_LAUNCH, feedback=_fb(which, "per_robot", K=np.zeros(f["K"].shape)))
    assert len(got) == 8 and got[0] == plain[0]
    for name, a, w in zip(PLAIN, (got[1],) + got[3:7], (plain[1],) + plain[3:7]):
        np.testing.assert_array_equal(a, w, err_msg=name)
    np.testing.assert_array_equal(got[2], _ubar(c))
    assert np.abs(got[7]).max() > 0      # the errors are still reported


# ---- 4. the host loop it replaces --------------------------------------------------------------------------------------------------------------
def test_host_loop_with_the_law_in_numpy_gives_the_same_trajectory():
    """`simulate` with a Python policy that applies the law: every step is the same `plant_step`, so q is equal bit for bit."""
    from contactimplicitmpc.jl_amd import plant
    which, variant = "pushbot", "per_robot"
    c, r, f = pfc.base_case(which), _closed(which, variant), pfc.feedback(which, variant)
    Ks, xs = pfc.per_step(f, c["T"], 2)

    class Policy:
        def __init__(self):
            self.t, self.prev = 0, c["q1"] - c["h"] * c["v1"]

        def __call__(self, q1):
            u = np.stack([pfc.law(Ks[self.t, b], xs[self.t, b], self.prev[b], q1[b], c["u"][self.t, b], f["n_sample"])[0] for b in range(2)])
            self.t, self.prev = self.t + 1, q1.copy()
            return u

    ok, q, u, g, b = plant.simulate(which, Policy(), c["q1"], c["v1"], c["T"], c["h"], float(c["mu"][0]))
    assert ok
    np.testing.assert_array_equal(q, r["q"])
    np.testing.assert_array_equal(u, r["u_applied"])
    np.testing.assert_array_equal(g, r["gamma"])


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,variant", [(w, "per_robot") for w in pfc.CASES], ids=pfc.CASES)
def test_step_gradients_are_the_sensitivity_at_the_applied_controls(which, variant):
    """`rollout(diff_sol=True, feedback=)`' dz blocks against `plant.sensitivity` on (z, θ) with θ's controls from u_applied."""
    from contactimplicitmpc.jl_amd import plant
    c, r = pfc.base_case(which), _closed(which, variant)
    G = r["G"]
    T, B = G.status.shape
    nth = pgc.dims(c["model"])[6]
    th = np.array([[pgc.step_theta(c, r["q"], r["u_applied"], t, b) for b in range(B)] for t in range(T)])
    for b in range(B):      # one call per robot: a terrain is shared by the knots of a call
        dz, st = plant.sensitivity(c["model"], G.z[:, b], th[:, b], pgc.REG, nth, terrain=c["terrain"])
        np.testing.assert_array_equal(G.dz[:, b], dz)
        np.testing.assert_array_equal(G.status[:, b], st)
    assert G.status.all()


def _raw(cot):
    return dict(g_q0=cot.g_q0, g_q1=cot.g_q1, u_step=cot.u_step, w_step=cot.w_step, g_mu=cot.g_mu, g_h=cot.g_h, xref_step=cot.xref_step)


def _chain_parity(which, variant, seed=0):
    """The device chain of a closed-loop tape against the extended restatements on the device's own blocks."""
    c, r, f = pfc.base_case(which), _closed(which, variant), pfc.feedback(which, variant)
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
    G = r["G"]
    T, B = G.status.shape
    plain, tape, fb_err = _tape(which, variant)
    with tape:
        for name, a in zip(("ok",) + PLAIN[:1] + ("u_applied",) + PLAIN[1:], plain):
            np.testing.assert_array_equal(a, r[name], err_msg=name)
        np.testing.assert_array_equal(fb_err, r["fb_err"])
        np.testing.assert_array_equal(tape.grad_status, G.status)
        gq, gg, gb = pac.random_cotangents(np.random.default_rng(seed), T, B, nq, nc, nb)
        cot = tape.vjp(gq, gg, gb)
    Ks, _ = pfc.per_step(f, T, B)
    ld, f64, bound = pfc.bounds(G.dz, gq, gg, gb, nq, nu, nw, Ks, f["n_sample"])
    figures = {}
    for k, dev in _raw(cot).items():
        figures[k] = pac.distance(dev, ld[k])
        print(f"{which} {variant} {k}: device {figures[k]:.2e} from chain_ld (bound {bound[k]:.2e}), bits equal chain_f64: "
              f"{dev.tobytes() == np.ascontiguousarray(f64[k]).tobytes()}")
    for k, dev in _raw(cot).items():
        assert dev.tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{which} {variant} {k} differs from chain_f64"
        assert figures[k] <= bound[k], f"{which} {variant} {k}: {figures[k]:.3e} > {bound[k]:.3e}"
    return c, r, f, cot, (gq, gg, gb), (ld, bound), Ks


@pytest.mark.parametrize("which,variant", PAIRS, ids=IDS)
def test_closed_loop_chain_matches_the_extended_restatements(which, variant):
    c, r, f, cot, _, _, _ = _chain_parity(which, variant)
    shared = np.ndim(f["K"]) == 3
    K_f = f["K"].shape[0]
    assert cot.K.shape == f["K"].shape and cot.x_ref.shape == f["x_ref"].shape
    np.testing.assert_array_equal(cot.K, pfc.fold_gains(cot.u_step, r["fb_err"], K_f, f["hold"], shared, 1))
    np.testing.assert_array_equal(cot.x_ref, pfc.fold_rows(cot.xref_step, K_f, f["hold"], shared))
    assert np.abs(cot.K).max() > 0 and np.abs(cot.x_ref).max() > 0 and cot.n_cut.tolist() == [0] * c["q1"].shape[0]


# ---- 6. the adjoint identity on the device's own blocks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hopper_2D", "quadruped"])
def test_cotangents_are_adjoint_to_the_closed_loop_forward_tangents(which):
    """⟨cotangents, forward_tangent(δ) over StepGradients.dz⟩ = ⟨RolloutCotangents, δ⟩ for a random δ in (q1, v1, ū, K, x_ref, μ), held to
    what the per-output bounds allow an inner product: Σ_k bound_k max|chain_ld_k| ‖δ_k‖₁, where K's direction meets u_step through
    δK_t e_t (its gradient is Σ gu_t ⊗ e_t) and x_ref's meets xref_step."""
    variant = "per_robot"
    c, r, f, cot, (gq, gg, gb), (ld, bound), Ks = _chain_parity(which, variant, seed=4)
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
    T, B = r["status"].shape
    rng = np.random.default_rng(3)
    dq1, dv1, du, dmu = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal((T, B, nu)), rng.standard_normal(B)
    dK, dx = rng.standard_normal(f["K"].shape), rng.standard_normal(f["x_ref"].shape)
    dq0 = dq1 - c["h"] * dv1
    L = pac.LD
    dK_step, dx_step = pfc.per_step(dict(f, K=dK, x_ref=dx), T, B)
    dq, dgb = pfc.forward_tangent(r["G"].dz, dq0, dq1, du, nq, nu, nw, Ks, r["fb_err"], f["n_sample"], dK=dK_step, dxref=dx_step, dmu=dmu)
    lhs = (np.asarray(gq, L) * dq).sum() + (np.concatenate([gg, gb], axis=2).astype(L) * dgb).sum()
    rhs = sum((np.asarray(a, L) * d).sum() for a, d in ((cot.q1, dq1), (cot.v1, dv1), (cot.u, du), (cot.mu, dmu), (cot.K, dK), (cot.x_ref, dx)))
    dKe = np.einsum("tbij,tbj->tbi", dK_step, r["fb_err"])
    tol = sum(bound[k] * float(np.abs(ld[k]).max()) * float(np.abs(d).sum())
              for k, d in (("g_q0", dq0), ("g_q1", dq1), ("u_step", du), ("u_step", dKe), ("g_mu", dmu), ("xref_step", dx_step)))
    print(f"{which}: <g, J d> = {float(lhs):.12e}, <J' g, d> = {float(rhs):.12e}, difference {float(abs(lhs - rhs)):.2e} (allowed {tol:.2e})")
    assert float(abs(lhs - rhs)) <= tol


# ---- 7. finite differences of the closed-loop device rollout, in flight ------------------------------------------------------------------------
def test_gain_and_reference_gradients_match_finite_differences_in_flight():
    """hopper_2D steps 0-3 (before the impact, where the step is smooth), robots 0 and 2, ε = 1e-5, central differences of the
    closed-loop `plant.rollout`, a loss linear in (q, γ, b), a random direction in K and in x_ref: ∂loss/∂K and ∂loss/∂x_ref from `vjp`
    are each held to a relative difference of 1e-4 - the tolerance of
    test_chain_matches_finite_differences_of_the_device_rollout_in_flight (tests/test_gpu_plant_adjoint.py), taken over unchanged."""
    from contactimplicitmpc.jl_amd import plant
    T, eps = 4, 1e-5
    base, f = pfc.base_case("hopper_2D"), pfc.feedback("hopper_2D", "per_robot")
    nq, nu, nc, nb = pgc.dims("hopper_2D")[:4]
    K, xr = f["K"][:T], f["x_ref"][:T]
    args = (base["model"], base["q1"], base["v1"], base["u"][:T], base["h"], base["mu"])
    for robot in (0, 2):
        rng = np.random.default_rng(100 + robot)
        gq, gg, gb = np.zeros((T + 2, 3, nq)), np.zeros((T, 3, nc)), np.zeros((T, 3, nb))
        gq[:, robot], gg[:, robot], gb[:, robot] = [g[:, 0] for g in pac.random_cotangents(rng, T, 1, nq, nc, nb)]
        dK, dx = np.zeros(K.shape), np.zeros(xr.shape)
        dK[:, robot], dx[:, robot] = rng.standard_normal(K.shape[2:]), rng.standard_normal(xr.shape[2:])
        *_, tape, _ = plant.rollout_tape(*args, feedback=plant.Feedback(K, xr, n_sample=f["n_sample"]))
        with tape:
            cot = tape.vjp(gq, gg, gb)
        assert cot.n_cut.tolist() == [0, 0, 0]

        def loss(sK, sx):
            ok, q, ua, gam, b, st, it, e = plant.rollout(*args, feedback=plant.Feedback(K + sK * dK, xr + sx * dx, n_sample=f["n_sample"]))
            assert ok
            return float((gq * q).sum() + (gg * gam).sum() + (gb * b).sum())
        for what, adj, fd in (("K", float((cot.K * dK).sum()), (loss(eps, 0.0) - loss(-eps, 0.0)) / (2 * eps)),
                              ("x_ref", float((cot.x_ref * dx).sum()), (loss(0.0, eps) - loss(0.0, -eps)) / (2 * eps))):
            rel = abs(fd - adj) / max(abs(fd), abs(adj))
            print(f"robot {robot} d/d{what}: device chain {adj:.9e}, central differences of the device rollout {fd:.9e}, relative difference {rel:.2e}")
            assert rel <= 1e-4


# ---- 8. torch ----------------------------------------------------------------------------------------------------------------------------------
def test_rollout_torch_fills_the_gradients_of_the_gains_and_the_reference():
    import torch
    from contactimplicitmpc.jl_amd import plant
    which, variant = "hopper_2D", "held"
    c, f = pfc.base_case(which), pfc.feedback(which, variant)
    T, B = c["T"], 3
    leaf = lambda a: torch.tensor(np.array(a), dtype=torch.float64, requires_grad=True)
    K, xr, u = leaf(f["K"]), leaf(f["x_ref"]), leaf(c["u"])
    q, gamma, b, status = plant.rollout_torch(c["model"], c["q1"], c["v1"], u, c["h"], c["mu"],
                                              feedback=plant.Feedback(K, xr, hold=f["hold"], n_sample=f["n_sample"]))
    rng = np.random.default_rng(5)
    cw, dw = rng.standard_normal((B, 4)), rng.standard_normal((T, B, 1))
    ((q[-1] * torch.tensor(cw)).sum() + (gamma * torch.tensor(dw)).sum()).backward()
    *plain, tape, fb_err = plant.rollout_tape(*_args(c), feedback=_fb(which, variant))
    gq = np.zeros((T + 2, B, 4))
    gq[-1] = cw
    with tape:
        cot = tape.vjp(gq=gq, ggamma=dw)
    np.testing.assert_array_equal(q.detach().numpy(), plain[1])
    for got, want in ((K.grad, cot.K), (xr.grad, cot.x_ref), (u.grad, cot.u)):
        assert got.numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    assert K.grad.shape == f["K"].shape and np.abs(cot.K).max() > 0 and np.abs(cot.x_ref).max() > 0
    # u.grad keeps its meaning, the gradient of the open-loop part: an open-loop rollout gives another one
    *_, open_tape = plant.rollout_tape(*_args(c))
    with open_tape:
        open_cot = open_tape.vjp(gq=gq, ggamma=dw)
    assert open_cot.K is None and open_cot.x_ref is None and open_cot.xref_step is None
    assert not np.array_equal(open_cot.u, cot.u)


# ---- 9. cut steps ------------------------------------------------------------------------------------------------------------------------------
def test_unconverged_steps_cut_the_flow_and_are_counted_under_feedback():
    from contactimplicitmpc.jl_amd import plant
    c = pfc.base_case("hopper_2D")
    (ok, q, ua, gam, b, st, it), tape, fb_err = _tape("hopper_2D", "per_robot", opts=dataclasses.replace(plant.SIM_OPTS, max_iter=1))
    gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), 14, 3, 4, 1, 2)
    with tape:
        cot = tape.vjp(gq, gg, gb)
    assert not ok and (st == 0).all() and (tape.grad_status == 0).all()
    assert q.shape == (16, 3, 4) and np.isfinite(q).all() and np.isfinite(ua).all()      # the rollout goes on
    u, e = pfc.law_on(q, _ubar(c), pfc.feedback("hopper_2D", "per_robot"))
    np.testing.assert_array_equal(ua, u)
    assert cot.n_cut.tolist() == [14, 14, 14]
    for a in (cot.xref_step, cot.u_step, cot.K, cot.x_ref):
        np.testing.assert_array_equal(a, 0.0)
    np.testing.assert_array_equal(cot.g_q0, gq[0])
    np.testing.assert_array_equal(cot.g_q1, gq[1])


# ---- 10. the two vjp entry points --------------------------------------------------------------------------------------------------------------
def _vjp_raw(entry, tape, gq, T, B, nq, nu, xref):
    from contactimplicitmpc.jl_amd import _lib
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)
    out = [np.zeros((B, nq)), np.zeros((B, nq)), np.zeros((T, B, nu))]
    n_cut = np.zeros(B, dtype=np.int32)
    extra = () if entry == "cimpc_plant_tape_vjp" else (dp(xref),)
    rc = getattr(_lib.load(), entry)(tape._handle, dp(gq), None, None, *[dp(a) for a in out], None, None, None, n_cut.ctypes.data_as(_lib._ip), *extra)
    return rc, out


def test_plain_vjp_on_a_closed_loop_tape_runs_the_feedback_path_and_an_open_loop_tape_refuses_xref():
    from contactimplicitmpc.jl_amd import plant
    c = pfc.base_case("hopper_2D")
    T, B, nq, nu = 14, 3, 4, 2
    gq = np.random.default_rng(9).standard_normal((T + 2, B, nq))
    _, tape, _ = _tape("hopper_2D", "shared")
    with tape:
        rc_a, plain = _vjp_raw("cimpc_plant_tape_vjp", tape, gq, T, B, nq, nu, None)
        rc_b, null = _vjp_raw("cimpc_plant_tape_vjp_feedback", tape, gq, T, B, nq, nu, None)
        xref = np.zeros((T, B, 2 * nq))
        rc_c, full = _vjp_raw("cimpc_plant_tape_vjp_feedback", tape, gq, T, B, nq, nu, xref)
        cot = tape.vjp(gq)
    assert (rc_a, rc_b, rc_c) == (0, 0, 0)
    for a, b, w in zip(plain, null, full):
        assert a.tobytes() == b.tobytes() == w.tobytes()
    np.testing.assert_array_equal(full[0], cot.g_q0)
    np.testing.assert_array_equal(xref, cot.xref_step)
    *_, open_tape = plant.rollout_tape(*_args(c))
    with open_tape:
        rc, _ = _vjp_raw("cimpc_plant_tape_vjp_feedback", open_tape, gq, T, B, nq, nu, np.zeros((T, B, 2 * nq)))
        rc_null, out = _vjp_raw("cimpc_plant_tape_vjp_feedback", open_tape, gq, T, B, nq, nu, None)
        open_cot = open_tape.vjp(gq)
    assert rc == -1 and rc_null == 0
    np.testing.assert_array_equal(out[0], open_cot.g_q0)
    assert not np.array_equal(open_cot.g_q0, cot.g_q0)
