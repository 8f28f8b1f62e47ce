"""The reverse chain on the device (csrc/plant_adjoint.hip: `plant.rollout_tape`, `RolloutTape.vjp`, `plant.rollout_torch`) against the
restatements of tests/plant_adjoint_cases.py, on the blocks the device itself returns through `rollout(diff_sol=True)`:

    every output within 100 x max(d(chain_np, chain_ld), 2.2e-16) of chain_ld, relative to that output's max|chain_ld|, and
    bit for bit equal to chain_f64, the float64 restatement in the order the definition states.

The bound is built from the restatements alone, never from a figure of the device.  A scalar identity (test 3) is held to what those
per-output bounds allow an inner product: Σ_k bound_k max|chain_ld_k| ‖δ_k‖₁ over the outputs k that meet a direction δ_k.

Measured on one MI355X: every output of every case equals chain_f64 bit for bit and is at most 6.3e-15 from chain_ld (particle, g_mu;
bounds from 2.2e-14 to 3.8e-13).  Adjoint identity: hopper_2D 4.8e-13 of 277 (allowed 3.2e-9), quadruped 6.0e-13 of 141 (1.7e-9).  Flight
finite differences of the device rollout: 2.8e-6 (robot 0) and 3.1e-5 (robot 2), the figures of the CPU restatement to the printed
digits.  Timings: scripts/plant_adjoint_ab.py, profiles/plant_adjoint.json.
"""
import dataclasses

import numpy as np
import pytest

import plant_adjoint_cases as pac
import plant_gradient_cases as pgc

pytestmark = pytest.mark.gpu


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def _blocks(c, **kw):
    """`rollout(diff_sol=True)` with every column of θ: (the seven plain values, StepGradients)."""
    from contactimplicitmpc.jl_amd import plant
    *plain, G = plant.rollout(*_args(c), terrain=c["terrain"], diff_sol=True, grad_cols=pgc.dims(c["model"])[6], **kw)
    return plain, G


def _tape(c, **kw):
    from contactimplicitmpc.jl_amd import plant
    kw.setdefault("grad_cols", pgc.dims(c["model"])[6])
    *plain, tape = plant.rollout_tape(*_args(c), terrain=c["terrain"], **kw)
    return plain, tape


def _cotangents(c, T, seed=0):
    nq, nu, nc, nb = pgc.dims(c["model"])[:4]
    return pac.random_cotangents(np.random.default_rng(seed), T, c["q1"].shape[0], nq, nc, nb)


def _raw(cot):
    return dict(g_q0=cot.g_q0, g_q1=cot.g_q1, u_step=cot.u_step, w_step=cot.w_step, g_mu=cot.g_mu, g_h=cot.g_h)


def _parity(what, c, **kw):
    """The device chain of a case against the restatements on the device's own blocks; returns (tape, cotangents used, device result)."""
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
    plain, G = _blocks(c, **kw)
    same, tape = _tape(c, **kw)
    T = G.dz.shape[0]
    assert G.dz.shape[2:] == (nr, nth) and tape.n_cols == nth and tape.T == T and tape.B == c["q1"].shape[0]
    np.testing.assert_array_equal(tape.grad_status, G.status)
    gq, gg, gb = _cotangents(c, T)
    cot = tape.vjp(gq, gg, gb)
    ld, f64, bound = pac.bounds(G.dz, gq, gg, gb, nq, nu, nw)
    assert cot.n_cut.tolist() == (G.status == 0).sum(axis=0).tolist()
    figures = {}
    for k, dev in _raw(cot).items():
        figures[k] = pac.distance(dev, ld[k])
        print(f"{what} {k}: device {figures[k]:.2e} from chain_ld (bound {bound[k]:.2e}), bits equal chain_f64: "
              f"{dev.tobytes() == np.ascontiguousarray(f64[k]).tobytes()}")
    for k, dev in _raw(cot).items():
        assert figures[k] <= bound[k], f"{what} {k}: {figures[k]:.3e} > {bound[k]:.3e}"
        assert dev.tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{what} {k} differs from chain_f64"
    return tape, (gq, gg, gb), cot, (ld, bound), G


# ---- 1. chain parity on the device's own blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_chain_matches_the_restatements_on_the_devices_blocks(which):
    """hopper_2D B = 3 T = 14 (flight, impact, hard contact), particle on the bowl, quadruped B = 2 T = 6, centroidal_quadruped_wall
    (nr = 58, n_cols = 53: the largest block, 49 KB of LDS, and a block that is not wholly in flight during a step)."""
    tape, *_ = _parity(which, pgc.rollout_case(which))
    tape.close()


# ---- 2. the forward values are the rollout's ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hopper_2D", "particle"])
def test_rollout_tape_returns_the_rollouts_values(which):
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case(which)
    plain = plant.rollout(*_args(c), terrain=c["terrain"])
    *_, G = plant.rollout(*_args(c), terrain=c["terrain"], diff_sol=True)
    got, tape = _tape(c, grad_cols=None, keep_z=True)
    with tape:
        assert len(got) == 7 and got[0] == plain[0]
        for a, w in zip(got[1:], plain[1:]):
            np.testing.assert_array_equal(a, w)
        np.testing.assert_array_equal(tape.grad_status, G.status)
        np.testing.assert_array_equal(tape.z, G.z)
        assert tape.model == c["model"] and tape.n_cols == G.dz.shape[3]
    assert tape.closed


# ---- 3. the adjoint identity against the forward route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hopper_2D", "quadruped"])
def test_cotangents_are_adjoint_to_the_forward_tangents(which):
    """⟨cotangents, forward_tangent(δ) over StepGradients.dz⟩ = ⟨RolloutCotangents, δ⟩ for a random δ in (q1, v1, u, μ)."""
    c = pgc.rollout_case(which)
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(c["model"])
    tape, (gq, gg, gb), cot, (ld, bound), G = _parity(which, c)
    tape.close()
    T, B = G.status.shape
    rng = np.random.default_rng(3)
    dq1, dv1, du, dmu = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal(c["u"].shape), rng.standard_normal(B)
    dq0 = dq1 - c["h"] * dv1
    L = pac.LD
    dq, dgb = pac.forward_tangent(G.dz, dq0, dq1, du, nq, nu, nw, dmu=dmu)      # N_sample = 1: step t applies u[t]
    lhs = (np.asarray(gq, L) * dq).sum() + (np.concatenate([gg, gb], axis=2).astype(L) * dgb).sum()
    rhs = sum((np.asarray(a, L) * d).sum() for a, d in ((cot.q1, dq1), (cot.v1, dv1), (cot.u, du), (cot.mu, dmu)))
    tol = sum(bound[k] * float(np.abs(ld[k]).max()) * float(np.abs(d).sum())
              for k, d in (("g_q0", dq0), ("g_q1", dq1), ("u_step", du), ("g_mu", dmu)))
    print(f"{which}: <g, J d> = {float(lhs):.12e}, <J' g, d> = {float(rhs):.12e}, difference {float(abs(lhs - rhs)):.2e} (allowed {tol:.2e})")
    assert cot.mu.shape == (B,) and cot.u.shape == c["u"].shape
    assert float(abs(lhs - rhs)) <= tol


# ---- 4. schedules ------------------------------------------------------------------------------------------------------------------------------
def _hopper(**over):
    c = dict(pgc.rollout_case("hopper_2D"))
    c.update(over)
    return c


def test_held_controls_fold_back_onto_their_rows():
    """N_sample = 2, K = 3, steps = 7: rows 0, 0, 1, 1, 2, 2 and the last row held for step 6."""
    c = _hopper(u=pgc.rollout_case("hopper_2D")["u"][[0, 5, 9]] * 2.0)
    tape, _, cot, _, G = _parity("N_sample 2", c, N_sample=2, steps=7)
    tape.close()
    assert G.status.shape == (7, 3) and cot.u.shape == (3, 3, 2)
    np.testing.assert_array_equal(cot.u, pac.fold_u(cot.u_step, 3, 2, False))
    assert np.abs(cot.u[2]).max() > 0


def test_shared_controls_take_the_sum_over_the_robots():
    rows = pgc.rollout_case("hopper_2D")["u"][[0, 5, 9], 0] * 2.0                 # (K, nu): one schedule for every robot
    shared, per_robot = _hopper(u=rows), _hopper(u=np.repeat(rows[:, None, :], 3, axis=1))
    gq, gg, gb = _cotangents(shared, 7)
    out = []
    for c in (shared, per_robot):
        _, tape = _tape(c, N_sample=2, steps=7)
        with tape:
            out.append(tape.vjp(gq, gg, gb))
    np.testing.assert_array_equal(out[0].u_step, out[1].u_step)
    assert out[0].u.shape == (3, 2) and out[1].u.shape == (3, 3, 2)
    np.testing.assert_array_equal(out[0].u, pac.fold_u(out[1].u_step, 3, 2, True))
    want = np.zeros((3, 2))
    for t in range(7):                                                             # the fold's order: ascending (t, b)
        for r in range(3):
            want[min(t // 2, 2)] += out[1].u_step[t, r]
    np.testing.assert_array_equal(out[0].u, want / 2)


def test_held_disturbances_fold_back_onto_their_rows():
    w = np.array([[0.02, -0.01], [-0.03, 0.015]])                                  # (K_w, nw) shared, each held for 3 steps, the last from there on
    c = _hopper()
    tape, _, cot, _, G = _parity("w_hold 3", c, w=w, w_hold=3, steps=8)
    tape.close()
    want = np.zeros((2, 2))
    for t in range(8):
        for r in range(3):
            want[min(t // 3, 1)] += cot.w_step[t, r]
    assert cot.w.shape == (2, 2) and np.abs(cot.w_step).max() > 0
    np.testing.assert_array_equal(cot.w, want)


def test_one_friction_coefficient_takes_the_sum_over_the_robots():
    gq, gg, gb = _cotangents(_hopper(), 14)
    out = []
    for mu in (0.5, np.full(3, 0.5)):
        _, tape = _tape(_hopper(mu=mu))
        with tape:
            out.append(tape.vjp(gq, gg, gb))
    np.testing.assert_array_equal(out[0].g_mu, out[1].g_mu)
    assert np.ndim(out[0].mu) == 0 and out[1].mu.shape == (3,)
    assert out[0].mu == (out[1].mu[0] + out[1].mu[1]) + out[1].mu[2]
    assert np.abs(out[1].mu).max() > 0


def test_a_single_step():
    c = _hopper(u=pgc.rollout_case("hopper_2D")["u"][:1])
    tape, _, cot, _, G = _parity("T = 1", c)
    tape.close()
    assert G.status.shape == (1, 3) and cot.u_step.shape == (1, 3, 2)


# ---- 5. cut steps ------------------------------------------------------------------------------------------------------------------------------
def test_unconverged_steps_cut_the_flow_and_are_counted():
    from contactimplicitmpc.jl_amd import plant
    c = _hopper()
    (ok, q, ua, gam, b, st, it), tape = _tape(c, opts=dataclasses.replace(plant.SIM_OPTS, max_iter=1))
    gq, gg, gb = _cotangents(c, 14)
    with tape:
        cot = tape.vjp(gq, gg, gb)      # returns: the call itself succeeds
    assert not ok and (st == 0).all() and (tape.grad_status == 0).all()
    assert cot.n_cut.tolist() == [14, 14, 14]
    np.testing.assert_array_equal(cot.g_q0, gq[0])
    np.testing.assert_array_equal(cot.g_q1, gq[1])
    for a in (cot.u_step, cot.u, cot.w_step, cot.g_mu, cot.g_h):
        np.testing.assert_array_equal(a, 0.0)


# ---- 6. torch ----------------------------------------------------------------------------------------------------------------------------------
def test_rollout_torch_backpropagates_through_the_tape():
    import torch
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    T, B = c["T"], 3
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    q1, v1, u, mu = leaf(c["q1"]), leaf(c["v1"]), leaf(c["u"]), leaf(c["mu"])
    w = torch.zeros((2, 2), dtype=torch.float64)                                  # a tensor that asks for no gradient
    q, gamma, b, status = plant.rollout_torch(c["model"], q1, v1, u, c["h"], mu, w=w, w_hold=7)
    assert status.dtype == torch.int32 and not status.requires_grad and q.requires_grad and gamma.requires_grad
    rng = np.random.default_rng(5)
    cw, dw = rng.standard_normal((B, 4)), rng.standard_normal((T, B, 1))
    loss = (q[-1] * torch.tensor(cw)).sum() + (gamma * torch.tensor(dw)).sum()
    loss.backward(retain_graph=True)
    once = [a.grad.clone().numpy() for a in (q1, v1, u, mu)]
    assert w.grad is None
    # the same cotangents through the tape: mu asks for its column, nothing asks for h's
    *plain, tape = plant.rollout_tape(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], w=w.numpy(), w_hold=7, grad_cols=2 * 4 + 2 + 2 + 1)
    gq = np.zeros((T + 2, B, 4))
    gq[-1] = cw
    with tape:
        cot = tape.vjp(gq=gq, ggamma=dw)
    np.testing.assert_array_equal(q.detach().numpy(), plain[1])
    for got, want in zip(once, (cot.q1, cot.v1, cot.u, cot.mu)):
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    assert np.abs(cot.u).max() > 0 and np.abs(cot.mu).max() > 0
    loss.backward()                                                                # a second walk of the same tape
    for a, g1 in zip((q1, v1, u, mu), once):
        np.testing.assert_array_equal(a.grad.numpy(), 2.0 * g1)
    # a leaf that does not ask gets None, the others are unchanged
    q1b, v1b = leaf(c["q1"]), torch.tensor(c["v1"])
    qb, *_ = plant.rollout_torch(c["model"], q1b, v1b, c["u"], c["h"], c["mu"])
    (qb[-1] * torch.tensor(cw)).sum().backward()
    assert v1b.grad is None and q1b.grad is not None and np.isfinite(q1b.grad.numpy()).all()


# ---- 7. finite differences of the device rollout, in flight --------------------------------------------------------------------------------
def test_chain_matches_finite_differences_of_the_device_rollout_in_flight():
    """hopper_2D steps 0-3, robots 0 and 2, ε = 1e-5, central differences of `plant.rollout`, a loss linear in (q, γ, b) and a random
    direction in (q1, v1, u): the relative difference is held to 1e-4, the bound of the CPU restatement (tests/test_plant_adjoint.py)."""
    from contactimplicitmpc.jl_amd import plant
    T, eps = 4, 1e-5
    base = pgc.rollout_case("hopper_2D")
    c = _hopper(u=base["u"][:T])
    nq, nu, nc, nb = pgc.dims("hopper_2D")[:4]
    for robot in (0, 2):
        rng = np.random.default_rng(100 + robot)
        gq, gg, gb = np.zeros((T + 2, 3, nq)), np.zeros((T, 3, nc)), np.zeros((T, 3, nb))
        gq[:, robot], gg[:, robot], gb[:, robot] = [g[:, 0] for g in pac.random_cotangents(rng, T, 1, nq, nc, nb)]
        dq1, dv1, du = np.zeros((3, nq)), np.zeros((3, nq)), np.zeros((T, 3, nu))
        dq1[robot], dv1[robot], du[:, robot] = rng.standard_normal(nq), rng.standard_normal(nq), rng.standard_normal((T, nu))
        _, tape = _tape(c)
        with tape:
            cot = tape.vjp(gq, gg, gb)
        assert cot.n_cut.tolist() == [0, 0, 0]
        adj = float((cot.q1 * dq1).sum() + (cot.v1 * dv1).sum() + (cot.u * du).sum())

        def loss(s):
            ok, q, ua, gam, b, st, it = plant.rollout(c["model"], c["q1"] + s * dq1, c["v1"] + s * dv1, c["u"] + s * du, c["h"], c["mu"])
            assert ok
            return float((gq * q).sum() + (gg * gam).sum() + (gb * b).sum())
        fd = (loss(eps) - loss(-eps)) / (2 * eps)
        rel = abs(fd - adj) / max(abs(fd), abs(adj))
        print(f"robot {robot}: device chain {adj:.9e}, central differences of the device rollout {fd:.9e}, relative difference {rel:.2e}")
        assert rel <= 1e-4


# ---- 8. the tape's lifetime ----------------------------------------------------------------------------------------------------------------
def test_tapes_are_independent_reusable_and_refuse_use_after_close():
    hop, par = pgc.rollout_case("hopper_2D"), pgc.rollout_case("particle")
    _, t_hop = _tape(hop)
    _, t_par = _tape(par)                                                          # two tapes alive at once
    g_hop, g_par = _cotangents(hop, 14, seed=1), _cotangents(par, 14, seed=2)
    a1 = t_hop.vjp(*g_hop)
    b1 = t_par.vjp(*g_par)
    a2 = t_hop.vjp(*g_hop)                                                         # again, after the other tape was walked
    for k, v in _raw(a1).items():
        assert v.tobytes() == _raw(a2)[k].tobytes(), k
    t_hop.close()
    b2 = t_par.vjp(*g_par)                                                         # the other tape outlives it
    for k, v in _raw(b1).items():
        assert v.tobytes() == _raw(b2)[k].tobytes(), k
    _, t_alone = _tape(hop)                                                        # and each is what it is alone
    with t_alone:
        a3 = t_alone.vjp(*g_hop)
    for k, v in _raw(a1).items():
        assert v.tobytes() == _raw(a3)[k].tobytes(), k
    with pytest.raises(ValueError):
        t_hop.vjp(*g_hop)
    t_hop.close()                                                                  # closing twice is harmless
    t_par.close()
    assert t_hop.closed and t_par.closed and t_alone.closed
