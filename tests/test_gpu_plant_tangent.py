"""The forward chain on the device (csrc/plant_tangent.hip: `RolloutTape.jvp`, `RolloutTape.transition`, forward mode of
`plant.rollout_torch`) against the restatements of tests/plant_tangent_cases.py, on the blocks the device itself returns through
`rollout(diff_sol=True)`:

    every output bit for bit equal to tangent_f64, the float64 restatement in the order the definition states, and within
    100 x max(d(tangent_np, tangent_ld), 2.2e-16) of tangent_ld, relative to that output's max|tangent_ld|.

The bound is built from the restatements alone, never from a figure of the device.  The adjoint identity (test 4) is held to the formula
of test 3 of tests/test_gpu_plant_adjoint.py, the finite differences in flight (test 5) to its 1e-4.

Measured on one MI355X: every bit-for-bit comparison holds on every case, alone and with 65 directions stacked, and every stacked
direction equals itself launched alone.  Distance from tangent_ld: hopper_2D 9.5e-15, particle 3.0e-15, quadruped 4.0e-15,
centroidal_quadruped_wall 3.4e-16; closed loop at most 5.9e-15 (hopper_2D, shared) over the 15 case-schedule pairs; bounds from 2.2e-14.
Adjoint identity on the device: hopper_2D 6.8e-14 of 277 (allowed 4.0e-9), quadruped 6.1e-13 of 141 (9.3e-10).  Flight finite
differences of the device rollout: 2.8e-6 (robot 0) and 3.1e-5 (robot 2) of the derivative, the adjoint test's figures.  `transition()`
at most 1.8e-15 from the longdouble product of the step matrices (bounds from 4.2e-14).  Timings: scripts/plant_tangent_ab.py,
profiles/plant_tangent.json.
"""
import dataclasses
import functools

import numpy as np
import pytest

import plant_adjoint_cases as pac
import plant_feedback_cases as pfc
import plant_gradient_cases as pgc
import plant_tangent_cases as ptc

pytestmark = pytest.mark.gpu

PAIRS = [(w, v) for w in pfc.CASES for v in pfc.variants(w)]
IDS = [f"{w}-{v}" for w, v in PAIRS]


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def _w(c):
    """One shared row of zero disturbances, so that the rollout has a w to take a tangent of."""
    return np.zeros((1, pgc.dims(c["model"])[4]))


@functools.lru_cache(maxsize=None)
def _blocks(which):
    """`rollout(diff_sol=True)` of a rollout case with every column of θ, once per process: StepGradients (read-only)."""
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case(which)
    *_, G = plant.rollout(*_args(c), terrain=c["terrain"], w=_w(c), diff_sol=True, grad_cols=pgc.dims(c["model"])[6])
    G.dz.setflags(write=False); G.status.setflags(write=False)
    return G


def _tape(c, **kw):
    from contactimplicitmpc.jl_amd import plant
    kw.setdefault("grad_cols", pgc.dims(c["model"])[6])
    kw.setdefault("w", _w(c))
    *plain, tape = plant.rollout_tape(*_args(c), terrain=c["terrain"], **kw)
    return plain, tape


def _random_arguments(rng, c, n_dir=None, closed=None):
    """A random δ in every argument of the rollout, in the caller's shapes (with a leading axis of n_dir when given)."""
    lead = () if n_dir is None else (n_dir,)
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    B = c["q1"].shape[0]
    d = dict(dq1=rng.standard_normal(lead + (B, nq)), dv1=rng.standard_normal(lead + (B, nq)), du=rng.standard_normal(lead + c["u"].shape),
             dw=rng.standard_normal(lead + (1, nw)), dmu=rng.standard_normal(lead + (B,)), dh=rng.standard_normal(lead) * c["h"])
    if closed is not None:
        d.update(dK=rng.standard_normal(lead + np.shape(closed["K"])), dx_ref=rng.standard_normal(lead + np.shape(closed["x_ref"])))
    return d


def _directions(c, T, args, n_dir, **kw):
    """The arguments as directions of the chain, one dict per direction (`plant_tangent_cases.step_inputs`)."""
    B = c["q1"].shape[0]
    pick = (lambda a, d: a) if n_dir is None else (lambda a, d: a[d])
    return [ptc.step_inputs(T, B, c["h"], c["v1"], **{k: pick(a, d) for k, a in args.items()}, **kw) for d in range(n_dir or 1)]


def _compare(what, got, D, dirs, dims, loop=None, checked=(0,)):
    """Device outputs (leading axis of directions) against tangent_f64, bit for bit in every direction, and against tangent_ld within
    its bound in the `checked` directions.  Returns the largest distance from tangent_ld."""
    nq, nu, nc, nb, nw = dims[:5]
    f64 = ptc.stacked(ptc.tangent_f64, D, dirs, nq, nu, nw, nc, loop)
    worst = 0.0
    for d in checked:
        ld, _, bound = ptc.bounds(D, dirs[d], nq, nu, nw, nc, loop)
        for k in bound:
            dist = pac.distance(got[k][d], ld[k])
            worst = max(worst, dist)
            print(f"{what}, direction {d}, {k}: device {dist:.2e} from tangent_ld (bound {bound[k]:.2e}), bits equal tangent_f64: "
                  f"{got[k][d].tobytes() == np.ascontiguousarray(f64[k][d]).tobytes()}")
            assert dist <= bound[k], f"{what} {k}: {dist:.3e} > {bound[k]:.3e}"
    for k in ptc.OUTPUTS:
        assert (got[k] is None) == (f64[k] is None), k
        if got[k] is not None:
            assert got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{what} {k} differs from tangent_f64"
    return worst


def _out(t, stacked=True):
    lift = (lambda a: a) if stacked else (lambda a: None if a is None else a[None])
    return dict(q=lift(t.q), gamma=lift(t.gamma), b=lift(t.b), u_applied=lift(t.u_applied))


# ---- 1. parity on the device's own blocks, 2. grouping does not matter -----------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_tangents_match_the_restatements_on_the_devices_blocks(which):
    """hopper_2D B = 3 T = 14, particle on the bowl, quadruped B = 2 T = 6, centroidal_quadruped_wall (the largest block): a random δ in
    every argument, once alone (n_dir = 1, unstacked) and once with the plan's group + 1 directions, so that the last rides in a second
    workgroup; then every direction of the stacked run launched alone returns the same bits."""
    c, G = pgc.rollout_case(which), _blocks(which)
    dims = pgc.dims(c["model"])
    T, B = G.status.shape
    _, tape = _tape(c)
    with tape:
        np.testing.assert_array_equal(tape.grad_status, G.status)
        n_dir = tape.group + 1
        assert n_dir == 65
        one = _random_arguments(np.random.default_rng(1), c)
        t1 = tape.jvp(**one)
        assert t1.q.shape == (T + 2, B, dims[0]) and t1.u_applied is None
        assert t1.n_cut.tolist() == (G.status == 0).sum(axis=0).tolist()
        worst = _compare(f"{which} alone", _out(t1, False), G.dz, _directions(c, T, one, None), dims)
        many = _random_arguments(np.random.default_rng(2), c, n_dir)
        tn = tape.jvp(**many)
        assert tn.q.shape == (n_dir, T + 2, B, dims[0]) and tn.n_cut.tolist() == t1.n_cut.tolist()
        worst = max(worst, _compare(f"{which} stacked", _out(tn), G.dz, _directions(c, T, many, n_dir), dims, checked=(0, n_dir - 1)))
        print(f"{which}: at most {worst:.2e} from tangent_ld")
        for d in range(n_dir):      # grouping does not matter
            alone = tape.jvp(**{k: a[d] for k, a in many.items()})
            for k in ("q", "gamma", "b"):
                assert getattr(alone, k).tobytes() == getattr(tn, k)[d].tobytes(), (d, k)


# ---- 3. closed loop ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closed(which, variant):
    from contactimplicitmpc.jl_amd import plant
    c, f = pfc.base_case(which), pfc.feedback(which, variant)
    fb = plant.Feedback(f["K"], f["x_ref"], hold=f["hold"], n_sample=f["n_sample"])
    out = plant.rollout(*_args(c), terrain=c["terrain"], w=_w(c), steps_per_launch=pfc.STEPS_PER_LAUNCH, diff_sol=True,
                        grad_cols=pgc.dims(c["model"])[6], feedback=fb)
    return dict(G=out[7], fb_err=out[8], fb=fb)


@pytest.mark.parametrize("which,variant", PAIRS, ids=IDS)
def test_closed_loop_tangents_match_the_restatement(which, variant):
    """The seven cases of tests/plant_feedback_cases.py (one per step instantiation) with their schedules, δK and δx_ref included, three
    directions stacked: bit for bit the closed-loop restatement, and the tangents of the applied controls come back."""
    c, f, r = pfc.base_case(which), pfc.feedback(which, variant), _closed(which, variant)
    dims = pgc.dims(c["model"])
    G = r["G"]
    T, B = G.status.shape
    from contactimplicitmpc.jl_amd import plant
    *_, tape, fb_err = plant.rollout_tape(*_args(c), terrain=c["terrain"], w=_w(c), grad_cols=dims[6], feedback=r["fb"],
                                          steps_per_launch=pfc.STEPS_PER_LAUNCH)
    n_dir = 3
    with tape:
        np.testing.assert_array_equal(fb_err, r["fb_err"])
        args = _random_arguments(np.random.default_rng(4), c, n_dir, closed=f)
        t = tape.jvp(**args)
    Ks, _ = pfc.per_step(f, T, B)                                                 # N_sample = 1: the device's rows are K as it stands
    dirs = _directions(c, T, args, n_dir, fb_hold=f["hold"], fb_err=r["fb_err"])
    worst = _compare(f"{which} {variant}", _out(t), G.dz, dirs, dims, loop=(Ks, f["n_sample"]), checked=(0,))
    print(f"{which} {variant}: at most {worst:.2e} from tangent_ld")
    assert t.u_applied.shape == (n_dir, T, B, dims[1]) and np.abs(t.u_applied - np.stack([d["du_step"] for d in dirs])).max() > 0
    assert t.n_cut.tolist() == [0] * B


# ---- 4. the adjoint identity on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hopper_2D", "quadruped"])
def test_tangents_are_adjoint_to_the_cotangents_on_the_device(which):
    """⟨g, jvp(δ)⟩ = ⟨vjp(g), δ⟩ for a random δ in (q1, v1, u, μ), both sides from the device, held to the formula of test 3 of
    tests/test_gpu_plant_adjoint.py: Σ_k bound_k max|chain_ld_k| ‖δ_k‖₁ over the outputs k of the reverse chain that meet a direction."""
    c, G = pgc.rollout_case(which), _blocks(which)
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = G.status.shape
    rng = np.random.default_rng(3)
    gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), T, B, nq, nc, nb)
    dq1, dv1, du, dmu = rng.standard_normal((B, nq)), rng.standard_normal((B, nq)), rng.standard_normal(c["u"].shape), rng.standard_normal(B)
    _, tape = _tape(c)
    with tape:
        cot = tape.vjp(gq, gg, gb)
        tan = tape.jvp(dq1=dq1, dv1=dv1, du=du, dmu=dmu)
    ld, f64, bound = pac.bounds(G.dz, gq, gg, gb, nq, nu, nw)
    L = pac.LD
    dq0 = dq1 - c["h"] * dv1
    lhs = (np.asarray(gq, L) * tan.q).sum() + (np.asarray(gg, L) * tan.gamma).sum() + (np.asarray(gb, L) * tan.b).sum()
    rhs = sum((np.asarray(a, L) * d).sum() for a, d in ((cot.q1, dq1), (cot.v1, dv1), (cot.u, du), (cot.mu, dmu)))
    tol = sum(bound[k] * float(np.abs(ld[k]).max()) * float(np.abs(d).sum())
              for k, d in (("g_q0", dq0), ("g_q1", dq1), ("u_step", du), ("g_mu", dmu)))
    print(f"{which}: <g, jvp(d)> = {float(lhs):.12e}, <vjp(g), d> = {float(rhs):.12e}, difference {float(abs(lhs - rhs)):.2e} (allowed {tol:.2e})")
    assert float(abs(lhs - rhs)) <= tol


# ---- 5. finite differences of the device rollout, in flight --------------------------------------------------------------------------------
def test_tangents_match_finite_differences_of_the_device_rollout_in_flight():
    """The construction of test_chain_matches_finite_differences_of_the_device_rollout_in_flight (tests/test_gpu_plant_adjoint.py):
    hopper_2D steps 0-3, robots 0 and 2, ε = 1e-5, the same seeds, a loss linear in (q, γ, b) and a random direction in (q1, v1, u):
    ⟨g, jvp(δ)⟩ against the central difference of `plant.rollout`, held to 1e-4."""
    from contactimplicitmpc.jl_amd import plant
    T, eps = 4, 1e-5
    base = pgc.rollout_case("hopper_2D")
    c = dict(base, u=base["u"][:T])
    nq, nu, nc, nb = pgc.dims("hopper_2D")[:4]
    for robot in (0, 2):
        rng = np.random.default_rng(100 + robot)
        gq, gg, gb = np.zeros((T + 2, 3, nq)), np.zeros((T, 3, nc)), np.zeros((T, 3, nb))
        gq[:, robot], gg[:, robot], gb[:, robot] = [g[:, 0] for g in pac.random_cotangents(rng, T, 1, nq, nc, nb)]
        dq1, dv1, du = np.zeros((3, nq)), np.zeros((3, nq)), np.zeros((T, 3, nu))
        dq1[robot], dv1[robot], du[:, robot] = rng.standard_normal(nq), rng.standard_normal(nq), rng.standard_normal((T, nu))
        _, tape = _tape(c)
        with tape:
            tan = tape.jvp(dq1=dq1, dv1=dv1, du=du)
        assert tan.n_cut.tolist() == [0, 0, 0]
        jv = float((gq * tan.q).sum() + (gg * tan.gamma).sum() + (gb * tan.b).sum())

        def loss(s):
            ok, q, ua, gam, b, st, it = plant.rollout(c["model"], c["q1"] + s * dq1, c["v1"] + s * dv1, c["u"] + s * du, c["h"], c["mu"])
            assert ok
            return float((gq * q).sum() + (gg * gam).sum() + (gb * b).sum())
        fd = (loss(eps) - loss(-eps)) / (2 * eps)
        rel = abs(fd - jv) / max(abs(fd), abs(jv))
        print(f"robot {robot}: device tangent {jv:.9e}, central differences of the device rollout {fd:.9e}, relative difference {rel:.2e}")
        assert rel <= 1e-4


# ---- 6. the transition matrix --------------------------------------------------------------------------------------------------------------
def test_transition_is_the_product_of_the_step_matrices():
    """hopper_2D: Φ = A_{T-1} ... A_0 with A_t = [0 I; ∂q3/∂q1 ∂q3/∂q2] from `StepGradients`, in longdouble; `transition()` within
    100 x max(d(the float64 product, the longdouble product), 2.2e-16) of it per robot, relative to max|Φ|."""
    c, G = pgc.rollout_case("hopper_2D"), _blocks("hopper_2D")
    nq = pgc.dims("hopper_2D")[0]
    T, B = G.status.shape

    def product(dtype, t1):
        out = []
        for b in range(B):
            P = np.eye(2 * nq, dtype=dtype)
            for t in range(t1):
                A = np.zeros((2 * nq, 2 * nq), dtype=dtype)
                A[:nq, nq:] = np.eye(nq)
                A[nq:, :nq], A[nq:, nq:] = G.dq3_dq1[t, b], G.dq3_dq2[t, b]
                P = A @ P
            out.append(P)
        return np.array(out)
    _, tape = _tape(c)
    with tape:
        Phi, Phi3, Phi0 = tape.transition(), tape.transition(t1=3), tape.transition(t1=0)
        with pytest.raises(ValueError):
            tape.transition(t0=1)
        with pytest.raises(ValueError):
            tape.transition(t1=T + 1)
    assert Phi.shape == Phi3.shape == (B, 2 * nq, 2 * nq)
    np.testing.assert_array_equal(Phi0, np.broadcast_to(np.eye(2 * nq), (B, 2 * nq, 2 * nq)))
    for name, got, t1 in (("T", Phi, T), ("3", Phi3, 3)):
        ld, f64 = product(pac.LD, t1), product(np.float64, t1)
        for b in range(B):
            bound = pac.FACTOR * max(pac.distance(f64[b], ld[b]), 2.2e-16)
            dist = pac.distance(got[b], ld[b])
            print(f"transition to {name}, robot {b}: device {dist:.2e} from the longdouble product (bound {bound:.2e}), max|Phi| {float(np.abs(ld[b]).max()):.3e}")
            assert dist <= bound
    assert np.abs(Phi).max() > 0


# ---- 7. cut steps ------------------------------------------------------------------------------------------------------------------------------
def test_unconverged_steps_cut_the_flow_and_are_counted():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    (ok, q, ua, gam, b, st, it), tape = _tape(c, opts=dataclasses.replace(plant.SIM_OPTS, max_iter=1))
    args = _random_arguments(np.random.default_rng(6), c, 2)
    with tape:
        t = tape.jvp(**args)      # returns: the call itself succeeds
    assert not ok and (tape.grad_status == 0).all()
    assert t.n_cut.tolist() == [14, 14, 14]
    dirs = _directions(c, 14, args, 2)
    for d in range(2):
        np.testing.assert_array_equal(t.q[d, 0], dirs[d]["dq0"])
        np.testing.assert_array_equal(t.q[d, 1], dirs[d]["dq1"])
    for a in (t.q[:, 2:], t.gamma, t.b):
        np.testing.assert_array_equal(a, 0.0)


# ---- 8. torch ----------------------------------------------------------------------------------------------------------------------------------
def test_rollout_torch_answers_forward_mode_through_the_tape():
    import torch
    import torch.autograd.forward_ad as fwAD
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    rng = np.random.default_rng(8)
    du, dmu = rng.standard_normal(c["u"].shape), rng.standard_normal(3)
    with fwAD.dual_level():
        u = fwAD.make_dual(torch.tensor(c["u"]), torch.tensor(du))
        q, gamma, b, status = plant.rollout_torch(c["model"], c["q1"], c["v1"], u, c["h"], c["mu"])
        tq, tg = fwAD.unpack_dual(q).tangent, fwAD.unpack_dual(gamma).tangent
        assert fwAD.unpack_dual(status).tangent is None
        mu = fwAD.make_dual(torch.tensor(c["mu"]), torch.tensor(dmu))
        q2, *_ = plant.rollout_torch(c["model"], c["q1"], c["v1"], u, c["h"], mu)
        tq2 = fwAD.unpack_dual(q2).tangent
    *plain, tape = plant.rollout_tape(*_args(c))
    with tape:
        t = tape.jvp(du=du)
    *_, tape_mu = plant.rollout_tape(*_args(c), grad_cols=2 * 4 + 2 + 2 + 1)
    with tape_mu:
        t2 = tape_mu.jvp(du=du, dmu=dmu)
    np.testing.assert_array_equal(q.detach().numpy(), plain[1])
    assert tq.numpy().tobytes() == t.q.tobytes() and tg.numpy().tobytes() == t.gamma.tobytes()
    assert tq2.numpy().tobytes() == t2.q.tobytes() and not np.array_equal(t2.q, t.q)
    assert np.abs(t.q).max() > 0


# ---- 9. the tape's lifetime --------------------------------------------------------------------------------------------------------------------
def test_jvp_and_vjp_interleave_on_tapes_alive_at_once_and_a_closed_tape_refuses():
    hop, par = pgc.rollout_case("hopper_2D"), pgc.rollout_case("particle")
    _, t_hop = _tape(hop)
    _, t_par = _tape(par)
    d_hop, d_par = _random_arguments(np.random.default_rng(1), hop, 3), _random_arguments(np.random.default_rng(2), par)
    g_hop = pac.random_cotangents(np.random.default_rng(3), 14, 3, 4, 1, 2)
    a1 = t_hop.jvp(**d_hop)
    v1 = t_hop.vjp(*g_hop)
    b1 = t_par.jvp(**d_par)
    a2 = t_hop.jvp(**d_hop)                                                        # again, after a vjp and the other tape's jvp
    v2 = t_hop.vjp(*g_hop)
    for k in ("q", "gamma", "b"):
        assert getattr(a1, k).tobytes() == getattr(a2, k).tobytes(), k
    assert v1.g_q0.tobytes() == v2.g_q0.tobytes() and v1.u_step.tobytes() == v2.u_step.tobytes()
    t_hop.close()
    b2 = t_par.jvp(**d_par)                                                        # the other tape outlives it
    assert b1.q.tobytes() == b2.q.tobytes()
    with pytest.raises(ValueError):
        t_hop.jvp(**d_hop)
    with pytest.raises(ValueError):
        t_hop.transition()
    t_par.close()
    assert t_hop.closed and t_par.closed


# ---- 10. what is refused with a tape in hand -----------------------------------------------------------------------------------------------
def test_tangents_the_tape_does_not_cover_are_refused_and_both_entries_run_a_closed_loop_tape():
    from contactimplicitmpc.jl_amd import _lib, plant
    c = pgc.rollout_case("hopper_2D")
    T, B, nq, nu, nw = 14, 3, 4, 2, 2
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib._dp)
    dq1, dq, n_cut = np.random.default_rng(0).standard_normal((1, B, nq)), np.zeros((1, T + 2, B, nq)), np.zeros(B, dtype=np.int32)
    cut = n_cut.ctypes.data_as(_lib._ip)
    lib = _lib.load()
    *_, short = plant.rollout_tape(*_args(c), w=_w(c))                            # grad_cols = 2nq + nu: no w, μ, h columns
    with short:
        ones = np.ones((1, B))
        assert lib.cimpc_plant_tape_jvp(short._handle, 1, None, dp(dq1), None, dp(np.ones((1, T, B, nw))), None, None, dp(dq), None, None, cut) == -1
        assert lib.cimpc_plant_tape_jvp(short._handle, 1, None, dp(dq1), None, None, dp(ones), None, dp(dq), None, None, cut) == -1
        assert lib.cimpc_plant_tape_jvp(short._handle, 1, None, dp(dq1), None, None, None, dp(ones), dp(dq), None, None, cut) == -1
        assert lib.cimpc_plant_tape_jvp_feedback(short._handle, 1, None, dp(dq1), None, None, None, None, dp(dq), None, None, cut,
                                                 dp(np.ones((1, T, B, 2 * nq))), None) == -1
        assert lib.cimpc_plant_tape_jvp_feedback(short._handle, 1, None, dp(dq1), None, None, None, None, dp(dq), None, None, cut,
                                                 None, dp(np.ones((1, T, B, nu)))) == -1
        # an open-loop tape through the feedback entry with its two arguments null: the plain call; δq1 alone moves q[0] and q[1] alike
        assert lib.cimpc_plant_tape_jvp_feedback(short._handle, 1, dp(dq1), dp(dq1), None, None, None, None, dp(dq), None, None, cut, None, None) == 0
        np.testing.assert_array_equal(dq[0], short.jvp(dq1=dq1[0]).q)
        for bad in (dict(dmu=np.ones(B)), dict(dh=1.0), dict(dw=np.ones((1, nw))), dict(dK=np.ones((T, nu, 2 * nq))), dict(dx_ref=np.ones((T, 2 * nq))),
                    dict(dq1=np.full((B, nq), np.nan)), dict(dq1=np.ones((B, nq + 1))), dict(dq1=np.ones((2, B, nq)), dv1=np.ones((3, B, nq))), dict()):
            with pytest.raises(ValueError):
                short.jvp(**bad)
    f = pfc.feedback("hopper_2D", "shared")
    *_, closed, fb_err = plant.rollout_tape(*_args(c), feedback=plant.Feedback(f["K"], f["x_ref"], hold=f["hold"], n_sample=f["n_sample"]))
    with closed:
        plain, full = np.zeros_like(dq), np.zeros_like(dq)
        assert lib.cimpc_plant_tape_jvp(closed._handle, 1, None, dp(dq1), None, None, None, None, dp(plain), None, None, cut) == 0
        assert lib.cimpc_plant_tape_jvp_feedback(closed._handle, 1, None, dp(dq1), None, None, None, None, dp(full), None, None, cut, None, None) == 0
    assert plain.tobytes() == full.tobytes() and not np.array_equal(plain, dq)      # the feedback statements ran through either entry
