"""The LQ backward pass on the device (csrc/plant_riccati.hip: `RolloutTape.lqr`, `TapeGains.feedback`) against the restatements of
tests/plant_riccati_cases.py, on the blocks the device itself returns through `rollout(diff_sol=True)`:

    every output bit for bit equal to lq_f64, the float64 restatement in the order csrc/plant_riccati.h states, and within
    100 x max(d(lq_np, lq_ld), 2.2e-16) of lq_ld, relative to that output's max|lq_ld|.

The bounds are built from the restatements alone, never from a figure of the device.  Shapes: those of `plant_gradient_cases.ROLLOUTS`
(hopper_2D B 3 T 14, particle B 1 T 14, quadruped B 2 T 6, centroidal_quadruped_wall B 1 T 2).

Measured on one MI355X: every bit-for-bit comparison holds on every case.  Distance from lq_ld: hopper_2D 7.1e-15 (three laps 6.5e-14,
bound 5.2e-12), particle 3.6e-15, quadruped 5.8e-15, centroidal_quadruped_wall 1.3e-15, the closed-loop tape 8.3e-15, the all-cut tape
1.7e-16; bounds from 2.2e-14.  `gains.tvlqr` on the gathered dense matrices: at most 5.3e-15 from lq_ld and 5.6e-15 from `lqr`.
`transition()` under `feedback()`: at most 2.4e-15 from the longdouble product of A - B K (bounds from 4.7e-14), the open loop's product
0.9 to 2.0 away.  Timings: scripts/plant_riccati_ab.py, profiles/plant_riccati.json.
"""
import dataclasses
import functools

import numpy as np
import pytest

import plant_adjoint_cases as pac
import plant_feedback_cases as pfc
import plant_gradient_cases as pgc
import plant_riccati_cases as prc

pytestmark = pytest.mark.gpu


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def _w(c):
    return np.zeros((1, pgc.dims(c["model"])[4]))


@functools.lru_cache(maxsize=None)
def _blocks(which):
    """`rollout(diff_sol=True)` of a rollout case with every column of θ (so that a block's columns outnumber the corner's), once per
    process: StepGradients (read-only)."""
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


def _weights(which, T, B, per_step=False, seed=0):
    """(Q, R, Qf, q, r) for a case: random symmetric positive definite weights, random linear terms."""
    nq, nu = pgc.dims(which)[:2]      # the four cases are named after their models
    rng = np.random.default_rng([seed, nq, nu, T])
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step)
    return Q, R, Qf, rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))


def _out(g):
    return dict(K=g.K, k=g.k, P0=g.P0, p0=g.p0, dV=g.dV, status=g.status, n_cut=g.n_cut)


def _compare(what, got, D, status, nq, nu, Q, R, Qf, **kw):
    """Device outputs against lq_f64 bit for bit and against lq_ld within its bounds; returns the largest distance from lq_ld."""
    ld, f64, bound = prc.bounds(D, status, nq, nu, Q, R, Qf, **kw)
    worst = 0.0
    for k in bound:
        dist = pac.distance(got[k], ld[k])
        worst = max(worst, dist)
        print(f"{what}, {k}: device {dist:.2e} from lq_ld (bound {bound[k]:.2e}), bits equal lq_f64: "
              f"{got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes()}")
        assert dist <= bound[k], f"{what} {k}: {dist:.3e} > {bound[k]:.3e}"
    for k in prc.OUTPUTS:
        assert (got[k] is None) == (f64[k] is None), k
        if got[k] is not None:
            assert got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{what} {k} differs from lq_f64"
    assert got["status"].tolist() == f64["status"].tolist() and got["n_cut"].tolist() == f64["n_cut"].tolist()
    return worst


# ---- a. parity on the device's own blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_gains_match_the_restatements_on_the_devices_blocks(which):
    """The pure-gain call (constant weights) and the call with linear terms (per-step weights, rho > 0); on hopper_2D also three laps with
    keep 5."""
    c, G = pgc.rollout_case(which), _blocks(which)
    nq, nu = pgc.dims(c["model"])[:2]
    T, B = G.status.shape
    Q, R, Qf, _, _ = _weights(which, T, B)
    Qs, Rs, Qfs, q, r = _weights(which, T, B, per_step=True, seed=1)
    _, tape = _tape(c)
    with tape:
        np.testing.assert_array_equal(tape.grad_status, G.status)
        pure = tape.lqr(Q, R, Qf)
        lin = tape.lqr(Qs, Rs, Qfs, q=q, r=r, rho=1e-2)
        laps = tape.lqr(Q, R, laps=3, keep=min(5, T)) if which == "hopper_2D" else None
    assert pure.K.shape == (T, B, nu, 2 * nq) and pure.k is None and pure.p0 is None and pure.dV is None and pure.status.tolist() == [0] * B
    assert lin.k.shape == (T, B, nu) and lin.p0.shape == (B, 2 * nq) and lin.dV.shape == (B, 2) and np.abs(lin.K).max() > 0
    worst = _compare(f"{which} pure", _out(pure), G.dz, G.status, nq, nu, Q, R, Qf)
    worst = max(worst, _compare(f"{which} linear", _out(lin), G.dz, G.status, nq, nu, Qs, Rs, Qfs, q=q, r=r, rho=1e-2))
    if laps is not None:
        assert laps.K.shape == (5, B, nu, 2 * nq)
        worst = max(worst, _compare(f"{which} laps", _out(laps), G.dz, G.status, nq, nu, Q, R, Q, laps=3, keep=5))
    print(f"{which}: at most {worst:.2e} from lq_ld")


# ---- b. the existing device Riccati chain on the dense matrices ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_gains_agree_with_tvlqr_on_the_gathered_dense_matrices(which):
    """`gains.tvlqr` (tvlqr_kernel, the dense chain) on A_t, B_t gathered on the host, n_prob = B: the same K and P0 within the bounds of
    lq_ld - not bit for bit, the dense chain sums over the zero blocks too and eliminates by rows of four."""
    from contactimplicitmpc.jl_amd import gains
    c, G = pgc.rollout_case(which), _blocks(which)
    nq, nu = pgc.dims(c["model"])[:2]
    T, B = G.status.shape
    Q, R, Qf, _, _ = _weights(which, T, B)
    _, tape = _tape(c)
    with tape:
        mine = tape.lqr(Q, R, Qf)
    AB = [[prc.dense_AB(G.dz[t, b], nq, nu) for t in range(T)] for b in range(B)]
    A, Bm = np.array([[ab[0] for ab in row] for row in AB]), np.array([[ab[1] for ab in row] for row in AB])
    Qh = np.broadcast_to(np.concatenate([np.broadcast_to(Q, (T,) + Q.shape), Qf[None]])[None], (B, T + 1) + Q.shape)
    K, P1 = gains.tvlqr(A, Bm, Qh, np.broadcast_to(R[None, None], (B, 1) + R.shape))
    ld, _, bound = prc.bounds(G.dz, G.status, nq, nu, Q, R, Qf)
    for key, theirs in (("K", K.transpose(1, 0, 2, 3)), ("P0", P1)):
        dist, gap = pac.distance(theirs, ld[key]), pac.distance(mine.__dict__[key], theirs)
        print(f"{which} {key}: tvlqr {dist:.2e} from lq_ld (bound {bound[key]:.2e}), lqr {gap:.2e} from tvlqr")
        assert dist <= bound[key] and pac.distance(mine.__dict__[key], ld[key]) <= bound[key]


# ---- c. a robot's rows do not depend on the robots that ride along -------------------------------------------------------------------------------
def test_each_hopper_alone_gives_its_rows():
    c = pgc.rollout_case("hopper_2D")
    T, B = 14, 3
    Q, R, Qf, q, r = _weights("hopper_2D", T, B)
    _, tape = _tape(c)
    with tape:
        whole = tape.lqr(Q, R, Qf, q=q, r=r, rho=1e-3)
    for b in range(B):
        one = dict(c, q1=c["q1"][b:b + 1], v1=c["v1"][b:b + 1], u=c["u"][:, b:b + 1], mu=c["mu"][b:b + 1])
        _, t1 = _tape(one)
        with t1:
            alone = t1.lqr(Q, R, Qf, q=q[:, b:b + 1], r=r[:, b:b + 1], rho=1e-3)
        for key in ("K", "k"):
            assert alone.__dict__[key][:, 0].tobytes() == np.ascontiguousarray(whole.__dict__[key][:, b]).tobytes(), (b, key)
        for key in ("P0", "p0", "dV"):
            assert alone.__dict__[key][0].tobytes() == whole.__dict__[key][b].tobytes(), (b, key)
    assert np.abs(whole.K).max() > 0


# ---- d. a closed-loop tape ------------------------------------------------------------------------------------------------------------------------
def test_a_closed_loop_tape_gives_the_restatement_on_its_own_blocks():
    """hopper_2D under per-robot feedback: the blocks are the plant's (u_t in θ), the tape's own gains play no part."""
    from contactimplicitmpc.jl_amd import plant
    which = "hopper_2D"
    c, f = pfc.base_case(which), pfc.feedback(which, "per_robot")
    fb = plant.Feedback(f["K"], f["x_ref"], hold=f["hold"], n_sample=f["n_sample"])
    dims = pgc.dims(c["model"])
    out = plant.rollout(*_args(c), terrain=c["terrain"], w=_w(c), diff_sol=True, grad_cols=dims[6], feedback=fb)
    G = out[7]
    T, B = G.status.shape
    Q, R, Qf, q, r = _weights(which, T, B, seed=2)
    *_, tape, fb_err = plant.rollout_tape(*_args(c), terrain=c["terrain"], w=_w(c), grad_cols=dims[6], feedback=fb)
    with tape:
        g = tape.lqr(Q, R, Qf, q=q, r=r)
    _compare("closed loop", _out(g), G.dz, G.status, dims[0], dims[1], Q, R, Qf, q=q, r=r)
    assert not np.array_equal(G.dz, _blocks(which).dz)      # the closed loop went elsewhere


# ---- e., f. cut steps, and a singular step ---------------------------------------------------------------------------------------------------------
def test_unconverged_steps_are_walked_through_and_a_singular_step_ends_a_robot_not_the_call():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    nq, nu, nc, nb = pgc.dims("hopper_2D")[:4]
    T, B = 14, 3
    Q, R, Qf, q, r = _weights("hopper_2D", T, B, seed=3)
    (ok, *_), tape = _tape(c, opts=dataclasses.replace(plant.SIM_OPTS, max_iter=1))
    D, status = np.zeros((T, B, nq + nc + nb, tape.n_cols)), np.zeros((T, B), dtype=np.int32)
    with tape:
        assert not ok and (tape.grad_status == 0).all()
        g = tape.lqr(Q, R, Qf, q=q, r=r)
        sing = tape.lqr(Q, np.zeros((nu, nu)), Qf, q=q, r=r)      # returns: the call itself succeeds
        reg = tape.lqr(Q, np.zeros((nu, nu)), Qf, q=q, r=r, rho=0.5)
    assert g.n_cut.tolist() == [14, 14, 14] and g.status.tolist() == [0, 0, 0]
    np.testing.assert_array_equal(g.K, 0.0)
    _compare("cut", _out(g), D, status, nq, nu, Q, R, Qf, q=q, r=r)
    assert np.abs(g.P0).max() > 0
    assert sing.status.tolist() == [1, 1, 1] and sing.n_cut.tolist() == [14, 14, 14]
    for a in (sing.K, sing.k, sing.P0, sing.p0, sing.dV):
        np.testing.assert_array_equal(a, 0.0)
    assert reg.status.tolist() == [0, 0, 0] and np.abs(reg.P0).max() > 0
    f64 = prc.lq_f64(D, status, nq, nu, Q, np.zeros((nu, nu)), Qf, q=q, r=r, rho=0.5)
    assert reg.P0.tobytes() == f64["P0"].tobytes() and reg.k.tobytes() == f64["k"].tobytes()


# ---- g. the gains as a Feedback ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_sample,steps", [(1, 14), (2, 5)], ids=["N_sample 1", "N_sample 2"])
def test_feedback_of_the_gains_retraces_the_trajectory_and_closes_the_loop(N_sample, steps):
    """Rolling out again under `gains.feedback(q)` from the same start: the error is exactly zero, so the trajectory is the open-loop one
    bit for bit.  On that closed-loop tape `transition()` is Π_t (A_t − B_t K_t): held to 100 x max(d(the float64 product, the longdouble
    product), 2.2e-16) per robot with the device's own K in both, which pins the sign, the layout and the N_sample scaling of
    `feedback()`."""
    from contactimplicitmpc.jl_amd import plant
    base = pgc.rollout_case("hopper_2D")
    c = dict(base, u=base["u"][:steps] * N_sample)      # nominal controls: a step applies u / N_sample
    nq, nu = pgc.dims("hopper_2D")[:2]
    *_, G = plant.rollout(*_args(c), N_sample=N_sample, diff_sol=True)
    T, B = G.status.shape
    assert T == steps * N_sample
    Q, R, Qf, _, _ = _weights("hopper_2D", T, B, seed=4)
    (ok, q, ua, gam, b, st, it), tape = _tape(c, N_sample=N_sample, grad_cols=None, w=None)
    with tape:
        g = tape.lqr(Q, R, Qf)
    fb = g.feedback(q)
    assert fb.hold == 1 and fb.n_sample == 1.0 and fb.K.shape == (T, B, nu, 2 * nq) and fb.x_ref.shape == (T, B, 2 * nq)
    np.testing.assert_array_equal(fb.K, g.K * N_sample)
    np.testing.assert_array_equal(fb.x_ref[:, :, nq:], q[1:T + 1])
    np.testing.assert_allclose(fb.x_ref[:, :, :nq], q[:T], rtol=0, atol=1e-15)
    ok2, q2, ua2, gam2, b2, st2, it2, closed, fb_err = plant.rollout_tape(*_args(c), N_sample=N_sample, feedback=fb)
    with closed:
        Phi = closed.transition()
        np.testing.assert_array_equal(closed.grad_status, tape.grad_status)
    assert ok and ok2
    np.testing.assert_array_equal(fb_err, 0.0)
    assert q2.tobytes() == q.tobytes() and gam2.tobytes() == gam.tobytes() and b2.tobytes() == b.tobytes()
    np.testing.assert_array_equal(ua2, ua)
    assert np.abs(g.K).max() > 0
    open_Phi = None
    for r in range(B):
        ld = prc.closed_loop_product(G.dz, g.K, nq, nu, r)
        f64 = np.eye(2 * nq)
        for t in range(T):
            A, Bm = prc.dense_AB(G.dz[t, r], nq, nu)
            f64 = (A - Bm @ g.K[t, r]) @ f64
        bound = pac.FACTOR * max(pac.distance(f64, ld), 2.2e-16)
        dist = pac.distance(Phi[r], ld)
        open_Phi = prc.closed_loop_product(G.dz, np.zeros_like(g.K), nq, nu, r)
        print(f"N_sample {N_sample}, robot {r}: transition {dist:.2e} from the longdouble product of A - B K (bound {bound:.2e}); "
              f"the open loop's product is {pac.distance(open_Phi, ld):.2e} away")
        assert dist <= bound
        assert pac.distance(open_Phi, ld) > 1e3 * bound      # the gains do move the product: a feedback() that applied none would fail
