"""The derivative of the clamped closed loop on the device (`Feedback(..., u_lo=, u_hi=, clamp_grad=True)` on `rollout(diff_sol=True)`,
`rollout_tape`, `RolloutTape.vjp` / `jvp` / `transition` and `rollout_torch`; plant_clamp_mask_kernel and the third
instantiations of plant_adjoint_kernel and plant_tangent_kernel) against the restatements of tests/plant_clamp_cases.py.

Cases (B <= 3, T <= 12, steps_per_launch = 2 so that a chunk boundary lies inside): hopper_2D with a schedule per robot and with K_f = 2 rows
held for 2 steps (n_sample = 4), pushbot (T = 4; nu = 2 in this project) and centroidal_quadruped_wall (two wavefronts a robot, nu = 12, B = 1,
T = 2).  The limits are those of tests/test_gpu_plant_boxqp.py's test_limited_closed_loop, built from the unlimited loop of the same call:
control 0 capped a quarter below what the law asks at step 0, control 1 finite limits one unit outside everything applied, the rest none.
Every case ASSERTS 0 < clamped bits < all bits, step 0's control 0 clamped and control 1 free throughout.

Held bit for bit: the tape call against `plant.rollout(feedback=limited)`, the mask against `plant.clamped_controls`, the blocks against the
open-loop blocks on u_applied, `vjp` and `jvp` against the ordered float64 restatements on the device's own blocks and mask (K and x_ref
after the folds), `transition()` against the 2nq unit directions, infinite limits against the unlimited closed-loop tape, `u_lo == u_hi`
against the open-loop tape on that constant control, `rollout_torch` against the tape.  Within bounds built from the restatements alone
(100 x max(d(np, ld), 2.2e-16) per output): both chains against longdouble, and `jvp` against `vjp`.  Finite differences in flight within
1e-4, the tolerance of test_gain_and_reference_gradients_match_finite_differences_in_flight (tests/test_gpu_plant_feedback.py), taken over
unchanged.  tests/README_plant_clamp.md has the figures the tests print."""
import dataclasses
import functools

import numpy as np
import pytest

import plant_adjoint_cases as pac
import plant_clamp_cases as pcc
import plant_feedback_cases as pfc
import plant_gradient_cases as pgc
import plant_tangent_cases as ptc

pytestmark = pytest.mark.gpu

NAMES = sorted(pcc.DEVICE_CASES)
PLAIN = ("q", "u_applied", "gamma", "b", "status", "iters")


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def _w(c):
    """One shared row of zero disturbances, so that the rollout has a w to take a tangent of."""
    return np.zeros((1, pgc.dims(c["model"])[4]))


def _kw(c):
    return dict(terrain=c["terrain"], w=_w(c), steps_per_launch=pcc.STEPS_PER_LAUNCH)


def _fb(f, **lim):
    from contactimplicitmpc.jl_amd import plant
    return plant.Feedback(f["K"], f["x_ref"], hold=f["hold"], n_sample=f["n_sample"], **lim)


def _same(a, b, what):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


@functools.lru_cache(maxsize=None)
def _limited(name):
    """A case under its limits, once per process: the unlimited loop the limits come from, the limited rollout without gradients, and the
    limited rollout with every column of θ differentiated (`clamp_grad=True`); every array read-only.  The conditions on the inputs are
    asserted here, for every test that uses the case."""
    from contactimplicitmpc.jl_amd import plant
    c, f = pcc.device_case(name)
    nth = pgc.dims(c["model"])[6]
    free = plant.rollout(*_args(c), feedback=_fb(f), **_kw(c))
    u_lo, u_hi = pcc.limits_from(free[2])
    roll = plant.rollout(*_args(c), feedback=_fb(f, u_lo=u_lo, u_hi=u_hi), **_kw(c))
    assert len(roll) == 8
    grad = plant.rollout(*_args(c), feedback=_fb(f, u_lo=u_lo, u_hi=u_hi, clamp_grad=True), diff_sol=True, grad_cols=nth, **_kw(c))
    assert len(grad) == 9
    ua = roll[2]
    T, B, nu = ua.shape
    mask = plant.clamped_controls(ua, u_lo, u_hi)
    fr = pcc.free_mask(mask, nu)
    bits = pcc.count_bits(mask, nu)
    print(f"{name}: {bits} of {ua.size} controls clamped, per robot {(~fr).sum(axis=(0, 2)).tolist()}; B {B}, T {T}, nu {nu}")
    assert 0 < bits < ua.size, "the case clamps nothing or everything"
    assert (~fr[0, :, 0]).all(), "control 0 of step 0 is not clamped"
    if nu >= 2:
        assert fr[:, :, 1].all(), "control 1 is not free throughout"
    assert roll[0] and grad[7].status.all()
    for a in roll[1:] + (u_lo, u_hi, mask, grad[7].dz, grad[7].status):
        a.setflags(write=False)
    return dict(c=c, f=f, free=free, u_lo=u_lo, u_hi=u_hi, roll=dict(zip(("ok",) + PLAIN + ("fb_err",), roll)), G=grad[7], grad=grad, mask=mask)


def _tape(name, **over):
    """`rollout_tape` of a case under its limits with clamp_grad=True: (the seven plain outputs, tape, fb_err)."""
    from contactimplicitmpc.jl_amd import plant
    r = _limited(name)
    c, f = r["c"], r["f"]
    kw = dict(_kw(c), grad_cols=pgc.dims(c["model"])[6], feedback=_fb(f, u_lo=r["u_lo"], u_hi=r["u_hi"], clamp_grad=True))
    kw.update(over)
    *plain, tape, fb_err = plant.rollout_tape(*_args(c), **kw)
    return plain, tape, fb_err


# ---- 1. the tape call -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_limited_tape_is_the_limited_rollout_with_its_mask_and_the_open_loop_blocks(name):
    from contactimplicitmpc.jl_amd import plant
    r = _limited(name)
    c, roll = r["c"], r["roll"]
    plain, tape, fb_err = _tape(name)
    with tape:
        assert plain[0] == roll["ok"]
        for key, a in zip(PLAIN, plain[1:]):
            _same(a, roll[key], f"{name}: {key} of the tape call against plant.rollout(feedback=limited)")
        _same(fb_err, roll["fb_err"], f"{name}: fb_err")
        assert tape.clamped.dtype == np.int32 and tape.clamped.shape == roll["status"].shape
        assert tape.clamped.tolist() == r["mask"].tolist() == pcc.clamped_words(roll["u_applied"], r["u_lo"], r["u_hi"]).tolist()
        grad_status = tape.grad_status.copy()
    # the blocks do not see the clamp: they are the open-loop blocks on the applied controls
    nth = pgc.dims(c["model"])[6]
    *_, open_tape = plant.rollout_tape(c["model"], c["q1"], c["v1"], roll["u_applied"], c["h"], c["mu"], grad_cols=nth, **_kw(c))
    with open_tape:
        assert open_tape.clamped is None
        np.testing.assert_array_equal(grad_status, open_tape.grad_status)
    *open_plain, open_G = plant.rollout(c["model"], c["q1"], c["v1"], roll["u_applied"], c["h"], c["mu"], diff_sol=True, grad_cols=nth, **_kw(c))
    _same(r["G"].dz, open_G.dz, f"{name}: the blocks of rollout(diff_sol=True, clamp_grad=True) against the open-loop blocks on u_applied")
    _same(r["G"].status, open_G.status, f"{name}: their status")
    np.testing.assert_array_equal(grad_status, open_G.status)
    for k, key in enumerate(PLAIN):      # and diff_sol=True under limits returns the limited rollout
        _same(r["grad"][k + 1], roll[key], f"{name}: {key} of rollout(diff_sol=True)")
    _same(r["grad"][8], roll["fb_err"], f"{name}: fb_err of rollout(diff_sol=True)")
    assert not np.array_equal(roll["q"], r["free"][1]), "the limits changed nothing"


# ---- 2. vjp -----------------------------------------------------------------------------------------------------------------------------------------
def _raw(cot):
    return dict(g_q0=cot.g_q0, g_q1=cot.g_q1, u_step=cot.u_step, w_step=cot.w_step, g_mu=cot.g_mu, g_h=cot.g_h, xref_step=cot.xref_step)


def _vjp_parity(name, seed=0):
    r = _limited(name)
    c, f, G = r["c"], r["f"], r["G"]
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = G.status.shape
    cots = pac.random_cotangents(np.random.default_rng(seed), T, B, nq, nc, nb)
    _, tape, fb_err = _tape(name)
    with tape:
        cot = tape.vjp(*cots)
        mask = tape.clamped.copy()
    Ks, _ = pfc.per_step(f, T, B)                                                 # N_sample = 1: the device's rows are K as it stands
    ld, f64, bound = pcc.chain_bounds(G.dz, *cots, nq, nu, nw, Ks, f["n_sample"], mask)
    for k, dev in _raw(cot).items():
        dist = pac.distance(dev, ld[k])
        print(f"{name} {k}: device {dist:.2e} from chain_ld (bound {bound[k]:.2e}), bits equal chain_f64: {dev.tobytes() == np.ascontiguousarray(f64[k]).tobytes()}")
        assert dev.tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{name} {k} differs from chain_f64"
        assert dist <= bound[k], f"{name} {k}: {dist:.3e} > {bound[k]:.3e}"
    return r, cot, cots, (ld, bound), Ks, mask, fb_err


@pytest.mark.parametrize("name", NAMES)
def test_vjp_is_the_masked_restatement_bit_for_bit_and_within_the_longdouble_bounds(name):
    r, cot, cots, _, Ks, mask, fb_err = _vjp_parity(name)
    f = r["f"]
    nu = Ks.shape[2]
    shared, K_f = np.ndim(f["K"]) == 3, f["K"].shape[0]
    assert cot.K.shape == f["K"].shape and cot.x_ref.shape == f["x_ref"].shape
    np.testing.assert_array_equal(cot.K, pfc.fold_gains(cot.u_step, fb_err, K_f, f["hold"], shared, 1))
    np.testing.assert_array_equal(cot.x_ref, pfc.fold_rows(cot.xref_step, K_f, f["hold"], shared))
    fr = pcc.free_mask(mask, nu)
    assert np.all(cot.u_step[~fr] == 0.0) and not np.signbit(cot.u_step[~fr]).any() and np.abs(cot.u_step[fr]).max() > 0
    assert np.abs(cot.K).max() > 0 and np.abs(cot.x_ref).max() > 0 and cot.n_cut.tolist() == [0] * fr.shape[1]
    # the clamp matters: the unmasked chain on the same blocks gives other numbers
    nq, _, nc, nb, nw = pgc.dims(r["c"]["model"])[:5]
    plain = pfc.chain_f64(r["G"].dz, *cots, nq, nu, nw, Ks, f["n_sample"])
    assert not np.array_equal(plain["g_q0"], cot.g_q0)


# ---- 3. jvp and transition ----------------------------------------------------------------------------------------------------------------------------
def _random_arguments(rng, c, f, n_dir=None):
    lead = () if n_dir is None else (n_dir,)
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    B = c["q1"].shape[0]
    return dict(dq1=rng.standard_normal(lead + (B, nq)), dv1=rng.standard_normal(lead + (B, nq)), du=rng.standard_normal(lead + c["u"].shape),
                dw=rng.standard_normal(lead + (1, nw)), dmu=rng.standard_normal(lead + (B,)), dK=rng.standard_normal(lead + np.shape(f["K"])),
                dx_ref=rng.standard_normal(lead + np.shape(f["x_ref"])))


def _directions(c, f, T, args, n_dir, fb_err):
    B = c["q1"].shape[0]
    pick = (lambda a, d: a) if n_dir is None else (lambda a, d: a[d])
    return [ptc.step_inputs(T, B, c["h"], c["v1"], **{k: pick(a, d) for k, a in args.items()}, fb_hold=f["hold"], fb_err=fb_err) for d in range(n_dir or 1)]


def _out(t, stacked=True):
    lift = (lambda a: a) if stacked else (lambda a: a[None])
    return dict(q=lift(t.q), gamma=lift(t.gamma), b=lift(t.b), u_applied=lift(t.u_applied))


@pytest.mark.parametrize("name", NAMES)
def test_jvp_is_the_masked_restatement_bit_for_bit_alone_and_stacked_and_transition_is_the_unit_directions(name):
    r = _limited(name)
    c, f, G = r["c"], r["f"], r["G"]
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = G.status.shape
    Ks, _ = pfc.per_step(f, T, B)
    one, many = _random_arguments(np.random.default_rng(1), c, f), _random_arguments(np.random.default_rng(2), c, f, 3)
    _, tape, fb_err = _tape(name)
    with tape:
        mask = tape.clamped.copy()
        t1, t3 = tape.jvp(**one), tape.jvp(**many)
        alone = [tape.jvp(**{k: a[d] for k, a in many.items()}) for d in range(3)]
        M = tape.transition()
        assert tape.group == 64
    targs = (nq, nu, nw, nc, Ks, f["n_sample"], mask)
    for what, got, dirs in ((f"{name} alone", _out(t1, False), _directions(c, f, T, one, None, fb_err)),
                            (f"{name} stacked", _out(t3), _directions(c, f, T, many, 3, fb_err))):
        f64 = pcc.stacked(pcc.tangent_f64, G.dz, dirs, *targs)
        ld, _, bound = pcc.tangent_bounds(G.dz, dirs[0], *targs)
        for k in pcc.TANGENT_OUTPUTS:
            dist = pac.distance(got[k][0], ld[k])
            print(f"{what} {k}: device {dist:.2e} from tangent_ld (bound {bound[k]:.2e}), bits equal tangent_f64: {got[k].tobytes() == f64[k].tobytes()}")
            assert got[k].tobytes() == np.ascontiguousarray(f64[k]).tobytes(), f"{what} {k} differs from tangent_f64"
            assert dist <= bound[k], f"{what} {k}: {dist:.3e} > {bound[k]:.3e}"
    for d in range(3):      # a direction's bits do not depend on what rides with it
        for k in pcc.TANGENT_OUTPUTS:
            assert getattr(alone[d], k).tobytes() == getattr(t3, k)[d].tobytes(), (d, k)
    fr = pcc.free_mask(mask, nu)
    assert np.all(t3.u_applied[:, ~fr] == 0.0) and not np.signbit(t3.u_applied[:, ~fr]).any() and np.abs(t3.u_applied[:, fr]).max() > 0
    assert t1.n_cut.tolist() == [0] * B
    # transition(): the 2nq unit directions of [dq0; dq1], restated
    units = [dict(dq0=np.tile(np.eye(2 * nq)[i, :nq], (B, 1)), dq1=np.tile(np.eye(2 * nq)[i, nq:], (B, 1))) for i in range(2 * nq)]
    want = pcc.stacked(pcc.tangent_f64, G.dz, units, *targs)["q"]
    _same(M, np.concatenate([want[:, T], want[:, T + 1]], axis=2).transpose(1, 2, 0), f"{name}: transition() against the unit directions")
    assert M.shape == (B, 2 * nq, 2 * nq)


# ---- 4. duality on the device ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_jvp_and_vjp_are_adjoint_within_their_bounds(name):
    """⟨g, jvp(δ)⟩ = ⟨vjp(g), δ⟩ in the chains' own per-step terms (δK meets u_step through δK e), both sides from the device, held to the sum
    of what the two chains' longdouble bounds allow their inner products (`plant_clamp_cases.duality`)."""
    r, cot, cots, (ld, bound), Ks, mask, fb_err = _vjp_parity(name, seed=4)
    c, f, G = r["c"], r["f"], r["G"]
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = G.status.shape
    args = _random_arguments(np.random.default_rng(3), c, f)
    _, tape, _ = _tape(name)
    with tape:
        tan = tape.jvp(**args)
    d = _directions(c, f, T, args, None, fb_err)[0]
    tld, _, tbound = pcc.tangent_bounds(G.dz, d, nq, nu, nw, nc, Ks, f["n_sample"], mask)
    lhs, rhs, allowed = pcc.duality(cots, dict(q=tan.q, gamma=tan.gamma, b=tan.b), _raw(cot), d, tld, tbound, ld, bound)
    print(f"{name}: <g, jvp(d)> = {float(lhs):.12e}, <vjp(g), d> = {float(rhs):.12e}, difference {float(abs(lhs - rhs)):.2e} (allowed {allowed:.2e})")
    assert float(abs(lhs - rhs)) <= allowed
    # and in the caller's terms: the folds are the transposes of the spreads
    L = pac.LD
    rhs2 = sum((np.asarray(a, L) * np.asarray(args[k], L).reshape(np.shape(a))).sum()
               for a, k in ((cot.q1, "dq1"), (cot.v1, "dv1"), (cot.u, "du"), (cot.w, "dw"), (cot.mu, "dmu"), (cot.K, "dK"), (cot.x_ref, "dx_ref")))
    print(f"{name}: in the caller's arguments <vjp(g), d> = {float(rhs2):.12e}, difference {float(abs(lhs - rhs2)):.2e}")
    assert float(abs(lhs - rhs2)) <= allowed


# ---- 5. infinite limits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_infinite_limits_give_the_unlimited_tapes_bits_and_an_empty_mask(name):
    from contactimplicitmpc.jl_amd import plant
    r = _limited(name)
    c, f = r["c"], r["f"]
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = r["mask"].shape
    cots = pac.random_cotangents(np.random.default_rng(5), T, B, nq, nc, nb)
    args = _random_arguments(np.random.default_rng(6), c, f, 2)
    wide, tape, fb_err = _tape(name, feedback=_fb(f, u_lo=np.full(nu, -np.inf), u_hi=np.full(nu, np.inf), clamp_grad=True))
    with tape:
        assert tape.clamped.tolist() == np.zeros((T, B), dtype=int).tolist()
        cot, tan = tape.vjp(*cots), tape.jvp(**args)
    *plain, free_tape, free_err = plant.rollout_tape(*_args(c), grad_cols=pgc.dims(c["model"])[6], feedback=_fb(f), **_kw(c))
    with free_tape:
        assert free_tape.clamped is None
        cot0, tan0 = free_tape.vjp(*cots), free_tape.jvp(**args)
    for a, b in zip(wide[1:], plain[1:]):
        _same(a, b, f"{name}: the rollout under infinite limits")
    _same(fb_err, free_err, name)
    for k, a in _raw(cot).items():
        _same(a, _raw(cot0)[k], f"{name}: vjp {k} under infinite limits")
    _same(cot.K, cot0.K, name); _same(cot.x_ref, cot0.x_ref, name); _same(cot.u, cot0.u, name)
    for k in pcc.TANGENT_OUTPUTS:
        _same(getattr(tan, k), getattr(tan0, k), f"{name}: jvp {k} under infinite limits")


# ---- 6. u_lo == u_hi ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_equal_limits_clamp_everything_and_leave_the_open_loop_chain(name):
    from contactimplicitmpc.jl_amd import plant
    r = _limited(name)
    c, f = r["c"], r["f"]
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    T, B = r["mask"].shape
    const = np.ascontiguousarray(r["free"][2].mean(axis=0))                                      # (B, nu): every robot's controls held there
    cots = pac.random_cotangents(np.random.default_rng(7), T, B, nq, nc, nb)
    _, tape, _ = _tape(name, feedback=_fb(f, u_lo=const, u_hi=const, clamp_grad=True))
    with tape:
        assert tape.clamped.tolist() == np.full((T, B), (1 << nu) - 1).tolist()
        cot = tape.vjp(*cots)
        tan = tape.jvp(**_random_arguments(np.random.default_rng(8), c, f))
    for a in (cot.K, cot.x_ref, cot.u, cot.u_step, cot.xref_step, tan.u_applied):
        assert np.all(a == 0.0)
    held = np.ascontiguousarray(np.broadcast_to(const, (T, B, nu)))
    *_, open_tape = plant.rollout_tape(c["model"], c["q1"], c["v1"], held, c["h"], c["mu"], grad_cols=pgc.dims(c["model"])[6], **_kw(c))
    with open_tape:
        cot0 = open_tape.vjp(*cots)
    _same(cot.g_q0, cot0.g_q0, f"{name}: g_q0 against the open-loop tape on the constant control")
    _same(cot.g_q1, cot0.g_q1, f"{name}: g_q1 against the open-loop tape on the constant control")
    assert cot.n_cut.tolist() == cot0.n_cut.tolist()


# ---- 7. finite differences of the limited device rollout, in flight -------------------------------------------------------------------------------------
def test_gain_and_reference_gradients_match_finite_differences_in_flight_under_limits():
    """test_gain_and_reference_gradients_match_finite_differences_in_flight of tests/test_gpu_plant_feedback.py under limits: hopper_2D steps
    0-3 (before the impact, where the step is smooth), robots 0 and 2, ε = 1e-5, central differences of the limited closed-loop
    `plant.rollout`, a loss linear in (q, γ, b), a random direction in K and in x_ref, relative difference <= 1e-4.  Control 0 is capped below
    everything the unlimited law asks for, by a quarter of its size, so that it is clamped at all four steps; control 1 has limits one unit
    outside.  The masks of the ±ε rollouts are asserted equal to the base mask, so no difference straddles the kink."""
    from contactimplicitmpc.jl_amd import plant
    T, eps = 4, 1e-5
    base, f = pfc.base_case("hopper_2D"), pfc.feedback("hopper_2D", "per_robot")
    nq, nu, nc, nb = pgc.dims("hopper_2D")[:4]
    K, xr = f["K"][:T], f["x_ref"][:T]
    args = (base["model"], base["q1"], base["v1"], base["u"][:T], base["h"], base["mu"])
    ua0 = plant.rollout(*args, feedback=plant.Feedback(K, xr, n_sample=f["n_sample"]))[2]
    u_lo, u_hi = np.full((3, nu), -np.inf), np.full((3, nu), np.inf)
    u_hi[:, 0] = ua0[:, :, 0].min(axis=0) - 0.25 * (np.abs(ua0[:, :, 0]).max(axis=0) + 1e-3)
    u_lo[:, 1], u_hi[:, 1] = ua0[:, :, 1].min(axis=0) - 1.0, ua0[:, :, 1].max(axis=0) + 1.0
    fb = lambda K_, x_, **kw: plant.Feedback(K_, x_, n_sample=f["n_sample"], u_lo=u_lo, u_hi=u_hi, **kw)
    want_mask = np.full((T, 3), 1, dtype=np.int32)                                # control 0 clamped, control 1 free, at all four steps
    for robot in (0, 2):
        rng = np.random.default_rng(100 + robot)
        gq, gg, gb = np.zeros((T + 2, 3, nq)), np.zeros((T, 3, nc)), np.zeros((T, 3, nb))
        gq[:, robot], gg[:, robot], gb[:, robot] = [g[:, 0] for g in pac.random_cotangents(rng, T, 1, nq, nc, nb)]
        dK, dx = np.zeros(K.shape), np.zeros(xr.shape)
        dK[:, robot], dx[:, robot] = rng.standard_normal(K.shape[2:]), rng.standard_normal(xr.shape[2:])
        *_, tape, _ = plant.rollout_tape(*args, feedback=fb(K, xr, clamp_grad=True))
        with tape:
            assert tape.clamped.tolist() == want_mask.tolist()
            cot = tape.vjp(gq, gg, gb)
        assert cot.n_cut.tolist() == [0, 0, 0]
        *_, free_tape, _ = plant.rollout_tape(*args, feedback=plant.Feedback(K, xr, n_sample=f["n_sample"]))
        with free_tape:
            free_cot = free_tape.vjp(gq, gg, gb)

        def loss(sK, sx):
            ok, q, ua, gam, b, st, it, e = plant.rollout(*args, feedback=fb(K + sK * dK, xr + sx * dx))
            assert ok
            assert plant.clamped_controls(ua, u_lo, u_hi).tolist() == want_mask.tolist(), "a perturbed rollout crossed the kink"
            return float((gq * q).sum() + (gg * gam).sum() + (gb * b).sum())
        for what, adj, free_adj, fd in (("K", float((cot.K * dK).sum()), float((free_cot.K * dK).sum()), (loss(eps, 0.0) - loss(-eps, 0.0)) / (2 * eps)),
                                        ("x_ref", float((cot.x_ref * dx).sum()), float((free_cot.x_ref * dx).sum()), (loss(0.0, eps) - loss(0.0, -eps)) / (2 * eps))):
            rel = abs(fd - adj) / max(abs(fd), abs(adj))
            rel_free = abs(fd - free_adj) / max(abs(fd), abs(free_adj))
            print(f"robot {robot} d/d{what}: limited chain {adj:.9e}, central differences of the limited rollout {fd:.9e}, relative difference {rel:.2e}; "
                  f"the unlimited tape's {free_adj:.9e} is {rel_free:.2e} away")
            assert rel <= 1e-4
            assert free_adj != adj, "the clamp does not matter here"
        assert not np.array_equal(cot.K, free_cot.K) and np.all(cot.K[:, robot, 0] == 0.0)


# ---- 8. torch ----------------------------------------------------------------------------------------------------------------------------------------------
def test_rollout_torch_differentiates_the_clamped_loop_in_both_modes():
    import torch
    import torch.autograd.forward_ad as fwAD
    from contactimplicitmpc.jl_amd import plant
    name = "hopper_2D-held"
    r = _limited(name)
    c, f = r["c"], r["f"]
    T, B = r["mask"].shape
    lim = dict(u_lo=r["u_lo"], u_hi=r["u_hi"], clamp_grad=True)
    kw = dict(terrain=c["terrain"], steps_per_launch=pcc.STEPS_PER_LAUNCH)
    leaf = lambda a: torch.tensor(np.array(a), dtype=torch.float64, requires_grad=True)
    K, xr, u = leaf(f["K"]), leaf(f["x_ref"]), leaf(c["u"])
    q, gamma, b, status = plant.rollout_torch(c["model"], c["q1"], c["v1"], u, c["h"], c["mu"],
                                              feedback=plant.Feedback(K, xr, hold=f["hold"], n_sample=f["n_sample"], **lim), **kw)
    rng = np.random.default_rng(5)
    cw, dw = rng.standard_normal((B, 4)), rng.standard_normal((T, B, 1))
    ((q[-1] * torch.tensor(cw)).sum() + (gamma * torch.tensor(dw)).sum()).backward()
    *plain, tape, fb_err = plant.rollout_tape(*_args(c), feedback=_fb(f, **lim), **kw)
    gq = np.zeros((T + 2, B, 4))
    gq[-1] = cw
    dK, dx = rng.standard_normal(f["K"].shape), rng.standard_normal(f["x_ref"].shape)
    with tape:
        assert tape.clamped.tolist() == plant.clamped_controls(plain[2], r["u_lo"], r["u_hi"]).tolist() and 0 < pcc.count_bits(tape.clamped, 2) < 2 * T * B
        cot = tape.vjp(gq=gq, ggamma=dw)
        tan = tape.jvp(dK=dK, dx_ref=dx)
    _same(q.detach().numpy(), plain[1], "q of rollout_torch")
    for got, want, what in ((K.grad, cot.K, "K.grad"), (xr.grad, cot.x_ref, "x_ref.grad"), (u.grad, cot.u, "u.grad")):
        _same(got.numpy(), want, what)
    assert np.abs(cot.K).max() > 0 and np.abs(cot.x_ref).max() > 0
    with fwAD.dual_level():
        Kd, xd = fwAD.make_dual(torch.tensor(np.array(f["K"])), torch.tensor(dK)), fwAD.make_dual(torch.tensor(np.array(f["x_ref"])), torch.tensor(dx))
        q2, g2, b2, _ = plant.rollout_torch(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"],
                                            feedback=plant.Feedback(Kd, xd, hold=f["hold"], n_sample=f["n_sample"], **lim), **kw)
        tq, tg, tb = (fwAD.unpack_dual(a).tangent.numpy() for a in (q2, g2, b2))
    _same(tq, tan.q, "the forward_ad tangent of q"); _same(tg, tan.gamma, "of gamma"); _same(tb, tan.b, "of b")
    assert np.abs(tan.q).max() > 0


# ---- 9. cut steps ------------------------------------------------------------------------------------------------------------------------------------------
def test_unconverged_steps_on_a_limited_tape_are_counted_and_nothing_flows_through_them():
    from contactimplicitmpc.jl_amd import plant
    name = "hopper_2D-per_robot"
    r = _limited(name)
    T, B = r["mask"].shape
    (ok, q, ua, gam, b, st, it), tape, fb_err = _tape(name, opts=dataclasses.replace(plant.SIM_OPTS, max_iter=1))
    gq, gg, gb = pac.random_cotangents(np.random.default_rng(0), T, B, 4, 1, 2)
    with tape:
        assert tape.clamped.tolist() == plant.clamped_controls(ua, r["u_lo"], r["u_hi"]).tolist()
        cot = tape.vjp(gq, gg, gb)
        tan = tape.jvp(dq1=np.ones((B, 4)), dK=np.ones(r["f"]["K"].shape))
        assert (tape.grad_status == 0).all()
    assert not ok and (st == 0).all() and np.isfinite(q).all() and np.isfinite(ua).all()      # the rollout goes on
    assert cot.n_cut.tolist() == [T] * B and tan.n_cut.tolist() == [T] * B
    for a in (cot.xref_step, cot.u_step, cot.K, cot.x_ref, tan.q[2:]):
        np.testing.assert_array_equal(a, 0.0)
    np.testing.assert_array_equal(cot.g_q0, gq[0])
    np.testing.assert_array_equal(cot.g_q1, gq[1])
