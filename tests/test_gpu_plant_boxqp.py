"""Control-limited iLQR on the device: the limited LQ backward pass (csrc/plant_riccati.hip:
`RolloutTape.lqr(u_lo=, u_hi=, u_nom=)`, a rho per robot, `TapeGains.clamped`), the limited closed loop (`Feedback(u_lo=, u_hi=)`, the third
state of plant_step_kernel), the limited line search (`linesearch(u_lo=, u_hi=)`) and `plant.ilqr(u_lo=, u_hi=)`, on real tapes and rollouts.
Shapes: `plant_gradient_cases.ROLLOUTS` (hopper_2D B 3 T 14 with per-robot friction, particle B 1 T 14, quadruped B 2 T 6,
centroidal_quadruped_wall B 1 T 2) and, for the closed loop, also pushbot B 2 T 4 and hopper_3D on its 3-D terrain B 1 T 4, so that each of
the six step instantiations runs the limited law once; hopper_2D there on a terrain per robot.

  1. `lqr` with limits: every output bit for bit what csrc/plant_boxqp.h gives on the host (tests/native/plant_boxqp_check.cpp, a team of
     one, on the blocks `rollout(diff_sol=True)` returns); with infinite limits bit for bit `lqr` without them; a rho array equals the
     scalar calls row by row
  2. what the entry refuses once it has a tape, each by its own reason, and a good call afterwards is unharmed
  3. the limited `rollout(feedback=)`: inside the box, on it and strictly inside it; the restated law on the returned fb_err; the open-loop
     rollout of the returned u_applied; infinite limits are the unlimited loop
  4. the limited `linesearch`: each candidate is the limited `rollout` on B robots; alpha = 0 retraces the parent; the new tape is
     `rollout_tape`'s of the chosen controls; infinite limits are the line search without limits
  5. `ilqr` with limits through contact on the hoppers, and in flight within 10 x the CPU restatement's figure

Every comparison is guarded: per robot 0 < clamped (step, control) pairs < T nu, so a case in which nothing or everything clamps fails.
For 1 and 2 the limits are placed from the unlimited pass of the same tape: control 0 gets an upper limit half a |k| below what the
unlimited pass asks for at the last step, control 1 a lower limit half a |k| above; the other controls have none (±inf beside finite
limits).  At the first step walked the unlimited optimum then lies outside the box, so that step clamps; the controls without limits never
do.  Measured figures: tests/README_plant_boxqp.md."""
import functools
import shutil
import subprocess

import numpy as np
import pytest

import plant_boxqp_cases as pbc
import plant_feedback_cases as pfc
import plant_gradient_cases as pgc
import plant_riccati_cases as prc
import test_plant_boxqp as tpb

pytestmark = pytest.mark.gpu
KEYS = prc.OUTPUTS


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def _w(c):
    return np.zeros((1, pgc.dims(c["model"])[4]))


@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("boxqp_gpu") / "plant_boxqp_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, tpb.SRC])
    return exe


@functools.lru_cache(maxsize=None)
def _parent(which):
    """A case's tape (left open), its blocks, its applied controls, weights, and limits placed from its unlimited pass; once per process."""
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case(which)
    nq, nu = pgc.dims(c["model"])[:2]
    nth = pgc.dims(c["model"])[6]
    *_, G = plant.rollout(*_args(c), terrain=c["terrain"], w=_w(c), diff_sol=True, grad_cols=nth)
    ok, q, ua, gamma, b, status, iters, tape = plant.rollout_tape(*_args(c), terrain=c["terrain"], w=_w(c), grad_cols=nth)
    T, B = ua.shape[:2]
    rng = np.random.default_rng([9, nq, nu, T])
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step=which == "particle")
    lq, lr = rng.standard_normal((T + 1, B, 2 * nq)), rng.standard_normal((T, B, nu))
    rho = 1e-3 * (1.0 + np.arange(B))
    free = tape.lqr(Q, R, Qf, q=lq, r=lr, rho=float(rho[0]))
    assert free.status.tolist() == [0] * B and free.clamped is None
    u_lo, u_hi = np.full((B, nu), -np.inf), np.full((B, nu), np.inf)
    want = ua[T - 1] + free.k[T - 1]                                     # (B, nu): what the unlimited pass asks for at the last step
    u_hi[:, 0] = want[:, 0] - 0.5 * np.abs(free.k[T - 1, :, 0])
    u_lo[:, 1] = want[:, 1] + 0.5 * np.abs(free.k[T - 1, :, 1])
    for a in (G.dz, G.status, ua, lq, lr, u_lo, u_hi):
        a.setflags(write=False)
    return dict(c=c, tape=tape, D=G.dz, status=G.status, ua=ua, nq=nq, nu=nu, Q=Q, R=R, Qf=Qf, lq=lq, lr=lr, rho=rho, u_lo=u_lo, u_hi=u_hi)


def _out(g):
    return dict(K=g.K, k=g.k, P0=g.P0, p0=g.p0, dV=g.dV, status=g.status, n_cut=g.n_cut, clamped=g.clamped)


def _same(a, b, what):
    assert a.shape == b.shape, what
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what} differs"


# ---- 1. the limited pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_limited_lqr_is_the_host_headers_bit_for_bit(which, host_chain):
    p = _parent(which)
    tape, nu = p["tape"], p["nu"]
    T, B = p["ua"].shape[:2]
    np.testing.assert_array_equal(tape.grad_status, p["status"])
    got = tape.lqr(p["Q"], p["R"], p["Qf"], q=p["lq"], r=p["lr"], rho=p["rho"], u_lo=p["u_lo"], u_hi=p["u_hi"], u_nom=p["ua"])
    assert got.clamped.shape == (T, B) and got.status.tolist() == [0] * B
    tpb.assert_some_but_not_all_clamp(got.clamped, nu, which)
    host = tpb.run_host(host_chain, p["D"], p["status"], p["nq"], nu, p["Q"], p["R"], p["Qf"], p["lq"], p["lr"], rho=p["rho"], u_lo=p["u_lo"],
                        u_hi=p["u_hi"], u_nom=p["ua"])
    tpb.assert_bitwise(_out(got), host, which)
    # what the outputs must be whatever computed them: inside the box exactly, zero rows of K where clamped, on a bound there
    lo, hi = p["u_lo"][None] - p["ua"], p["u_hi"][None] - p["ua"]
    c = (got.clamped[:, :, None] >> np.arange(nu)) & 1 == 1
    assert np.all(got.k >= lo) and np.all(got.k <= hi)
    assert not got.K[c].any() and np.all((got.k[c] == lo[c]) | (got.k[c] == hi[c]))
    keep = tape.lqr(p["Q"], p["R"], p["Qf"], q=p["lq"], r=p["lr"], rho=p["rho"], u_lo=p["u_lo"], u_hi=p["u_hi"], u_nom=p["ua"], keep=1)
    _same(keep.K, got.K[:1], f"{which}: K with keep 1")
    _same(keep.clamped, got.clamped[:1], f"{which}: clamped with keep 1")
    _same(keep.P0, got.P0, f"{which}: P0 with keep 1")


@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_infinite_limits_are_the_unlimited_pass_and_a_rho_array_is_the_scalar_calls(which):
    p = _parent(which)
    tape, nu = p["tape"], p["nu"]
    T, B = p["ua"].shape[:2]
    args, kw = (p["Q"], p["R"], p["Qf"]), dict(q=p["lq"], r=p["lr"])
    inf = np.full(nu, np.inf)
    limited = tape.lqr(*args, **kw, rho=p["rho"], u_lo=p["u_lo"], u_hi=p["u_hi"], u_nom=p["ua"])
    tpb.assert_some_but_not_all_clamp(limited.clamped, nu, which)
    array_free = tape.lqr(*args, **kw, rho=p["rho"])                     # a rho array, no limits: the limited entry
    assert array_free.clamped is not None and not array_free.clamped.any()
    for b in range(B):
        rho = float(p["rho"][b])
        plain = tape.lqr(*args, **kw, rho=rho)                          # the existing entry
        open_box = tape.lqr(*args, **kw, rho=rho, u_lo=-inf, u_hi=inf, u_nom=p["ua"])
        scalar = tape.lqr(*args, **kw, rho=rho, u_lo=p["u_lo"], u_hi=p["u_hi"], u_nom=p["ua"])
        assert plain.clamped is None and not open_box.clamped.any()
        for key in KEYS:
            _same(getattr(open_box, key), getattr(plain, key), f"{which}, rho {rho}: {key} under infinite limits")
            cut = (lambda a: a[:, b]) if key in ("K", "k") else (lambda a: a[b])
            _same(cut(getattr(array_free, key)), cut(getattr(plain, key)), f"{which} robot {b}: {key} of the rho array without limits")
            _same(cut(getattr(limited, key)), cut(getattr(scalar, key)), f"{which} robot {b}: {key} of the rho array with limits")
        assert open_box.status.tolist() == plain.status.tolist() and open_box.n_cut.tolist() == plain.n_cut.tolist()
        assert limited.clamped[:, b].tolist() == scalar.clamped[:, b].tolist() and limited.status[b] == scalar.status[b]
    if B > 1:
        assert limited.K[:, 0].tobytes() != tape.lqr(*args, **kw, rho=float(p["rho"][1]), u_lo=p["u_lo"], u_hi=p["u_hi"], u_nom=p["ua"]).K[:, 0].tobytes()


# ---- 2. refusals behind a real tape ------------------------------------------------------------------------------------------------------------
def test_the_entry_refuses_what_needs_a_tape_to_see_and_a_good_call_is_unharmed():
    p = _parent("hopper_2D")
    tape, nu = p["tape"], p["nu"]
    T, B = p["ua"].shape[:2]
    args, kw = (p["Q"], p["R"], p["Qf"]), dict(q=p["lq"], r=p["lr"])
    good = dict(rho=p["rho"], u_lo=p["u_lo"], u_hi=p["u_hi"], u_nom=p["ua"])
    before = tape.lqr(*args, **kw, **good)

    def poisoned(a, at, v=np.nan):
        a = np.array(a)
        a[at] = v
        return a
    calls = {"u_lo above u_hi": dict(good, u_lo=poisoned(p["u_lo"], (1, 0), 1e9)),
             "a NaN limit": dict(good, u_hi=poisoned(p["u_hi"], (2, 1))),
             "a non-finite entry of u_nom": dict(good, u_nom=poisoned(p["ua"], (13, 2, 1))),
             "a rho that is negative or not finite": dict(good, rho=poisoned(p["rho"], 1, -1.0))}
    for reason, call in calls.items():
        with pytest.raises(ValueError) as err:
            tape.lqr(*args, **kw, **call)
        assert str(err.value) == "cimpc_plant_tape_lqr_box: " + reason
    for bad, match in ((dict(good, rho=np.zeros(B + 1)), "rho must be"), (dict(good, u_lo=p["u_lo"][:2], u_hi=p["u_hi"][:2]), "u_lo and u_hi must be"),
                       (dict(good, u_nom=None), "go together")):
        with pytest.raises(ValueError, match=match):
            tape.lqr(*args, **kw, **bad)
    with pytest.raises(ValueError, match="linear terms"):
        tape.lqr(*args, **good)
    after = tape.lqr(*args, **kw, **good)
    tpb.assert_some_but_not_all_clamp(after.clamped, nu, "after the refusals")
    tpb.assert_bitwise(_out(after), _out(before), "after the refusals")


# ---- 3. the limited closed loop: every step instantiation once -----------------------------------------------------------------------------------
LOOPS = ("hopper_2D", "particle", "quadruped", "centroidal_quadruped_wall", "pushbot", "hopper_3D")


@functools.lru_cache(maxsize=None)
def _loop_case(which):
    """(case, feedback dict, terrain) of `plant_feedback_cases` at the sizes of this file: hopper_2D B 3 T 14 with per-robot friction and a
    terrain per robot, particle B 1 T 14, quadruped B 2 T 6, centroidal_quadruped_wall B 1 T 2, pushbot B 2 T 4, hopper_3D on its 3-D
    terrain B 1 T 4; the per-robot schedule (n_sample = 4)."""
    c, f = dict(pfc.base_case(which)), dict(pfc.feedback(which, "per_robot"))
    if which == "pushbot":
        c.update(u=c["u"][:4], T=4)
        f.update(K=f["K"][:4], x_ref=f["x_ref"][:4])
    if which == "hopper_3D":
        c.update(q1=c["q1"][:1], v1=c["v1"][:1], u=c["u"][:, :1], mu=c["mu"][:1])
        f.update(K=f["K"][:, :1], x_ref=f["x_ref"][:, :1])
    terrain = ["flat_2D_lc", "sine3_2D_lc", "sine1_2D_lc"] if which == "hopper_2D" else c["terrain"]
    return c, f, terrain


def _limited_law(f, fb_err, ubar, u_lo, u_hi):
    """limit(ubar + sum_j K[:, j] e[j]) on the returned errors, in the stated order."""
    T, B = ubar.shape[:2]
    Ks, _ = pfc.per_step(f, T, B)
    u = np.zeros(ubar.shape)
    for t in range(T):
        for b in range(B):
            s = np.zeros(ubar.shape[2])
            for j in range(fb_err.shape[2]):
                s = s + Ks[t, b][:, j] * fb_err[t, b, j]
            u[t, b] = pbc.limit(ubar[t, b] + s, u_lo[b], u_hi[b])
    return u


@pytest.mark.parametrize("which", LOOPS)
def test_limited_closed_loop(which):
    """Limits from the unlimited closed loop of the same call: control 0 may not exceed a quarter below what the law asks for at step 0 (so
    step 0 is on that bound), control 1 has finite limits one unit outside everything the unlimited loop applied, the rest none."""
    from contactimplicitmpc.jl_amd import plant
    c, f, terrain = _loop_case(which)
    args, kw = _args(c), dict(terrain=terrain, steps_per_launch=pfc.STEPS_PER_LAUNCH)
    fb = lambda **lim: plant.Feedback(f["K"], f["x_ref"], hold=f["hold"], n_sample=f["n_sample"], **lim)
    free = plant.rollout(*args, feedback=fb(), **kw)
    ua0 = free[2]
    T, B, nu = ua0.shape
    u_lo, u_hi = np.full((B, nu), -np.inf), np.full((B, nu), np.inf)
    u_hi[:, 0] = ua0[0, :, 0] - 0.25 * (np.abs(ua0[0, :, 0]) + 1e-3)
    u_lo[:, 1], u_hi[:, 1] = ua0[:, :, 1].min(axis=0) - 1.0, ua0[:, :, 1].max(axis=0) + 1.0
    ok, q, ua, gamma, b, status, iters, fb_err = plant.rollout(*args, feedback=fb(u_lo=u_lo, u_hi=u_hi), **kw)
    on_bound = (ua == u_lo[None]) | (ua == u_hi[None])
    inside = (ua > u_lo[None]) & (ua < u_hi[None]) & np.isfinite(u_lo[None]) & np.isfinite(u_hi[None])
    print(f"{which}: {int(on_bound.sum())} of {ua.size} applied controls on a bound, {int(inside.sum())} strictly inside finite limits")
    assert np.all(ua >= u_lo[None]) and np.all(ua <= u_hi[None])
    assert on_bound[0, :, 0].all() and 0 < on_bound.sum() < ua.size and inside.sum() > 0
    ubar = np.broadcast_to(c["u"], (T, B, nu))
    _same(ua, _limited_law(f, fb_err, ubar, u_lo, u_hi), f"{which}: u_applied against the limited law on the returned fb_err")
    _, e = pfc.law_on(q, ubar, f)
    _same(fb_err, e, f"{which}: fb_err against the law on the returned trajectory")
    replay = plant.rollout(c["model"], c["q1"], c["v1"], ua, c["h"], c["mu"], terrain=terrain, steps_per_launch=pfc.STEPS_PER_LAUNCH)
    for name, got, ref in (("q", q, replay[1]), ("gamma", gamma, replay[3]), ("b", b, replay[4]), ("status", status, replay[5]), ("iters", iters, replay[6])):
        _same(got, ref, f"{which}: {name} against the open-loop rollout of u_applied")
    assert not np.array_equal(q, free[1]), "the limits changed nothing"
    wide = plant.rollout(*args, feedback=fb(u_lo=np.full(nu, -np.inf), u_hi=np.full(nu, np.inf)), **kw)
    assert len(wide) == len(free) == 8
    for k in range(1, 8):
        _same(wide[k], free[k], f"{which}: output {k} under infinite limits")


# ---- 4. the limited line search ------------------------------------------------------------------------------------------------------------------
ALPHAS = (1.0, 0.3, 0.0)


def _kw(which):
    c = pgc.rollout_case(which)
    return dict(terrain=c["terrain"], w=_w(c), grad_cols=pgc.dims(c["model"])[6])


@functools.lru_cache(maxsize=None)
def _ls_parent(which):
    """The nominal of a case with a tracking cost, and limits that hold the nominal's controls and cut into the unlimited full step: for
    every control but the last the limit lies halfway between the nominal's extreme and the extreme the unlimited pass asks for, on whichever side
    the pass pushes further; the last control has none."""
    from contactimplicitmpc.jl_amd import plant
    p = _parent(which)
    c, tape, ua, nq, nu = p["c"], p["tape"], p["ua"], p["nq"], p["nu"]
    ok, q, ua2, gamma, b, status, iters = plant.rollout(*_args(c), terrain=c["terrain"], w=_w(c))
    assert ua2.tobytes() == ua.tobytes()
    T, B = ua.shape[:2]
    rng = np.random.default_rng([7, nq, nu, T])
    x = np.concatenate([q[:-1], q[1:]], axis=2)
    cost = plant.TrackingCost(p["Q"], p["R"], p["Qf"], x_goal=x + 0.02 * rng.standard_normal(x.shape), u_goal=ua * 0.5)
    J, lq, lr = cost.evaluate(q, ua)
    free = tape.lqr(p["Q"], p["R"], p["Qf"], q=lq, r=lr, rho=1e-3)
    want = ua + free.k
    u_lo, u_hi = np.full((B, nu), -np.inf), np.full((B, nu), np.inf)
    for i in range(nu - 1):              # the last control keeps none
        up, down = want[:, :, i].max(axis=0) - ua[:, :, i].max(axis=0), ua[:, :, i].min(axis=0) - want[:, :, i].min(axis=0)
        hi_side, lo_side = (up >= down) & (up > 0), (down > up) & (down > 0)      # neither: the pass pulls this control inwards, no limit
        u_hi[hi_side, i] = (ua[:, :, i].max(axis=0) + 0.5 * up)[hi_side]
        u_lo[lo_side, i] = (ua[:, :, i].min(axis=0) - 0.5 * down)[lo_side]
    assert np.all(ua >= u_lo[None]) and np.all(ua <= u_hi[None])
    assert (np.isfinite(u_lo) | np.isfinite(u_hi)).any(axis=1).all(), "a robot without a limit"
    gains = tape.lqr(p["Q"], p["R"], p["Qf"], q=lq, r=lr, rho=1e-3, u_lo=u_lo, u_hi=u_hi, u_nom=ua)
    assert gains.status.tolist() == [0] * B
    return dict(p, q=q, gamma=gamma, b=b, status=status, iters=iters, cost=cost, J=J, lq=lq, lr=lr, gains=gains, free=free, lo=u_lo, hi=u_hi)


def _tape_answers(tape, p, lq, lr, seed=0):
    nq, nu, nc, nb = pgc.dims(tape.model)[:4]
    rng = np.random.default_rng([seed, tape.T, tape.B])
    g = tape.lqr(p["Q"], p["R"], p["Qf"], q=lq, r=lr, rho=1e-3)
    v = tape.vjp(gq=rng.standard_normal((tape.T + 2, tape.B, nq)), ggamma=rng.standard_normal((tape.T, tape.B, nc)), gb=rng.standard_normal((tape.T, tape.B, nb)))
    return dict(K=g.K, k=g.k, P0=g.P0, p0=g.p0, dV=g.dV, g_q0=v.g_q0, g_q1=v.g_q1, u_step=v.u_step, grad_status=tape.grad_status)


@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_limited_linesearch(which):
    import dataclasses
    from contactimplicitmpc.jl_amd import plant
    p = _ls_parent(which)
    c, tape, gains, cost, ua, q = p["c"], p["tape"], p["gains"], p["cost"], p["ua"], p["q"]
    T, B, nu = ua.shape
    lim = dict(u_lo=p["lo"], u_hi=p["hi"])
    tpb.assert_some_but_not_all_clamp(gains.clamped, nu, which)
    open_door = np.full(B, np.inf)
    with_all = tape.linesearch(gains, q, ua, cost, open_door, ALPHAS, **lim)
    with_all.tape.close()
    fb = dataclasses.replace(gains.feedback(q), **lim)
    saturated = 0
    for ci, a in enumerate(ALPHAS):      # a. each candidate is the limited closed loop on B robots
        one = tape.linesearch(gains, q, ua, cost, open_door, (a,), **lim)
        one.tape.close()
        ubar = pbc.limit(ua + a * gains.k, p["lo"][None], p["hi"][None])
        ok, rq, rua, rg, rb, rst, rit, fb_err = plant.rollout(c["model"], c["q1"], c["v1"], ubar, c["h"], c["mu"], feedback=fb, terrain=c["terrain"], w=_w(c))
        assert rst.all() and one.choice.tolist() == [0] * B, "every candidate of these cases converges"
        _same(one.J[0], cost.evaluate(rq, rua)[0], f"{which} alpha {a}: J")
        _same(with_all.J[ci], one.J[0], f"{which} alpha {a}: J of the three-alpha call")
        for name, got, ref in (("q", one.q, rq), ("u_applied", one.u_applied, rua), ("gamma", one.gamma, rg), ("b", one.b, rb), ("status", one.status, rst),
                               ("iters", one.iters, rit)):
            _same(got, ref, f"{which} alpha {a}: {name}")
        assert np.all(one.u_applied >= p["lo"][None]) and np.all(one.u_applied <= p["hi"][None])
        saturated += int(((one.u_applied == p["lo"][None]) | (one.u_applied == p["hi"][None])).sum())
        if a == 0.0:                     # b. alpha = 0 retraces the parent, whose controls lie in the box
            for name in ("q", "gamma", "b"):
                _same(getattr(one, name), p[name], f"{which}: {name} at alpha 0")
            _same(one.u_applied, ua, f"{which}: u_applied at alpha 0")
            _same(one.J[0], p["J"], f"{which}: J at alpha 0")
    assert saturated > 0, "no candidate touched a limit"
    # c. the new tape is the open-loop tape of the chosen controls
    ls = tape.linesearch(gains, q, ua, cost, open_door, (0.3, 1.0), **lim)
    J, lq, lr = cost.evaluate(ls.q, ls.u_applied)
    _same(ls.lin_q, lq, f"{which}: lin_q"); _same(ls.lin_r, lr, f"{which}: lin_r")
    *_, ref_tape = plant.rollout_tape(c["model"], c["q1"], c["v1"], ls.u_applied, c["h"], c["mu"], **_kw(which))
    with ls.tape, ref_tape:
        mine, refs = (_tape_answers(t, p, lq, lr, seed=1) for t in (ls.tape, ref_tape))
    for key in refs:
        _same(mine[key], refs[key], f"{which}: {key} of the new tape")
    # d. limits that never bind: the entry with limits against the one without, on the unlimited gains
    inf = np.full(nu, np.inf)
    a, b_ = (tape.linesearch(p["free"], q, ua, cost, p["J"], ALPHAS, **kw) for kw in (dict(), dict(u_lo=-inf, u_hi=inf)))
    with a.tape, b_.tape:
        for name in ("J", "ok", "choice", "q", "u_applied", "gamma", "b", "status", "iters", "lin_q", "lin_r"):
            _same(getattr(b_, name), getattr(a, name), f"{which}: {name} under infinite limits")
        _same(b_.tape.grad_status, a.tape.grad_status, f"{which}: grad_status under infinite limits")


# ---- 5. limited iLQR through contact -------------------------------------------------------------------------------------------------------------
def test_limited_ilqr_through_contact_on_the_hoppers():
    """The hopper contact case of `test_gpu_plant_linesearch`, with limits at 0.6 of the largest |u| the unlimited run ends with."""
    import plant_linesearch_cases as plc
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    kw = dict(alphas=(1.0, 0.5, 0.25), rho0=1e-6, armijo=1e-4, tol=0.0)
    free = plant.ilqr(*_args(c), cost, max_iter=3, **kw)
    free.tape.close()
    bound = 0.6 * np.abs(free.u).max()
    nu = free.u.shape[2]
    u_lo, u_hi = np.full(nu, -bound), np.full(nu, bound)
    assert (np.abs(free.u) > bound).any(), "the unlimited run stays inside the limits: they would not bind"
    runs = [plant.ilqr(*_args(c), cost, max_iter=n, u_lo=u_lo, u_hi=u_hi, **kw) for n in (1, 2, 3)]
    for r in runs:
        r.tape.close()
    res = runs[-1]
    n_it, B = res.J.shape
    print(f"limited hoppers: J0 {res.J0}, J {res.J.tolist()}, alpha {res.alpha.tolist()}, rho {res.rho.tolist()}, accepted {res.accepted.tolist()}, "
          f"limit {bound:.4f}, unlimited J {free.J[-1].tolist()}")
    assert res.accepted.any(), "no robot accepted any iteration"
    J_prev = res.J0
    for i in range(n_it):
        _same(runs[i].J[i], res.J[i], f"iteration {i + 1} of the shorter run")
        assert (res.J[i] <= J_prev).all(), "J increased"
        for b in range(B):
            if res.accepted[i, b]:
                dV, a = runs[i].gains.dV[b], res.alpha[i, b]
                assert res.J[i, b] <= J_prev[b] + 1e-4 * (a * dV[0] + (a * a) * dV[1]), f"Armijo fails at iteration {i + 1}, robot {b}"
            else:
                assert res.J[i, b] == J_prev[b] and np.isnan(res.alpha[i, b])
        J_prev = res.J[i]
        assert np.all(runs[i].u >= -bound) and np.all(runs[i].u <= bound), "a nominal left the box"
    tpb.assert_some_but_not_all_clamp(res.gains.clamped, nu, "the last backward pass")
    assert (np.abs(res.u) == bound).any(), "no control of the result saturates"
    ok, q, ua, *_ = plant.rollout(c["model"], c["q1"], c["v1"], res.u, c["h"], c["mu"])
    _same(q, res.q, "the open-loop rollout of the returned controls")
    _same(cost.evaluate(res.q, res.u)[0], res.J[-1], "the returned cost")


def test_limited_ilqr_in_flight_meets_ten_times_the_cpu_figure():
    """The flight case under `plant_boxqp_cases.flight_limits`, two iterations at rho 0 as `ilqr_cpu_box` runs them: both accepted for both
    particles, the controls in the box with some on it, and the projected gradient of J about the returned nominal (longdouble adjoint chain
    on the device's own blocks), relative to the first nominal's, at most 10 x the CPU restatement's figure - the rule of
    tests/README_plant_linesearch.md; the bound comes from the CPU plant alone."""
    import plant_linesearch_cases as plc
    from contactimplicitmpc.jl_amd import plant
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    u_lo, u_hi = pbc.flight_limits()
    cpu = pbc.flight_cpu()
    cpu_figure = cpu[-1]["pg_end"] / cpu[0]["pg"]
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    res = plant.ilqr(*_args(case), cost, alphas=pbc.FLIGHT_ALPHAS, max_iter=pbc.FLIGHT_ITERATIONS, rho0=0.0, tol=0.0, terrain=case["terrain"],
                     u_lo=u_lo, u_hi=u_hi)
    res.tape.close()
    assert res.accepted.shape == (2, 2) and res.accepted.all()
    assert np.all(res.u >= u_lo[None]) and np.all(res.u <= u_hi[None])
    on = (res.u == u_lo[None]) | (res.u == u_hi[None])
    assert 0 < on.sum() < on.size
    tpb.assert_some_but_not_all_clamp(res.gains.clamped, 3, "flight: the last backward pass")

    def figure(u):
        *_, q, ua, _, _, _, _, G = plant.rollout(case["model"], case["q1"], case["v1"], u, case["h"], case["mu"], terrain=case["terrain"], diff_sol=True)
        _, lq, lr = cost.evaluate(q, ua)
        return float(np.abs(pbc.projected_gradient_ld(G.dz, ua, lq, lr, 3, 3, u_lo, u_hi)).max())
    start, end = figure(pbc.limit(np.broadcast_to(case["u"], res.u.shape), u_lo[None], u_hi[None])), figure(res.u)
    print(f"flight: projected gradient {start:.3e} -> {end:.3e}, {end / start:.3e} of the start (CPU restatement {cpu_figure:.3e}, bound {10 * cpu_figure:.3e}); "
          f"J {res.J0} -> {res.J[-1]} (CPU {cpu[-1]['J_new']})")
    assert end / start <= 10 * cpu_figure
