"""The device-resident iLQR loop (`plant.ilqr(device_loop=True)`, `cimpc_plant_ilqr`; csrc/plant_ilqr.hip)
against the host loop `plant.ilqr(device_loop=False)` in the same process.  Every comparison is bitwise (NaN matching NaN): each stage
already equals its host-driven call bit for bit and the rules are one header, so there is no tolerance to fix.

  1. contact, without limits: the hopper case (B 3, T 14), max_iter 1 and 4 - the result, the last gains, the final tape's answers, and an
     open-loop rollout of the returned controls
  2. the same under a per-robot disturbance schedule held 7 steps, per-robot friction and per-robot terrains (uploaded once now)
  3. the bookkeeping: settings under which the HOST loop shows a rejection followed by an acceptance, a robot stopped by `small` beside
     one that continues, a robot stopped by rho_max, and an end before max_iter - asserted on the host's history first
  4. limits: the flight case, and the hoppers at 0.6 of the largest |u| of the unlimited run; every control inside the box exactly
  5. a second step instantiation: the particle on its bowl
  6. the caller's tape answers `lqr` and `vjp` after a device loop as before it; a second device loop gives the first one's bits

tests/README_plant_ilqr.md has what was measured.
"""
import numpy as np
import pytest

import plant_boxqp_cases as pbc
import plant_gradient_cases as pgc
import plant_ilqr_cases as pic
import plant_linesearch_cases as plc
import plant_staging_cases as pst

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{what} differs"


def _tape_answers(tape, cost, q, u, seed=0):
    """What a tape says: `lqr` with the cost's linear terms on (q, u) and a `vjp` of seeded random cotangents."""
    nq, nu, nc, nb = pgc.dims(tape.model)[:4]
    _, lq, lr = cost.evaluate(q, u)
    rng = np.random.default_rng([seed, tape.T, tape.B])
    g = tape.lqr(cost.Q, cost.R, cost.Qf, q=lq, r=lr, rho=1e-3)
    v = tape.vjp(gq=rng.standard_normal((tape.T + 2, tape.B, nq)), ggamma=rng.standard_normal((tape.T, tape.B, nc)), gb=rng.standard_normal((tape.T, tape.B, nb)))
    out = dict(K=g.K, k=g.k, P0=g.P0, p0=g.p0, dV=g.dV, lq_status=g.status, lq_cut=g.n_cut, g_q0=v.g_q0, g_q1=v.g_q1, u_step=v.u_step, n_cut=v.n_cut,
               grad_status=tape.grad_status)
    for key in ("w_step", "g_mu", "g_h"):
        if getattr(v, key) is not None:
            out[key] = getattr(v, key)
    return out


def _compare(dev, host, cost, what, limited=False):
    """Everything the two loops return, and what their final tapes answer; closes both tapes."""
    with dev.tape, host.tape:
        for name in ("u", "q", "gamma", "b", "J", "alpha", "rho", "accepted", "J0"):      # n_iter through the history's shape
            _same(getattr(dev, name), getattr(host, name), f"{what}: {name}")
        for name in ("K", "k", "dV", "status", "n_cut") + (("clamped",) if limited else ()):
            _same(getattr(dev.gains, name), getattr(host.gains, name), f"{what}: gains.{name}")
        _same(dev.gains.K_blocks.transpose(0, 1, 3, 2), dev.gains.K, f"{what}: K in both forms")
        mine, theirs = (_tape_answers(r.tape, cost, r.q, r.u) for r in (dev, host))
    assert sorted(mine) == sorted(theirs)
    for key in theirs:
        _same(mine[key], theirs[key], f"{what}: {key} of the final tape")
    print(f"{what}: {host.J.shape[0]} iterations, accepted {host.accepted.tolist()}, rho {host.rho.tolist()}, J0 {host.J0.tolist()}, J {host.J[-1].tolist()}")


def _both(args, cost, **kw):
    from contactimplicitmpc.jl_amd import plant
    return plant.ilqr(*args, cost, device_loop=True, **kw), plant.ilqr(*args, cost, device_loop=False, **kw)


def _contact():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    return c, plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)


# ---- 1. contact, without limits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", (1, 4))
def test_contact_without_limits(max_iter):
    from contactimplicitmpc.jl_amd import plant
    c, cost = _contact()
    dev, host = _both(pic.args(c), cost, max_iter=max_iter, **pic.CONTACT)
    assert host.J.shape == (max_iter, 3) and host.accepted.any()
    ok, q, *_ = plant.rollout(c["model"], c["q1"], c["v1"], dev.u, c["h"], c["mu"])
    _same(q, dev.q, "the open-loop rollout of the returned controls")
    _compare(dev, host, cost, f"contact, max_iter {max_iter}")


# ---- 2. the same with more varied inputs ------------------------------------------------------------------------------------------------------
def test_contact_under_per_robot_disturbances_friction_and_terrains():
    c, cost = _contact()
    kw = pic.rollout_kw("hopper_2D")
    assert np.shape(kw["w"])[1] == 3 and len(kw["terrain"]) == 3 and kw["w_hold"] == 7 and len(set(c["mu"].tolist())) == 3
    dev, host = _both(pic.args(c), cost, max_iter=3, **pic.CONTACT, **kw)
    _compare(dev, host, cost, "contact, varied inputs")


# ---- 3. the bookkeeping -------------------------------------------------------------------------------------------------------------------------
def test_the_bookkeeping_follows_the_host_loop_through_every_event():
    from contactimplicitmpc.jl_amd import plant
    c, (Q, R, Qf, x_goal, u_goal), kw = pic.bookkeeping()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    host = plant.ilqr(*pic.args(c), cost, device_loop=False, **kw)
    seen = pic.events(host, **kw)
    print(f"bookkeeping (host): accepted {host.accepted.tolist()}, rho {host.rho.tolist()}, J0 {host.J0.tolist()}, J {host.J.tolist()}, events {seen}")
    assert not host.accepted.all(), "a run that never rejects cannot pass"
    assert all(seen.values()), f"the host loop's history lacks an event: {seen}"
    dev = plant.ilqr(*pic.args(c), cost, device_loop=True, **kw)
    assert dev.J.shape[0] == host.J.shape[0] < kw["max_iter"]
    _compare(dev, host, cost, "bookkeeping")


# ---- 4. limits ----------------------------------------------------------------------------------------------------------------------------------
def _inside(res, u_lo, u_hi):
    assert np.all(res.u >= u_lo) and np.all(res.u <= u_hi), "a returned control lies outside the box"


def test_limits_in_flight():
    from contactimplicitmpc.jl_amd import plant
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    u_lo, u_hi = pbc.flight_limits()
    dev, host = _both(pic.args(case), cost, alphas=pbc.FLIGHT_ALPHAS, max_iter=2, rho0=0.0, tol=0.0, terrain=case["terrain"], u_lo=u_lo, u_hi=u_hi)
    assert host.accepted.all() and host.gains.clamped.any()
    _inside(dev, u_lo, u_hi)
    _compare(dev, host, cost, "flight under limits", limited=True)


def test_limits_through_contact_on_the_hoppers():
    from contactimplicitmpc.jl_amd import plant
    c, cost = _contact()
    free = plant.ilqr(*pic.args(c), cost, max_iter=3, armijo=1e-4, **pic.CONTACT)
    free.tape.close()
    bound = 0.6 * np.abs(free.u).max()
    assert (np.abs(free.u) > bound).any(), "the unlimited run stays inside the limits: they would not bind"
    nu = free.u.shape[2]
    u_lo, u_hi = np.full(nu, -bound), np.full(nu, bound)
    dev, host = _both(pic.args(c), cost, max_iter=3, u_lo=u_lo, u_hi=u_hi, **pic.CONTACT)
    assert host.gains.clamped.any()
    _inside(dev, u_lo, u_hi)
    _compare(dev, host, cost, "hoppers under limits", limited=True)
    # limits per robot: the expansion kernel writes the candidates' limit rows
    lo3, hi3 = np.stack([u_lo, 1.5 * u_lo, 2.0 * u_lo]), np.stack([u_hi, 1.5 * u_hi, 2.0 * u_hi])
    dev, host = _both(pic.args(c), cost, max_iter=2, u_lo=lo3, u_hi=hi3, **pic.CONTACT)
    _inside(dev, lo3, hi3)
    _compare(dev, host, cost, "hoppers under per-robot limits", limited=True)


# ---- 5. a second step instantiation -------------------------------------------------------------------------------------------------------------
def test_the_particle_on_its_bowl():
    from contactimplicitmpc.jl_amd import plant
    import plant_riccati_cases as prc
    c = pgc.rollout_case("particle")
    nq, nu = pgc.dims(c["model"])[:2]
    T = c["T"]
    rng = np.random.default_rng([7, nq, nu, T])
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step=True)      # a weight per step: n_Q = n_R = T
    goal = np.concatenate([c["q1"][0], c["q1"][0]]) + 0.02 * rng.standard_normal((T + 1, 2 * nq))
    cost = plant.TrackingCost(Q, R, Qf, x_goal=goal)
    dev, host = _both(pic.args(c), cost, alphas=(1.0, 0.3), max_iter=1, rho0=1e-3, tol=0.0, terrain=c["terrain"])
    assert host.J.shape == (1, 1)
    _compare(dev, host, cost, "particle")


# ---- 6. the caller's tape ------------------------------------------------------------------------------------------------------------------------
def test_the_callers_tape_is_untouched_and_a_second_loop_gives_the_first_ones_bits():
    from contactimplicitmpc.jl_amd import plant
    c, cost = _contact()
    kw = pic.rollout_kw("hopper_2D")
    ok, q, ua, gamma, b, status, iters, tape = plant.rollout_tape(*pic.args(c), **kw)
    with tape:
        before = _tape_answers(tape, cost, q, ua, seed=3)
        runs = [plant.ilqr_from_tape(tape, q, ua, gamma, b, status, iters, cost, max_iter=3, **pic.CONTACT) for _ in range(2)]
        after = _tape_answers(tape, cost, q, ua, seed=3)
    for key in before:
        _same(after[key], before[key], f"{key} of the caller's tape after the loop")
    first, second = runs
    assert first.accepted.any()
    _compare(second, first, cost, "a second device loop")
    # and the loop from a tape is the loop from the rollout's arguments
    whole = plant.ilqr(*pic.args(c), cost, device_loop=True, max_iter=3, **pic.CONTACT, **kw)
    whole.tape.close()
    for name in ("u", "q", "J", "alpha", "rho", "accepted"):
        _same(getattr(whole, name), getattr(first, name), f"ilqr(device_loop=True) against ilqr_from_tape: {name}")


# ---- the optional staged arrays ----------------------------------------------------------------------------------------------------------------
def test_shared_absent_and_per_robot_arrays_give_the_same_bits():
    """The entry's optional staged arrays (csrc/plant_staging.h) at B = 2, T = 4, two step lengths, two iterations: mu, w and the limits shared
    against the same values per robot, and no limits against infinite ones, every returned array bit for bit (tests/plant_staging_cases.py)."""
    from contactimplicitmpc.jl_amd import plant
    args, _, (Q, R, Qf, x_goal, u_goal) = pst.hopper()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)

    def run(mu, **kw):
        res = plant.ilqr(*args, mu, cost, device_loop=True, **pst.LOOP, **kw)
        out = pst.arrays(res)
        res.tape.close()
        return out

    print("cimpc_plant_ilqr:", pst.loop_pairs(run), "arrays compared")
