"""The receding-horizon iLQR policy (`plant.ILQRPolicy`, `cimpc_plant_mpc`; csrc/plant_mpc.hip) against the
definition it is held to: control step s is, bit for bit (NaN matching NaN), `plant.ilqr(device_loop=True)` on `ref.window(s, H)` from the
plan advanced by `shift` (`plant_mpc_cases.compose`).  Each stage of that composition already equals its own host-driven call, and the index
rules are one header, so there is no tolerance to fix.

  1. a closed loop through contact: the three hoppers (H 14, n_iter 2) against a true plant with permuted frictions and one impulse, over a
     reference shorter than S + H (the held last goal)
  2. per-robot terrains and friction in the planner; one step against the host loop as well
  3. limits: the flight case under its limits, the hoppers under per-robot limits; every plan row inside the box
  4. the bookkeeping starts again at every control step: an early end, then level 0 and every robot active
  5. shift 0 twice, shift 3, shift beyond H, and reset
  6. the handle owns its state: unrelated plant calls between two control steps, and policies alive side by side
  7. H = 1, B = 1
  8. it controls: the executed cost under MPC below that of replaying the step-0 plan open loop (tests/README_plant_mpc.md has the figures)
"""
import numpy as np
import pytest

import plant_boxqp_cases as pbc
import plant_gradient_cases as pgc
import plant_ilqr_cases as pic
import plant_mpc_cases as pmc
import plant_staging_cases as pst

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{what} differs"


def _same_step(pol, u, res, what):
    """One control step of a policy against the composition's `ILQRResult`: u, the diagnostics, n_done and the plan."""
    last = pol.last
    _same(u, res.u[0], f"{what}: u")
    for name in ("J0", "J", "alpha", "rho", "accepted"):
        _same(getattr(last, name), getattr(res, name), f"{what}: {name}")
    assert last.n_done == res.J.shape[0], f"{what}: n_done {last.n_done} against {res.J.shape[0]}"
    pu, pq, pg, pb, pst, pit = pol.plan()
    for name, mine in (("u", pu), ("q", pq), ("gamma", pg), ("b", pb)):
        _same(mine, getattr(res, name), f"{what}: plan {name}")
    _same(last.converged, pst.all(axis=0), f"{what}: converged")
    assert pit.shape == pst.shape and (pit >= 0).all()


def _clip(u, lo, hi):
    return u if lo is None else np.where(u < lo, lo, np.where(u > hi, hi, u))


def _drive(plant, pol, c, ref, u0, S, n_iter, kw, what, true_mu=None, impulse=None, terrain=None, u_lo=None, u_hi=None, clamped=None):
    """S control steps of `pol` against the composition, on a true plant (`plant_step`) with its own frictions and one impulse (step, w); the
    planner's terrains are the true plant's.  Returns the per-step `ILQRPolicyStep`s; clamped (a list) receives, per step, whether the
    composition's last backward pass clamped a control."""
    model, h, H = c["model"], c["h"], pol.H
    B = c["q1"].shape[0]
    q0, q1 = c["q1"] - h * c["v1"], c["q1"].copy()
    v1 = c["v1"]
    plan = _clip(np.broadcast_to(u0 if np.ndim(u0) == 3 else np.asarray(u0)[:, None], (H, B, np.shape(u0)[-1])), u_lo, u_hi)
    true_mu = c["mu"] if true_mu is None else true_mu
    steps, s = [], 0
    lim = {} if u_lo is None else dict(u_lo=u_lo, u_hi=u_hi)
    for i in range(S):
        shift = 0 if i == 0 else 1
        s += shift
        u = pol.control(q1, v1)
        assert pol.s == s and pol.last.shift == shift
        uc, res = pmc.compose(plant, model, q1, v1, plan[pmc.warm_rows(shift, H)], h, c["mu"], ref, s, H, n_iter, terrain=terrain, **lim, **kw)
        _same_step(pol, u, res, f"{what}, control step {i}")
        if u_lo is not None:
            pu = pol.plan()[0]
            assert np.all(pu >= u_lo) and np.all(pu <= u_hi), f"{what}, control step {i}: a plan row lies outside the box"
        steps.append(pol.last)
        if clamped is not None:
            clamped.append(bool(res.gains.clamped.any()))
        plan = res.u
        w = None
        if impulse is not None and impulse[0] == i:
            w = np.broadcast_to(impulse[1], (B, len(impulse[1]))).copy()
        q2 = pmc.true_step(plant, model, q0, q1, u, true_mu, h, w=w, terrain=terrain if terrain is not None else c["terrain"])
        q0, q1 = q1, q2
        v1 = (q1 - q0) / h
    print(f"{what}: n_done {[p.n_done for p in steps]}, accepted {[p.accepted.tolist() for p in steps]}, J0 {[p.J0.tolist() for p in steps]}")
    return steps


# ---- 1. a closed loop through contact -----------------------------------------------------------------------------------------------------------
def test_a_closed_loop_through_contact_is_the_composition_bit_for_bit():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    H, S, L, n_iter = 14, 4, 10, 2
    ref = pmc.hopper_reference(plant, L=L)
    assert L < S + H
    with plant.ILQRPolicy(c["model"], 3, H, c["h"], c["mu"], ref, c["u"], n_iter=n_iter, **pic.CONTACT) as pol:
        steps = _drive(plant, pol, c, ref, c["u"], S, n_iter, pic.CONTACT, "contact", true_mu=c["mu"][[2, 0, 1]], impulse=(2, np.array([0.3, 0.0])))
        gamma = pol.plan()[2]
    assert any(p.accepted.any() for p in steps), "no control step accepted a candidate"
    assert (gamma.max(axis=(0, 2)) > 1e-3).all(), "the landing does not lie inside the horizon"


# ---- 2. per-robot terrains and friction in the planner --------------------------------------------------------------------------------------------
def test_per_robot_terrains_and_friction_in_the_planner():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    kw = pic.rollout_kw("hopper_2D")
    terrain, grad_cols = kw["terrain"], kw["grad_cols"]
    assert len(terrain) == 3 and len(set(terrain)) == 3 and len(set(c["mu"].tolist())) == 3
    H, n_iter = 14, 1
    ref = pmc.hopper_reference(plant, L=10, per_robot=True)
    settings = dict(pic.CONTACT, grad_cols=grad_cols)
    with plant.ILQRPolicy(c["model"], 3, H, c["h"], c["mu"], ref, c["u"], n_iter=n_iter, terrain=terrain, **settings) as pol:
        _drive(plant, pol, c, ref, c["u"], 2, n_iter, settings, "per-robot terrains", terrain=terrain)
        pol.reset(c["u"])
        u = pol.control(c["q1"], c["v1"])
        host = plant.ilqr(c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"], ref.window(0, H), max_iter=n_iter, terrain=terrain, device_loop=False, **settings)
        host.tape.close()
        _same_step(pol, u, host, "per-robot terrains, the host loop")


# ---- 3. limits ------------------------------------------------------------------------------------------------------------------------------------
def test_limits_in_flight():
    from contactimplicitmpc.jl_amd import plant
    case, ref = pmc.flight_reference(plant)
    u_lo, u_hi = pbc.flight_limits()
    kw = dict(alphas=pbc.FLIGHT_ALPHAS, rho0=0.0, tol=0.0)
    with plant.ILQRPolicy(case["model"], 2, case["T"], case["h"], case["mu"], ref, case["u"], n_iter=2, terrain=case["terrain"], u_lo=u_lo, u_hi=u_hi, **kw) as pol:
        clamped = []
        steps = _drive(plant, pol, case, ref, case["u"], 3, 2, kw, "flight under limits", terrain=case["terrain"], u_lo=u_lo, u_hi=u_hi, clamped=clamped)
    assert steps[0].accepted.all()
    assert clamped[0], "the first step's backward pass clamps no control: the limits do not bind"      # the setting of test_gpu_plant_ilqr.py's flight test


def test_per_robot_limits_through_contact():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    bound = 0.6 * np.abs(c["u"]).max()
    u_hi = np.outer([1.0, 1.5, 2.0], np.full(2, bound))
    u_lo = -u_hi
    assert (np.abs(c["u"]) > u_hi).any(), "the first plan lies inside the limits: the clip would do nothing"
    ref = pmc.hopper_reference(plant, L=10)
    with plant.ILQRPolicy(c["model"], 3, 14, c["h"], c["mu"], ref, c["u"], n_iter=2, u_lo=u_lo, u_hi=u_hi, **pic.CONTACT) as pol:
        _drive(plant, pol, c, ref, c["u"], 2, 2, pic.CONTACT, "hoppers under per-robot limits", u_lo=u_lo, u_hi=u_hi)


# ---- 4. the bookkeeping ---------------------------------------------------------------------------------------------------------------------------
def test_the_bookkeeping_starts_again_at_every_control_step():
    from contactimplicitmpc.jl_amd import plant
    c, ref, kw = pmc.bookkeeping_reference(plant)
    kw = dict(kw)
    n_iter = kw.pop("max_iter")
    assert n_iter == 6 and ref.x_ref.ndim == 3
    with plant.ILQRPolicy(c["model"], 3, c["T"], c["h"], c["mu"], ref, c["u"], n_iter=n_iter, **kw) as pol:
        steps = _drive(plant, pol, c, ref, c["u"], 2, n_iter, kw, "bookkeeping")
    assert steps[0].n_done < n_iter, "the first control step did not end early"
    assert not steps[0].accepted.all(), "a step that never rejects leaves every robot at level 0 anyway"
    assert steps[0].rho[-1].max() > kw["rho0"], "no robot had left level 0 when the first control step ended"
    _same(steps[1].rho[0], np.full(3, kw["rho0"]), "rho of the second step's first iteration")


# ---- 5. shift -------------------------------------------------------------------------------------------------------------------------------------
def test_shift_zero_three_beyond_the_horizon_and_reset():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    H, n_iter = 14, 1
    ref = pmc.hopper_reference(plant, L=10)
    a = (c["model"], c["q1"], c["v1"])
    b = (c["h"], c["mu"], ref)
    with plant.ILQRPolicy(c["model"], 3, H, c["h"], c["mu"], ref, c["u"], n_iter=n_iter, **pic.CONTACT) as pol:
        u = pol.control(c["q1"], c["v1"])
        first = (u, pol.last, pol.plan())
        _, res = pmc.compose(plant, *a, c["u"], *b, 0, H, n_iter, **pic.CONTACT)
        _same_step(pol, u, res, "the first step")
        s = 0
        for shift in (0, 3, H + 2, H):
            plan = res.u
            s += shift
            u = pol.control(c["q1"], c["v1"], shift=shift)
            assert pol.s == s
            warm = plan[pmc.warm_rows(shift, H)]
            if shift == 0:
                _same(warm, plan, "shift 0 leaves the plan as it is")
            if shift >= H:
                _same(warm, np.broadcast_to(plan[-1], plan.shape), "shift >= H: every row the last")
            _, res = pmc.compose(plant, *a, warm, *b, s, H, n_iter, **pic.CONTACT)
            _same_step(pol, u, res, f"shift {shift}")
        pol.reset(c["u"])
        assert pol.s == 0
        u = pol.control(c["q1"], c["v1"])
        _same(u, first[0], "reset, then control: u")
        for name in ("J0", "J", "alpha", "rho", "accepted", "converged"):
            _same(getattr(pol.last, name), getattr(first[1], name), f"reset, then control: {name}")
        for mine, theirs, name in zip(pol.plan(), first[2], ("u", "q", "gamma", "b", "status", "iters")):
            _same(mine, theirs, f"reset, then control: plan {name}")


# ---- 6. the handle owns its state -------------------------------------------------------------------------------------------------------------------
def test_unrelated_plant_calls_and_other_policies_do_not_disturb_a_policy():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    terrain = pic.rollout_kw("hopper_2D")["terrain"]      # per-robot terrains: what another call overwrites in the shared workspace
    H, n_iter = 14, 2
    ref = pmc.hopper_reference(plant, L=10)
    make = lambda: plant.ILQRPolicy(c["model"], 3, H, c["h"], c["mu"], ref, c["u"], n_iter=n_iter, terrain=terrain, **pic.CONTACT)
    q1b, v1b = c["q1"] + np.array([0.01, 0.0, 0.0, 0.0]), c["v1"] * 0.9
    p = pgc.rollout_case("particle")
    fcase, fref = pmc.flight_reference(plant)
    fkw = dict(alphas=pbc.FLIGHT_ALPHAS, rho0=0.0, tol=0.0)

    def snapshot(pol, u):
        return [u, pol.last.J0, pol.last.J, pol.last.alpha, pol.last.rho, pol.last.accepted, *pol.plan()]

    with make() as alone:
        alone.control(c["q1"], c["v1"])
        want = snapshot(alone, alone.control(q1b, v1b))
    with make() as pol, make() as twin, plant.ILQRPolicy(fcase["model"], 2, fcase["T"], fcase["h"], fcase["mu"], fref, fcase["u"], n_iter=1,
                                                         terrain=fcase["terrain"], **fkw) as other:
        pol.control(c["q1"], c["v1"])
        twin.control(c["q1"] + 0.02, c["v1"])      # another plan of the same size, from another state
        ok, *_ = plant.rollout(p["model"], p["q1"], p["v1"], p["u"], p["h"], p["mu"], terrain=p["terrain"])
        res = plant.ilqr(fcase["model"], fcase["q1"], fcase["v1"], fcase["u"], fcase["h"], fcase["mu"], fref.window(0, fcase["T"]), max_iter=1,
                         terrain=fcase["terrain"], device_loop=True, **fkw)
        res.tape.close()
        uo = other.control(fcase["q1"], fcase["v1"])
        _same_step(other, uo, res, "the other policy beside the two")
        got = snapshot(pol, pol.control(q1b, v1b))
        twin.control(q1b, v1b)
    for k, (mine, theirs) in enumerate(zip(got, want)):
        _same(mine, theirs, f"the second step after unrelated calls, item {k}")


# ---- 7. H = 1, B = 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_one_stage_one_robot():
    from contactimplicitmpc.jl_amd import plant
    import plant_riccati_cases as prc
    c = pgc.rollout_case("particle")
    rng = np.random.default_rng(17)
    Q, R, Qf = prc.weights(rng, 6, 3)
    goal = np.concatenate([c["q1"][0], c["q1"][0]]) + 0.01 * rng.standard_normal((3, 6))
    ref = plant.TrackingReference(Q, R, Qf, x_ref=goal, u_ref=np.zeros((2, 3)))
    kw = dict(alphas=(1.0, 0.3), rho0=1e-3, tol=0.0)
    u0 = np.zeros((1, 3))
    with plant.ILQRPolicy(c["model"], 1, 1, c["h"], c["mu"], ref, u0, n_iter=1, terrain=c["terrain"], **kw) as pol:
        steps = _drive(plant, pol, c, ref, u0, 2, 1, kw, "H = 1, B = 1", terrain=c["terrain"])
    assert all(p.J.shape == (1, 1) for p in steps)


# ---- 8. it controls -----------------------------------------------------------------------------------------------------------------------------------
def test_the_policy_controls_better_than_replaying_its_first_plan():
    """The scene of scripts/closed_loop_ilqr_mpc.py.  On the MI355X (tests/README_plant_mpc.md): the executed cost per robot under MPC and under
    open-loop replay of the step-0 plan, under the same impulse and the same true friction."""
    from contactimplicitmpc.jl_amd import plant
    c, ref, u0, kw = pmc.scene(plant)
    H = pmc.SCENE_STEPS
    first_plan = []
    with plant.ILQRPolicy(c["model"], 3, H, c["h"], c["mu"], ref, u0, **kw) as pol:
        pol.start(c["q1"] - c["h"] * c["v1"])

        def mpc(q):
            u = pol(q)
            if not first_plan:
                first_plan.append(pol.plan()[0])
            return u
        q_mpc, u_mpc = pmc.run_scene(plant, mpc)
        assert pol.s == H - 1
    q_open, u_open = pmc.run_scene(plant, pmc.replay(first_plan[0]))
    _same(u_open, first_plan[0], "the replayed controls")
    J_mpc, J_open = pmc.executed_cost(ref, q_mpc, u_mpc), pmc.executed_cost(ref, q_open, u_open)
    print(f"executed cost under MPC {J_mpc.tolist()}, under open-loop replay of the step-0 plan {J_open.tolist()}")
    assert (J_mpc < J_open).all(), f"MPC {J_mpc.tolist()} against open loop {J_open.tolist()}"


# ---- the optional staged arrays ----------------------------------------------------------------------------------------------------------------
def test_shared_absent_and_per_robot_arrays_give_the_same_bits():
    """Two control steps of a policy whose mu and limits are shared against the same values per robot, and without limits against infinite
    ones (csrc/plant_staging.h; tests/plant_staging_cases.py): the controls, the diagnostics and the plan bit for bit, at B = 2, H = 4."""
    from contactimplicitmpc.jl_amd import plant
    (model, q1, v1, u, h), _, _ = pst.hopper()
    ref = pmc.hopper_reference(plant, L=6)

    def run(mu, u_lo=None, u_hi=None):
        lim = {} if u_lo is None else dict(u_lo=u_lo, u_hi=u_hi)
        u0 = u if u_lo is None else np.clip(u, u_lo, u_hi)      # a plan inside its limits
        out = {}
        with plant.ILQRPolicy(model, pst.B, pst.T, h, mu, ref, u0, n_iter=pst.ITERS, alphas=pst.ALPHAS, rho0=1e-6, tol=0.0, **lim) as pol:
            for s in range(2):
                out[f"step {s}: u"] = pol.control(q1, v1)
                out.update(pst.arrays(pol.last, f"step {s}: "))
            out.update(zip(("plan u", "plan q", "plan gamma", "plan b", "plan status", "plan iters"), pol.plan()))
        return out

    print("cimpc_plant_mpc_create, _control, _plan:", pst.loop_pairs(run, with_w=False), "arrays compared")
