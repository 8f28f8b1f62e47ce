"""The sampling policy (`plant.SamplingPolicy`, `cimpc_plant_sampler`; csrc/plant_sample.hip) against the
definition it is held to: a control step is, bit for bit (NaN matching NaN), the composition of `plant_sample_cases.compose` - the goal
window, the warm rows, the restated candidates, ONE `plant.rollout` of N B robots, `TrackingCost.evaluate`, the restated choice and update -
run in the same process.  The one link with a distance is the device's `exp` (test 4).

  1. a closed loop through contact: the three hoppers (H 14, N 4, n_iter 2, lam 0) against a true plant with permuted frictions and an impulse
  2. per-robot terrains, friction and goals, noise held over 3 steps; a policy over the first two robots alone gives those robots' bits
  3. limits: the flight case under its limits, shared and per robot; candidates clip, and every row stays inside the box
  4. the MPPI mean: the weights against `math.exp` in ulps, the new plan on the device's weights bit for bit, `plan()` against `plant.rollout`
  5. repeatability, another seed, shifts 0, 3, H and H + 2, and the draws 2 s and 2 s + 1
  6. the handle owns its state: other policies and plant calls between two control steps
  7. H = 1, B = 1, N = 1, and N = 65
  8. ineligible candidates under a low iteration cap: a robot whose candidates all fail keeps its plan, a robot with both kinds chooses an eligible one
  9. it controls: the executed cost under the policy against open-loop replay of the step-0 plan (tests/README_plant_sample.md has the figures)
"""
import dataclasses
import math

import numpy as np
import pytest

import plant_boxqp_cases as pbc
import plant_gradient_cases as pgc
import plant_ilqr_cases as pic
import plant_mpc_cases as pmc
import plant_sample_cases as psc
import plant_staging_cases as pst

pytestmark = pytest.mark.gpu

# The margin of link 4(a), in ulps of the unnormalised weight: four times the largest distance between the device's exp and `math.exp`
# seen in this test's runs on the MI355X (tests/README_plant_sample.md), since the installed ROCm documentation states no bound.
EXP_ULPS_SEEN = 1
EXP_ULPS = 4 * EXP_ULPS_SEEN


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: {a.shape} against {b.shape}"
    assert a.dtype.kind == b.dtype.kind or {a.dtype.kind, b.dtype.kind} <= {"i", "b"}, f"{what}: {a.dtype} against {b.dtype}"
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{what} differs"


def _policy(plant, c, B, H, ref, u0, st, **kw):
    return plant.SamplingPolicy(c["model"], B, H, c["h"], c["mu"][:B] if np.size(c["mu"]) > 1 else c["mu"], ref, u0, **st, **kw)


def _compose(plant, c, q1, v1, warm, ref, s, H, st, **kw):
    st = dict(st)
    return psc.compose(plant, c["model"], q1, v1, warm, c["h"], c["mu"][:q1.shape[0]] if np.size(c["mu"]) > 1 else c["mu"], ref, s, H, st.pop("n_samples"),
                       st.pop("sigma"), **st, **kw)


def _same_step(plant, pol, u, comp, what, state=None, terrain=None):
    """One control step of a policy against the composition: u, the diagnostics and the plan.  With lam > 0 the plan's trajectory is held to
    `plant.rollout` on the plan from state = (q1, v1) instead of to the chosen candidate's rows."""
    last = pol.last
    _same(u, comp["u"], f"{what}: u")
    for name in ("J0", "J_nom", "J_best", "choice", "n_eligible", "J", "weights", "converged"):
        _same(getattr(last, name), comp[name], f"{what}: {name}")
    pu, pq, pg, pb, pst, pit = pol.plan()
    _same(pu, comp["plan"], f"{what}: plan u")
    _same(pu[0], u, f"{what}: u is row 0 of the plan")
    if pol.lam == 0.0:
        want = comp["traj"]
    else:
        r = plant.rollout(pol.model, state[0], state[1], pu, pol.h, pol.mu, terrain=terrain)
        want = (r[1], r[3], r[4], r[5], r[6])
    for name, mine, theirs in zip(("q", "gamma", "b", "status", "iters"), (pq, pg, pb, pst, pit), want):
        _same(mine, theirs, f"{what}: plan {name}")


def _drive(plant, pol, c, ref, u0, S, st, what, true_mu=None, impulse=None, terrain=None, lim=None, seen=None):
    """S control steps of `pol` against the composition, on a true plant (`plant_step`) with its own frictions and one impulse (step, w).
    seen (a list) receives the compositions."""
    model, h, H, B = c["model"], c["h"], pol.H, pol.B
    q1, v1 = c["q1"][:B].copy(), c["v1"][:B]
    q0 = q1 - h * v1
    lim = lim or {}
    plan = psc.limit(np.broadcast_to(u0 if np.ndim(u0) == 3 else np.asarray(u0)[:, None], (H, B, np.shape(u0)[-1])), *psc._limits(lim.get("u_lo"), lim.get("u_hi"), np.shape(u0)[-1]))
    true_mu = c["mu"] if true_mu is None else true_mu
    s = 0
    for i in range(S):
        shift = 0 if i == 0 else 1
        s += shift
        u = pol.control(q1, v1)
        assert pol.s == s and pol.last.shift == shift
        comp = _compose(plant, c, q1, v1, plan[pmc.warm_rows(shift, H)], ref, s, H, st, terrain=terrain, **lim)
        _same_step(plant, pol, u, comp, f"{what}, control step {i}", state=(q1, v1), terrain=terrain)
        if lim:
            lo, hi = psc._limits(lim["u_lo"], lim["u_hi"], u.shape[-1])
            assert np.all(comp["cand"] >= lo) and np.all(comp["cand"] <= hi), f"{what}, control step {i}: a candidate row lies outside the box"
            assert np.all(pol.plan()[0] >= lo) and np.all(pol.plan()[0] <= hi), f"{what}, control step {i}: a plan row lies outside the box"
        if seen is not None:
            seen.append(comp)
        plan = comp["plan"]
        w = None
        if impulse is not None and impulse[0] == i:
            w = np.broadcast_to(impulse[1], (B, len(impulse[1]))).copy()
        q2 = pmc.true_step(plant, model, q0, q1, u, true_mu, h, w=w, terrain=terrain if terrain is not None else c["terrain"])
        q0, q1 = q1, q2
        v1 = (q1 - q0) / h
    return seen


def _hoppers(plant, **st):
    c = pgc.rollout_case("hopper_2D")
    return c, dict(dict(n_samples=4, sigma=psc.hopper_sigma(c), noise_hold=1, lam=0.0, n_iter=2, seed=0), **st)


# ---- 1. a closed loop through contact -----------------------------------------------------------------------------------------------------------
def test_a_closed_loop_through_contact_is_the_composition_bit_for_bit():
    from contactimplicitmpc.jl_amd import plant
    c, st = _hoppers(plant)
    H, S, L = 14, 4, 10
    ref = pmc.hopper_reference(plant, L=L)
    with _policy(plant, c, 3, H, ref, c["u"], st) as pol:
        seen = _drive(plant, pol, c, ref, c["u"], S, st, "contact", true_mu=c["mu"][[2, 0, 1]], impulse=(2, np.array([0.3, 0.0])), seen=[])
        gamma = pol.plan()[2]
    assert seen[0]["ok"][0, 1:].any(axis=0).all(), "step 0: a robot without an eligible candidate beside the plan itself"      # sigma: psc.hopper_sigma
    assert any((comp["choice"] > 0).any() for comp in seen), "no control step chose a perturbed candidate"
    assert (gamma.max(axis=(0, 2)) > 1e-3).all(), "the landing does not lie inside the horizon"
    print(f"contact: choice {[comp['choice'].tolist() for comp in seen]}, J_best {[comp['J_best'][-1].tolist() for comp in seen]}")


# ---- 2. per-robot terrains, friction and goals ---------------------------------------------------------------------------------------------------
def test_per_robot_terrains_friction_and_goals_and_a_sub_batch():
    from contactimplicitmpc.jl_amd import plant
    c, st = _hoppers(plant, noise_hold=3, n_iter=1, seed=5)
    terrain = pic.rollout_kw("hopper_2D")["terrain"]
    assert len(terrain) == 3 and len(set(terrain)) == 3 and len(set(c["mu"].tolist())) == 3
    H = 14
    assert psc.noise_rows(H, 3) == 5 and H % 3 != 0      # the last noise row is partial
    ref = pmc.hopper_reference(plant, L=10, per_robot=True)
    with _policy(plant, c, 3, H, ref, c["u"], st, terrain=terrain) as pol:
        _drive(plant, pol, c, ref, c["u"], 2, st, "per-robot terrains", terrain=terrain)
        pol.reset(c["u"])
        u3 = pol.control(c["q1"], c["v1"])
        last3, plan3 = pol.last, pol.plan()
    ref2 = plant.TrackingReference(ref.Q, ref.R, ref.Qf, x_ref=ref.x_ref[:, :2], u_ref=ref.u_ref)
    with _policy(plant, c, 2, H, ref2, c["u"][:, :2], st, terrain=terrain[:2]) as pol:
        u2 = pol.control(c["q1"][:2], c["v1"][:2])
        _same(u2, u3[:2], "the first two robots alone: u")
        for name in ("J0", "J_nom", "J_best", "choice", "n_eligible", "J", "weights", "converged"):
            _same(getattr(pol.last, name), getattr(last3, name)[..., :2], f"the first two robots alone: {name}")
        for name, mine, theirs in zip(("u", "q", "gamma", "b", "status", "iters"), pol.plan(), plan3):
            _same(mine, theirs[:, :2], f"the first two robots alone: plan {name}")


# ---- 3. limits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_robot", (False, True))
def test_limits_in_flight(per_robot):
    from contactimplicitmpc.jl_amd import plant
    case, ref = pmc.flight_reference(plant)
    u_lo, u_hi = pbc.flight_limits()
    if not per_robot:
        u_lo, u_hi = u_lo[:1], u_hi[:1]
    assert case["q1"].shape[0] == 2 and case["T"] == 8 and u_lo.shape == ((2, 3) if per_robot else (1, 3))
    st = dict(n_samples=4, sigma=np.full(3, float(u_hi.max())), noise_hold=2, lam=0.0, n_iter=2, seed=2)      # sigma of the size of the box: candidates clip
    lim = dict(u_lo=u_lo, u_hi=u_hi)
    with _policy(plant, case, 2, case["T"], ref, case["u"], st, terrain=case["terrain"], **lim) as pol:
        seen = _drive(plant, pol, case, ref, case["u"], 2, st, "flight under limits", terrain=case["terrain"], lim=lim, seen=[])
    cand = seen[0]["cand"][:, :, 1:]
    assert ((cand == u_lo) | (cand == u_hi)).any(), "no candidate entry sits on a bound: the limits do not bind"


# ---- 4. the MPPI mean -----------------------------------------------------------------------------------------------------------------------------
def test_the_mppi_mean_weights_in_ulps_and_the_plan_on_the_devices_weights_bit_for_bit():
    """lam = 3.0, of the size of the spread of J over a robot's candidates at step 0 (read off the composition, which the test prints and
    holds lam to within a factor of four of)."""
    from contactimplicitmpc.jl_amd import plant
    lam = 3.0
    c, st = _hoppers(plant, lam=lam)
    H = 14
    ref = pmc.hopper_reference(plant, L=10)
    with _policy(plant, c, 3, H, ref, c["u"], st) as pol:
        u = pol.control(c["q1"], c["v1"])
        raw = pol.raw_weights()
        comp = _compose(plant, c, c["q1"], c["v1"], c["u"], ref, 0, H, st, raw=raw)
        _same(pol.last.J, comp["J"], "J")
        spread = comp["J"][0].max(axis=0) - comp["J"][0].min(axis=0)
        print(f"MPPI: spread of J at step 0 per robot {spread.tolist()}, lam {lam}")
        assert spread.min() / 4.0 <= lam <= 4.0 * spread.max()
        # (a) the device's unnormalised weights against math.exp on the device's own J
        worst = 0
        for it in range(st["n_iter"]):
            J, ok, ch = pol.last.J[it], comp["ok"][it], comp["choice"][it]
            assert (ch >= 0).all() and ok.sum() > 3
            want = np.array([[math.exp(-((J[k, b] - J[ch[b], b]) / lam)) if ok[k, b] else 0.0 for b in range(3)] for k in range(st["n_samples"])])
            assert np.array_equal(raw[it] == 0.0, want == 0.0)
            d = int(psc.ulps(raw[it][ok], want[ok]).max())
            worst = max(worst, d)
        print(f"MPPI: the device's exp against math.exp: at most {worst} ulp")
        assert worst <= EXP_ULPS, f"{worst} ulps between the device's exp and math.exp, margin {EXP_ULPS}"
        # (b) everything else on the device's weights, bit for bit; plan() is plant.rollout on the plan, run once
        assert pol.plan_rollouts == 0
        _same_step(plant, pol, u, comp, "MPPI", state=(c["q1"], c["v1"]))
        assert pol.plan_rollouts == 1
        again = pol.plan()
        assert pol.plan_rollouts == 1, "a second plan() rolled the plan out again"
        for mine, theirs in zip(again, pol.plan()):
            _same(mine, theirs, "a second plan()")
        assert (pol.last.weights.sum(axis=1) > 0.999).all() and (pol.last.weights > 0).sum() > 2 * 3 * st["n_iter"], "the mean is over one candidate only"
        assert not np.array_equal(pol.plan()[0], comp["cand"][-1][:, comp["choice"][-1], np.arange(3)]), "the mean is a candidate"


# ---- 5. repeatability and shift -------------------------------------------------------------------------------------------------------------------
def test_repeatability_another_seed_shifts_and_draws():
    from contactimplicitmpc.jl_amd import plant
    c, st = _hoppers(plant)
    H = 14
    ref = pmc.hopper_reference(plant, L=10)
    q1, v1 = c["q1"], c["v1"]
    snapshot = lambda pol, u: [u, *(getattr(pol.last, k) for k in ("J0", "J_nom", "J_best", "choice", "n_eligible", "J", "weights", "converged")), *pol.plan()]
    with _policy(plant, c, 3, H, ref, c["u"], st) as pol:
        pol.reset(s=3)
        first = snapshot(pol, pol.control(q1, v1))
        assert pol.s == 3
        comp = _compose(plant, c, q1, v1, c["u"], ref, 3, H, st, draws=[6, 7])      # n_iter 2: the draws of step s are 2 s and 2 s + 1
        _same_step(plant, pol, first[0], comp, "s = 3 with explicit draws")
        other = _compose(plant, c, q1, v1, c["u"], ref, 3, H, st, draws=[3, 4])
        assert not np.array_equal(other["J"], comp["J"]), "the draw does not enter"
        pol.reset(c["u"], s=3)
        for k, (mine, theirs) in enumerate(zip(snapshot(pol, pol.control(q1, v1)), first)):
            _same(mine, theirs, f"reset, then control at the same s: item {k}")
        s = 3
        for shift in (0, 3, H, H + 2):
            plan = comp["plan"]
            s += shift
            u = pol.control(q1, v1, shift=shift)
            assert pol.s == s
            warm = plan[pmc.warm_rows(shift, H)]
            if shift >= H:
                _same(warm, np.broadcast_to(plan[-1], plan.shape), "shift >= H: every row the last")
            comp = _compose(plant, c, q1, v1, warm, ref, s, H, st)
            _same_step(plant, pol, u, comp, f"shift {shift}")
    with _policy(plant, c, 3, H, ref, c["u"], dict(st, seed=(1 << 32) + 1)) as pol:
        pol.reset(s=3)
        pol.control(q1, v1)
        assert not (np.array_equal(pol.last.choice, first[4]) and np.array_equal(pol.last.J, first[6], equal_nan=True)), "another seed, the same choice and J"


# ---- 6. the handle owns its state -------------------------------------------------------------------------------------------------------------------
def test_unrelated_plant_calls_and_other_policies_do_not_disturb_a_policy():
    from contactimplicitmpc.jl_amd import plant
    c, st = _hoppers(plant)
    terrain = pic.rollout_kw("hopper_2D")["terrain"]      # per-robot terrains: what another call overwrites in the shared workspace
    H = 14
    ref = pmc.hopper_reference(plant, L=10)
    make = lambda **kw: _policy(plant, c, 3, H, ref, c["u"], dict(st, **kw), terrain=terrain)
    q1b, v1b = c["q1"] + np.array([0.01, 0.0, 0.0, 0.0]), c["v1"] * 0.9
    p = pgc.rollout_case("particle")
    snapshot = lambda pol, u: [u, *(getattr(pol.last, k) for k in ("J0", "J_nom", "J_best", "choice", "n_eligible", "J", "weights", "converged")), *pol.plan()]
    with make() as alone:
        alone.control(c["q1"], c["v1"])
        want = snapshot(alone, alone.control(q1b, v1b))
    with make() as pol, make(seed=9, n_samples=7, lam=2.0) as twin, plant.ILQRPolicy(c["model"], 3, H, c["h"], c["mu"], ref, c["u"], n_iter=1, **pic.CONTACT) as ilqr:
        pol.control(c["q1"], c["v1"])
        twin.control(c["q1"] + 0.02, c["v1"])      # another sampling policy, of another size, from another state
        twin.plan()
        ilqr.control(c["q1"], c["v1"])
        ok, *_ = plant.rollout(p["model"], p["q1"], p["v1"], p["u"], p["h"], p["mu"], terrain=p["terrain"])
        got = snapshot(pol, pol.control(q1b, v1b))
    for k, (mine, theirs) in enumerate(zip(got, want)):
        _same(mine, theirs, f"the second step after unrelated calls, item {k}")


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_stage_one_robot_one_candidate_and_more_candidates_than_a_wavefront():
    from contactimplicitmpc.jl_amd import plant
    import plant_riccati_cases as prc
    c = pgc.rollout_case("particle")
    rng = np.random.default_rng(17)
    Q, R, Qf = prc.weights(rng, 6, 3)
    goal = np.concatenate([c["q1"][0], c["q1"][0]]) + 0.01 * rng.standard_normal((3, 6))
    ref = plant.TrackingReference(Q, R, Qf, x_ref=goal, u_ref=np.zeros((2, 3)))
    u0 = np.array([[0.01, -0.0, 0.02]])
    st = dict(n_samples=1, sigma=np.full(3, 0.05), noise_hold=1, lam=0.0, n_iter=1, seed=4)
    with _policy(plant, c, 1, 1, ref, u0, st, terrain=c["terrain"]) as pol:
        u = pol.control(c["q1"], c["v1"])
        comp = _compose(plant, c, c["q1"], c["v1"], u0[:, None], ref, 0, 1, st, terrain=c["terrain"])
        _same_step(plant, pol, u, comp, "H = B = N = 1")
        _same(pol.plan()[0], u0[:, None], "N = 1: the plan is unchanged")
        assert np.signbit(pol.plan()[0][0, 0, 1]), "-0.0 in the plan must stay -0.0"
        _same(pol.last.J_best[0], pol.last.J0, "J_best = J0")
        assert pol.last.choice.tolist() == [[0]] and pol.last.n_eligible.tolist() == [[1]] and pol.last.weights.tolist() == [[[1.0]]]
    for lam in (0.0, 0.05):
        st = dict(n_samples=65, sigma=np.full(3, 0.05), noise_hold=1, lam=lam, n_iter=2, seed=4)
        u0 = np.zeros((2, 3))
        with _policy(plant, c, 1, 2, ref, u0, st, terrain=c["terrain"]) as pol:
            u = pol.control(c["q1"], c["v1"])
            comp = _compose(plant, c, c["q1"], c["v1"], u0[:, None], ref, 0, 2, st, terrain=c["terrain"], raw=pol.raw_weights() if lam else None)
            _same_step(plant, pol, u, comp, f"N = 65, lam {lam}", state=(c["q1"], c["v1"]), terrain=c["terrain"])
            assert pol.last.J.shape == (2, 65, 1) and (pol.last.n_eligible == 65).all()
            if lam:
                want = np.vectorize(math.exp)(-((pol.last.J - pol.last.J_best[:, None]) / lam))
                worst = int(psc.ulps(pol.raw_weights(), want).max())
                print(f"N = 65: the device's exp against math.exp: at most {worst} ulp over {want.size} weights")
                assert worst <= EXP_ULPS


# ---- 8. ineligible candidates -----------------------------------------------------------------------------------------------------------------------
# Found on the composition by a search over seeds 0 .. 15 and the iteration cap (tests/README_plant_sample.md): with max_iter = 8 and seed 2 the
# flight steps converge and the contact steps of some candidates do not - robot 0 has both kinds of candidate (2 of 4 eligible), robot 1 only
# eligible ones, and robot 2 none.
INELIGIBLE = dict(max_iter=8, seed=2)


def test_a_robot_whose_candidates_all_fail_keeps_its_plan_and_a_robot_with_both_kinds_chooses_among_the_eligible():
    from contactimplicitmpc.jl_amd import plant
    c, st = _hoppers(plant, n_iter=1, seed=INELIGIBLE["seed"])
    H, N = 14, st["n_samples"]
    ref = pmc.hopper_reference(plant, L=10)
    opts = dataclasses.replace(plant.SIM_OPTS, max_iter=INELIGIBLE["max_iter"])
    with _policy(plant, c, 3, H, ref, c["u"], st, opts=opts) as pol:
        u = pol.control(c["q1"], c["v1"])
        comp = _compose(plant, c, c["q1"], c["v1"], c["u"], ref, 0, H, st, opts=opts)
        _same_step(plant, pol, u, comp, "ineligible candidates")
        ne, ch = comp["n_eligible"][0], comp["choice"][0]
        print(f"ineligible: n_eligible {ne.tolist()}, choice {ch.tolist()}, converged steps of the kept trajectories {pol.plan()[4].sum(axis=0).tolist()} of {H}")
        assert ((ne > 0) & (ne < N)).any(), "no robot with both kinds of candidate"
        none = ne == 0
        assert none.any(), "no robot with every candidate ineligible"
        assert np.isfinite(comp["J"][0][:, none]).all(), "the candidates are ineligible for their J, not for their steps"
        assert (pol.last.choice[0][none] == -1).all() and not pol.last.weights[0][:, none].any() and not pol.last.converged[none].any()
        _same(pol.plan()[0][:, none], c["u"][:, none], "the plan is kept")
        _same(pol.last.J_best[0][none], pol.last.J_nom[0][none], "J_best is J_nom where there is no choice")
        mixed = (ne > 0) & (ne < N)
        assert comp["ok"][0][ch[mixed], np.flatnonzero(mixed)].all(), "a choice that is not eligible"
        assert pol.last.converged[~none].all()


# ---- 9. it controls -----------------------------------------------------------------------------------------------------------------------------------
def test_the_policy_controls_better_than_replaying_its_first_plan():
    """The scene of scripts/closed_loop_sampling_mpc.py with `plant_sample_cases.SCENE_SAMPLING`, fixed before the first run.  That run on the
    MI355X showed the executed cost under the policy below the replay's for every robot (56.69, 20.55, 44.44 against 57.85, 41.00, 127.94;
    tests/README_plant_sample.md), so the ordering is asserted."""
    from contactimplicitmpc.jl_amd import plant
    c, ref, u0, _ = pmc.scene(plant)
    H = pmc.SCENE_STEPS
    st = dict(psc.SCENE_SAMPLING)
    st["sigma"] = np.full(2, st.pop("sigma_fraction") * np.abs(c["u"]).max())
    first_plan = []
    with plant.SamplingPolicy(c["model"], 3, H, c["h"], c["mu"], ref, u0, **st) as pol:
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
    print(f"executed cost under the sampling policy {J_mpc.tolist()}, under open-loop replay of the step-0 plan {J_open.tolist()}")
    assert (J_mpc < J_open).all(), f"the sampling policy {J_mpc.tolist()} against open loop {J_open.tolist()}"


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
        with plant.SamplingPolicy(model, pst.B, pst.T, h, mu, ref, u0, n_samples=4, sigma=np.array([0.002, 0.01]), n_iter=pst.ITERS, seed=3, **lim) as pol:
            for s in range(2):
                out[f"step {s}: u"] = pol.control(q1, v1)
                out.update(pst.arrays(pol.last, f"step {s}: "))
            out.update(zip(("plan u", "plan q", "plan gamma", "plan b", "plan status", "plan iters"), pol.plan()))
        return out

    print("cimpc_plant_sampler_create, _control, _plan:", pst.loop_pairs(run, with_w=False), "arrays compared")
