"""The line search and iLQR on the device (csrc/plant_linesearch.hip: `RolloutTape.linesearch`, `TrackingCost`, `plant.ilqr`; DESIGN.md
section 3, item 3f) against the calls they replace and against a known answer.  Shapes: those of `plant_gradient_cases.ROLLOUTS`
(hopper_2D B 3 T 14 - with a per-robot disturbance schedule, per-robot friction and per-robot terrains -, particle B 1 T 14 on its bowl, quadruped B 2 T 6,
centroidal_quadruped_wall B 1 T 2, the two-wavefront step), at most three step lengths.

  1. one launch of n_alpha candidates = n_alpha closed-loop `rollout_tape` calls on B robots, bit for bit; J = `TrackingCost.evaluate`
  2. alpha = 0 retraces the parent, J = J_nom, and the new tape answers `lqr` and `vjp` as the parent's does
  3. the returned tape is the open-loop tape of the chosen controls; lin_q, lin_r are the host's
  4. a forced rejection (J_nom = -inf) leaves that robot's rows and tape blocks the parent's and every other robot untouched
  5. flight: one full iLQR step lands on the longdouble LQ optimum; the bounds are 10 x the gaps of the CPU restatement
     (`plant_linesearch_cases.flight_gaps_cpu`), never a figure of the device
  6. through contact: four iLQR iterations on the hoppers keep Armijo's inequality, never increase J, leave rejected robots alone, and
     the returned controls reproduce the returned trajectory in an open-loop `rollout`

Measured figures: tests/README_plant_linesearch.md.
"""
import functools

import numpy as np
import pytest

import plant_gradient_cases as pgc
import plant_linesearch_cases as plc
import plant_riccati_cases as prc
import plant_staging_cases as pst

pytestmark = pytest.mark.gpu
ALPHAS = (1.0, 0.3, 0.0)


def _kw(which):
    """The rollout keywords of a case: every column of θ on the tape; hopper_2D under a per-robot disturbance schedule held 7 steps, every
    hopper on a terrain of its own."""
    c = pgc.rollout_case(which)
    nw, nth = pgc.dims(c["model"])[4], pgc.dims(c["model"])[6]
    B = c["q1"].shape[0]
    w, w_hold, terrain = np.zeros((1, nw)), 1, c["terrain"]
    if which == "hopper_2D":
        w, w_hold, terrain = 1e-3 * np.random.default_rng(3).standard_normal((2, B, nw)), 7, ["flat_2D_lc", "sine3_2D_lc", "sine1_2D_lc"]
    return dict(terrain=terrain, w=w, w_hold=w_hold, grad_cols=nth)


def _args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


@functools.lru_cache(maxsize=None)
def _parent(which):
    """The nominal of a case, once per process: dict(c, q, ua, gamma, b, tape, cost, J, lq, lr, gains); the tape stays open."""
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case(which)
    nq, nu = pgc.dims(c["model"])[:2]
    ok, q, ua, gamma, b, status, iters, tape = plant.rollout_tape(*_args(c), **_kw(which))
    T, B = ua.shape[:2]
    rng = np.random.default_rng([7, nq, nu, T])
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step=which == "particle")
    x = np.concatenate([q[:-1], q[1:]], axis=2)
    x_goal = x + 0.02 * rng.standard_normal(x.shape) if B > 1 else (x + 0.02 * rng.standard_normal(x.shape))[:, 0]      # per robot, or shared
    u_goal = None if which == "quadruped" else ua[:, 0] * 0.5
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    J, lq, lr = cost.evaluate(q, ua)
    gains = tape.lqr(Q, R, Qf, q=lq, r=lr, rho=1e-3)
    assert gains.status.tolist() == [0] * B and np.isfinite(J).all()
    for a in (q, ua, gamma, b, J, lq, lr):
        a.setflags(write=False)
    return dict(c=c, q=q, ua=ua, gamma=gamma, b=b, status=status, iters=iters, tape=tape, cost=cost, J=J, lq=lq, lr=lr, gains=gains, Q=Q, R=R, Qf=Qf)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what} differs"


def _tape_answers(tape, Q, R, Qf, lq, lr, seed=0):
    """What a tape says: `lqr` with linear terms and a `vjp` of random cotangents, as a dict of arrays."""
    mid_dims = pgc.dims(tape.model)
    nq, nu, nc, nb = mid_dims[:4]
    rng = np.random.default_rng([seed, tape.T, tape.B])
    g = tape.lqr(Q, R, Qf, q=lq, r=lr, rho=1e-3)
    v = tape.vjp(gq=rng.standard_normal((tape.T + 2, tape.B, nq)), ggamma=rng.standard_normal((tape.T, tape.B, nc)), gb=rng.standard_normal((tape.T, tape.B, nb)))
    out = dict(K=g.K, k=g.k, P0=g.P0, p0=g.p0, dV=g.dV, lq_status=g.status, lq_cut=g.n_cut, g_q0=v.g_q0, g_q1=v.g_q1, u_step=v.u_step, n_cut=v.n_cut,
               grad_status=tape.grad_status)
    for key in ("w_step", "g_mu", "g_h"):
        if getattr(v, key) is not None:
            out[key] = getattr(v, key)
    return out


ROBOT_FIRST = ("P0", "p0", "dV", "lq_status", "lq_cut", "g_q0", "g_q1", "n_cut", "g_mu", "g_h")      # the answers whose leading axis is the robot


def _robot(key, a, b):
    """Robot b's part of an answer array."""
    return a[b] if key in ROBOT_FIRST else a[:, b]


# ---- 1. one launch equals n_alpha launches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_one_launch_equals_one_closed_loop_rollout_per_step_length(which):
    from contactimplicitmpc.jl_amd import plant
    p = _parent(which)
    c, tape, gains, cost = p["c"], p["tape"], p["gains"], p["cost"]
    B = p["ua"].shape[1]
    open_door = np.full(B, np.inf)      # every converged candidate with a finite J is acceptable: the call returns it
    with_all = tape.linesearch(gains, p["q"], p["ua"], cost, open_door, ALPHAS)
    assert with_all.J.shape == (3, B) and with_all.ok.shape == (3, B)
    with_all.tape.close()
    compared = 0
    for ci, a in enumerate(ALPHAS):
        one = tape.linesearch(gains, p["q"], p["ua"], cost, open_door, (a,))
        one.tape.close()
        ok, q, ua, gamma, b, status, iters, ref_tape, fb_err = plant.rollout_tape(c["model"], c["q1"], c["v1"], p["ua"] + a * gains.k, c["h"], c["mu"],
                                                                                   feedback=gains.feedback(p["q"]), **_kw(which))
        ref_tape.close()
        J_ref = cost.evaluate(q, ua)[0]
        _same(one.J[0], J_ref, f"{which} alpha {a}: J")
        _same(with_all.J[ci], one.J[0], f"{which} alpha {a}: J of the three-alpha call")
        conv = status.all(axis=0) & np.isfinite(J_ref)
        assert one.ok[0].tolist() == conv.tolist() and with_all.ok[ci].tolist() == conv.tolist()
        assert one.choice.tolist() == np.where(conv, 0, -1).tolist()
        assert conv.all(), "every candidate of these cases converges: a rejected one would come back as the parent's rows and escape the comparison below"
        print(f"{which} alpha {a}: J {one.J[0]}, converged {conv.tolist()}")
        for rb in range(B):
            compared += 1
            for name, got, ref in (("q", one.q, q), ("u_applied", one.u_applied, ua), ("gamma", one.gamma, gamma), ("b", one.b, b),
                                   ("status", one.status, status), ("iters", one.iters, iters)):
                _same(got[:, rb], ref[:, rb], f"{which} alpha {a} robot {rb}: {name}")
    assert compared == 3 * B


# ---- 2. alpha = 0 retraces the parent ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_alpha_zero_retraces_the_parent(which):
    p = _parent(which)
    ls = p["tape"].linesearch(p["gains"], p["q"], p["ua"], p["cost"], p["J"], (0.0,), armijo=0.0)
    with ls.tape:
        _same(ls.J[0], p["J"], f"{which}: J")
        assert ls.choice.tolist() == [0] * p["ua"].shape[1]      # J <= J_nom + 0 holds with equality
        for name in ("q", "gamma", "b"):
            _same(getattr(ls, name), p[name], f"{which}: {name}")
        _same(ls.u_applied, p["ua"], f"{which}: u_applied")
        _same(ls.lin_q, p["lq"], f"{which}: lin_q"); _same(ls.lin_r, p["lr"], f"{which}: lin_r")
        mine, parents = (_tape_answers(t, p["Q"], p["R"], p["Qf"], p["lq"], p["lr"]) for t in (ls.tape, p["tape"]))
    for key in parents:
        _same(mine[key], parents[key], f"{which}: {key} of the new tape")


# ---- 3. the returned tape is the chosen trajectory's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_the_returned_tape_is_the_open_loop_tape_of_the_chosen_controls(which):
    from contactimplicitmpc.jl_amd import plant
    p = _parent(which)
    c = p["c"]
    ls = p["tape"].linesearch(p["gains"], p["q"], p["ua"], p["cost"], np.full(p["J"].shape, np.inf), (0.3, 1.0))
    J, lq, lr = p["cost"].evaluate(ls.q, ls.u_applied)
    _same(ls.lin_q, lq, f"{which}: lin_q"); _same(ls.lin_r, lr, f"{which}: lin_r")
    assert (ls.choice >= 0).all()
    _same(ls.J[ls.choice, np.arange(len(J))], J, f"{which}: J of the chosen")
    ok, q, ua, gamma, b, status, iters, ref_tape = plant.rollout_tape(c["model"], c["q1"], c["v1"], ls.u_applied, c["h"], c["mu"], **_kw(which))
    _same(ls.q, q, f"{which}: the open-loop rollout of the chosen controls")
    with ls.tape, ref_tape:
        mine, refs = (_tape_answers(t, p["Q"], p["R"], p["Qf"], lq, lr, seed=1) for t in (ls.tape, ref_tape))
    for key in refs:
        _same(mine[key], refs[key], f"{which}: {key}")


# ---- 4. rejection ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pgc.ROLLOUTS)
def test_a_rejected_robot_keeps_the_parents_rows_and_blocks(which):
    p = _parent(which)
    B = p["ua"].shape[1]
    rb = B - 1
    J_nom = np.full(B, np.inf)
    rows = (p["gamma"], p["b"], p["status"], p["iters"])
    free = p["tape"].linesearch(p["gains"], p["q"], p["ua"], p["cost"], J_nom, (0.3, 0.0), parent_rows=rows)
    J_nom[rb] = -np.inf
    forced = p["tape"].linesearch(p["gains"], p["q"], p["ua"], p["cost"], J_nom, (0.3, 0.0), parent_rows=rows)
    assert forced.choice[rb] == -1 and not forced.ok[:, rb].any()
    _same(forced.J, free.J, f"{which}: J")
    with free.tape, forced.tape:
        a_free, a_forced, a_parent = (_tape_answers(t, p["Q"], p["R"], p["Qf"], p["lq"], p["lr"], seed=2) for t in (free.tape, forced.tape, p["tape"]))
    for name, parent in (("q", p["q"]), ("u_applied", p["ua"]), ("gamma", p["gamma"]), ("b", p["b"]), ("status", p["status"]), ("iters", p["iters"]),
                         ("lin_q", p["lq"]), ("lin_r", p["lr"])):
        _same(getattr(forced, name)[:, rb], parent[:, rb], f"{which}: {name} of the rejected robot")
        for other in range(B - 1):
            _same(getattr(forced, name)[:, other], getattr(free, name)[:, other], f"{which}: {name} of robot {other}")
    for key in a_parent:
        _same(_robot(key, a_forced[key], rb), _robot(key, a_parent[key], rb), f"{which}: {key} of the rejected robot")
        for other in range(B - 1):
            _same(_robot(key, a_forced[key], other), _robot(key, a_free[key], other), f"{which}: {key} of robot {other}")


def test_a_rejected_robot_without_parent_rows_gets_no_other_trajectorys():
    p = _parent("hopper_2D")
    ls = p["tape"].linesearch(p["gains"], p["q"], p["ua"], p["cost"], np.array([np.inf, -np.inf, np.inf]), (0.3,))
    ls.tape.close()
    assert ls.choice.tolist() == [0, -1, 0]
    assert np.isnan(ls.gamma[:, 1]).all() and np.isnan(ls.b[:, 1]).all() and (ls.status[:, 1] == -1).all() and (ls.iters[:, 1] == -1).all()
    assert np.isfinite(ls.gamma[:, [0, 2]]).all() and (ls.status[:, [0, 2]] == 1).all()


# ---- what the entry refuses once it has a tape ---------------------------------------------------------------------------------------------------
def test_the_entry_refuses_what_needs_a_tape_to_see():
    """The refusals behind the tape's B and T, each by its own reason (`cimpc_last_error(NULL)`), and the wrapper's own for a closed-loop tape."""
    import dataclasses
    from contactimplicitmpc.jl_amd import _lib, plant
    p = _parent("hopper_2D")
    tape, gains, cost, B = p["tape"], p["gains"], p["cost"], 3

    def poisoned(a, at):
        a = np.array(a)
        a[at] = np.nan
        return a
    calls = {"a non-finite entry of K": lambda: tape.linesearch(dataclasses.replace(gains, K=poisoned(gains.K, (5, 1, 0, 3))), p["q"], p["ua"], cost, p["J"], (1.0,)),
             "a non-finite entry of k": lambda: tape.linesearch(dataclasses.replace(gains, k=poisoned(gains.k, (0, 2, 1))), p["q"], p["ua"], cost, p["J"], (1.0,)),
             "a non-finite entry of q_nom": lambda: tape.linesearch(gains, poisoned(p["q"], (15, 0, 2)), p["ua"], cost, p["J"], (1.0,)),
             "a non-finite entry of u_nom": lambda: tape.linesearch(gains, p["q"], poisoned(p["ua"], (13, 2, 1)), cost, p["J"], (1.0,)),
             "an argument that cimpc_plant_rollout_tape refuses for the tape's B robots": lambda: tape.linesearch(gains, p["q"], p["ua"], cost, p["J"], (1.0,), w_hold=0),
             "n_x of the cost neither 1 nor B": lambda: _two_goal_columns(tape, gains, p)}
    for reason, call in calls.items():
        with pytest.raises(_lib.CimpcError):
            call()
        assert _lib.load().cimpc_last_error(None).decode() == "cimpc_plant_tape_linesearch: " + reason
    c = p["c"]
    *_, closed_loop, _ = plant.rollout_tape(c["model"], c["q1"], c["v1"], p["ua"], c["h"], c["mu"], feedback=gains.feedback(p["q"]), **_kw("hopper_2D"))
    with closed_loop, pytest.raises(ValueError, match="open-loop"):
        closed_loop.linesearch(gains, p["q"], p["ua"], cost, p["J"], (1.0,))
    ok = tape.linesearch(gains, p["q"], p["ua"], cost, p["J"], (0.0,))      # the tape and the workspace are as they were
    ok.tape.close()
    _same(ok.J[0], p["J"], "J after the refusals")


def _two_goal_columns(tape, gains, p):
    """The line search with a cost whose goals have two columns for three robots: only the library can see that (the struct is made by hand)."""
    from contactimplicitmpc.jl_amd import plant

    class TwoColumns(plant.TrackingCost):
        def _struct(self, nq, nu, B, T):
            cc, keep = super()._struct(nq, nu, B, T)
            cc.n_x = 2
            return cc, keep
    cost = TwoColumns(p["Q"], p["R"], p["Qf"])
    return tape.linesearch(gains, p["q"], p["ua"], cost, p["J"], (1.0,))


# ---- 5. flight: a known answer -------------------------------------------------------------------------------------------------------------
def test_one_full_step_in_flight_lands_on_the_lq_optimum():
    """Measured: see tests/README_plant_linesearch.md."""
    from contactimplicitmpc.jl_amd import plant
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    gu_cpu, gj_cpu = plc.flight_gaps_cpu()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    *_, q0, ua0, _, _, _, _, G = plant.rollout(*_args(case), terrain=case["terrain"], diff_sol=True)
    J_nom, lq, lr = cost.evaluate(q0, ua0)
    res = plant.ilqr(*_args(case), cost, alphas=(1.0,), max_iter=1, rho0=0.0, terrain=case["terrain"])
    res.tape.close()
    assert res.accepted.shape == (1, 2) and res.accepted.all()
    _same(res.J0, J_nom, "the first nominal's cost")
    gu, gj = plc.flight_gaps(G.dz, ua0, res.u, lq, lr, J_nom, res.J[0], res.gains.dV, Q, R, Qf)
    print(f"flight: controls {gu:.3e} from the LQ optimum (CPU restatement {gu_cpu:.3e}, bound {10 * gu_cpu:.3e}); "
          f"decrease {gj:.3e} from dV1 + dV2 (CPU {gj_cpu:.3e}, bound {10 * gj_cpu:.3e})")
    assert gu <= 10 * gu_cpu, f"controls: {gu:.3e} > {10 * gu_cpu:.3e}"
    assert gj <= 10 * gj_cpu, f"decrease: {gj:.3e} > {10 * gj_cpu:.3e}"


# ---- 6. through contact ------------------------------------------------------------------------------------------------------------------------
def test_ilqr_through_contact_on_the_hoppers():
    from contactimplicitmpc.jl_amd import plant
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    cpu = plc.ilqr_cpu(c, Q, R, Qf, x_goal, u_goal, (1.0, 0.5, 0.25), 1, rho=1e-6)[0]
    assert cpu["accepted"].all(), "the cost is chosen so that the CPU restatement accepts iteration 1 for all three hoppers"
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)
    armijo = 1e-4
    # after every iteration: the loop itself, cut short - the rows a rejected robot must keep are the previous call's
    runs = [plant.ilqr(*_args(c), cost, alphas=(1.0, 0.5, 0.25), max_iter=n, rho0=1e-6, armijo=armijo, tol=0.0) for n in (1, 2, 3, 4)]
    for r in runs:
        r.tape.close()
    res = runs[-1]
    n_it, B = res.J.shape
    print(f"hoppers: J0 {res.J0}, J {res.J.tolist()}, alpha {res.alpha.tolist()}, rho {res.rho.tolist()}, accepted {res.accepted.tolist()}")
    assert res.accepted.any(), "no robot accepted any iteration"
    assert res.accepted[0].all(), "iteration 1 is accepted for all three hoppers, as on the CPU"
    J_prev = res.J0
    for i in range(n_it):
        _same(runs[i].J[i], res.J[i], f"iteration {i + 1} of the shorter run")
        assert (res.J[i] <= J_prev).all(), "J increased"
        for b in range(B):
            if res.accepted[i, b]:
                dV, a = runs[i].gains.dV[b], res.alpha[i, b]      # the gains of iteration i + 1 are the last ones of the run that stops there
                assert res.J[i, b] <= J_prev[b] + armijo * (a * dV[0] + (a * a) * dV[1]), f"Armijo fails at iteration {i + 1}, robot {b}"
            else:
                assert res.J[i, b] == J_prev[b] and np.isnan(res.alpha[i, b])
                if i > 0:
                    for name in ("u", "q", "gamma", "b"):
                        _same(getattr(runs[i], name)[:, b], getattr(runs[i - 1], name)[:, b], f"{name} of rejected robot {b} at iteration {i + 1}")
        J_prev = res.J[i]
    ok, q, ua, *_ = plant.rollout(c["model"], c["q1"], c["v1"], res.u, c["h"], c["mu"])
    _same(q, res.q, "the open-loop rollout of the returned controls")
    _same(cost.evaluate(res.q, res.u)[0], res.J[-1], "the returned cost")


# ---- the optional staged arrays ----------------------------------------------------------------------------------------------------------------
def test_shared_absent_and_per_robot_arrays_give_the_same_bits():
    """`plant.ilqr`'s host loop: cimpc_plant_tape_linesearch_box and cimpc_plant_tape_lqr_box, iteration after iteration."""
    # the entry's optional staged arrays (csrc/plant_staging.h) at B = 2, T = 4, two step lengths, two iterations: mu, w and the limits shared
    # against the same values per robot, and no limits against infinite ones, every returned array bit for bit (tests/plant_staging_cases.py).
    from contactimplicitmpc.jl_amd import plant
    args, _, (Q, R, Qf, x_goal, u_goal) = pst.hopper()
    cost = plant.TrackingCost(Q, R, Qf, x_goal=x_goal, u_goal=u_goal)

    def run(mu, **kw):
        res = plant.ilqr(*args, mu, cost, device_loop=False, **pst.LOOP, **kw)
        out = pst.arrays(res)
        res.tape.close()
        return out

    print("cimpc_plant_tape_linesearch_box, cimpc_plant_tape_lqr_box:", pst.loop_pairs(run), "arrays compared")
