"""Restatements and cases shared by the tests of the receding-horizon iLQR policy (tests/test_plant_mpc.py without a device,
tests/test_gpu_plant_mpc.py on it, scripts/closed_loop_ilqr_mpc.py): the rules of DESIGN.md section 3, item 3j
(csrc/plant_mpc.h).

`x_rows`, `u_rows`, `warm_rows` are the index rules in NumPy.  `compose` is the definition a control step is held to: `plant.ilqr` with
`device_loop=True` on the goal window of the step, from the shifted plan.  The scenes are built from the cases of the earlier items: the
three hoppers of `plant_gradient_cases.rollout_case`, the contact cost and the flight case of `plant_linesearch_cases`, the flight limits
of `plant_boxqp_cases`, the bookkeeping settings of `plant_ilqr_cases`.
"""
import numpy as np

import plant_gradient_cases as pgc
import plant_linesearch_cases as plc


def x_rows(s, H, L):
    return np.minimum(s + np.arange(H + 1), L)


def u_rows(s, H, L):
    return np.minimum(s + np.arange(H), L - 1)


def warm_rows(shift, H):
    return np.minimum(np.arange(H) + shift, H - 1)


def compose(plant, model, q1, v1, u_warm, h, mu, ref, s, H, n_iter, **kw):
    """Control step s by the calls that exist without the policy: (u (B, nu), the `ILQRResult`, its tape closed)."""
    res = plant.ilqr(model, q1, v1, u_warm, h, mu, ref.window(s, H), max_iter=n_iter, device_loop=True, **kw)
    res.tape.close()
    return res.u[0], res


def true_step(plant, model, q0, q1, u, mu, h, w=None, terrain=None):
    """One step of the TRUE plant, robot by robot where frictions differ (`plant_step` takes one coefficient): q2 (B, nq)."""
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64).reshape(-1), (q1.shape[0],))
    q2 = np.zeros_like(q1)
    for b in range(q1.shape[0]):
        ter = terrain if terrain is None or isinstance(terrain, str) else terrain[b]
        out = plant.plant_step(model, q0[b:b + 1], q1[b:b + 1], u[b:b + 1], float(mu[b]), h, w=None if w is None else w[b:b + 1], terrain=ter)
        q2[b] = out[0][0]
    return q2


def hopper_reference(plant, L=10, per_robot=False):
    """The contact cost's weights with L stages of goals: the body carried from where it starts to 5 cm further along, one goal per stage; per
    robot, robot b's goal lies (1 + b / 2) times as far."""
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, _, _ = plc.contact_cost()
    along = 0.05 * np.arange(L + 1)[:, None] / L * np.array([1.0, 0.0, 0.0, 0.0])
    if per_robot:
        goal = c["q1"][None] + along[:, None, :] * (1.0 + 0.5 * np.arange(3))[None, :, None]      # (L + 1, 3, 4)
    else:
        goal = c["q1"][0] + along                                                                  # (L + 1, 4)
    return plant.TrackingReference(Q, R, Qf, x_ref=np.concatenate([goal, goal], axis=-1), u_ref=np.zeros((L, 2)))


def bookkeeping_reference(plant):
    """The goals per robot of `plant_ilqr_cases.bookkeeping`, held: L = 1."""
    import plant_ilqr_cases as pic
    c, (Q, R, Qf, x_goal, u_goal), kw = pic.bookkeeping()
    return c, plant.TrackingReference(Q, R, Qf, x_ref=x_goal[:2], u_ref=u_goal[:1]), kw


def flight_reference(plant):
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    return case, plant.TrackingReference(Q, R, Qf, x_ref=x_goal[:3, 0], u_ref=u_goal[:2, 0])


# ---- the closed-loop scene of scripts/closed_loop_ilqr_mpc.py and of the test that the policy controls --------------------------------------
SCENE_STEPS = 20                               # S control steps, and the horizon H: the step-0 plan covers the whole run
SCENE_IMPULSE = (np.array([0.4, 0.0]), 6)      # w of the ImpulseDisturbance (hopper_2D: nw = 2) and the one simulator step it acts at; chosen once
SCENE_TRUE_MU = 0.5                            # the true plant's friction for every hopper; the planner believes the rollout case's (0.8, 0.3, 0.05)
SCENE_KW = dict(n_iter=2, alphas=(1.0, 0.5, 0.25), rho0=1e-6, tol=0.0)


def scene(plant):
    """(case, reference, first plan (H, B, nu), the policy's keywords): the three hoppers of the rollout case asked to carry the body 5 cm
    along over L = SCENE_STEPS stages and to hold it there; the first plan is the case's controls, the last row held to H = SCENE_STEPS."""
    c = pgc.rollout_case("hopper_2D")
    ref = hopper_reference(plant, L=SCENE_STEPS)
    u0 = c["u"][np.minimum(np.arange(SCENE_STEPS), c["T"] - 1)]
    return c, ref, u0, dict(SCENE_KW)


def executed_cost(ref, q, u):
    """`TrackingCost` of an executed closed-loop trajectory q (S + 2, B, nq), u (S, B, nu) against the reference from step 0: (B,)."""
    return ref.window(0, u.shape[0]).evaluate(q, u)[0]


def run_scene(plant, policy):
    """`simulate` on the scene's true plant (its own friction, the impulse): policy is a callable of q (B, nq) -> q (S + 2, B, nq), u (S, B, nu)."""
    c = pgc.rollout_case("hopper_2D")
    dist = plant.ImpulseDisturbance([SCENE_IMPULSE[0]], [SCENE_IMPULSE[1]])
    ok, q, u, *_ = plant.simulate(c["model"], policy, c["q1"], c["v1"], SCENE_STEPS, c["h"], SCENE_TRUE_MU, disturbances=dist)
    return q, u


def replay(u_plan):
    """The open-loop policy that replays a plan (H, B, nu) row by row, the last row held."""
    t = [0]

    def policy(q):
        u = u_plan[min(t[0], u_plan.shape[0] - 1)]
        t[0] += 1
        return u
    return policy
