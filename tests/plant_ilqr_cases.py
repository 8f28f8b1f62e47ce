"""Restatements and cases shared by the tests of the device-resident iLQR loop (tests/test_plant_ilqr.py without a device,
tests/test_gpu_plant_ilqr.py on it, scripts/plant_ilqr_ab.py): the rules of DESIGN.md section 3, item 3h (csrc/plant_ilqr.h).

`rules_np` is the NumPy lines `plant.ilqr` runs between its backward pass and its line search, copied from the loop with one change:
rho is read from the ladder (`ladder`, the loop's own expression rho0 * float(rho_factor) ** level on the levels 0 .. max_iter) where the
loop evaluates the power.  `states` draws random robots and appends the edge states by hand.  `rollout_kw` restates the varied rollout
keywords of the line-search tests (a per-robot disturbance schedule held 7 steps, per-robot terrains; friction is per robot in the case
itself).  `bookkeeping` is the case whose HOST loop shows a rejection followed by an acceptance, a robot stopped by `small` beside one that
continues, a robot stopped by rho_max, and an early end.
"""
import functools

import numpy as np

import plant_gradient_cases as pgc
import plant_linesearch_cases as plc


def ladder(rho0, rho_factor, max_iter):
    return np.ascontiguousarray(rho0 * float(rho_factor) ** np.arange(max_iter + 1, dtype=np.int64), dtype=np.float64)


def rules_np(level, active, J, J_cand, choice, lq_status, alphas, lad, rho_max, tol):
    """One iteration's bookkeeping for B robots.  level (B,) ints, active (B,) bools, J (B,), J_cand (n_alpha, B), choice (B,) with -1 for
    none, lq_status (B,).  Returns dict(rho, J_nom, level, active, J, alpha, accepted): rho and J_nom as the stages before the line search
    get them, the rest after it; J is both the robot's new cost and the history's."""
    B = len(level)
    alphas = np.asarray(alphas, dtype=np.float64)
    with np.errstate(all="ignore"):
        rho = lad[level]
        J_nom = np.where(active & (lq_status == 0), J, -np.inf)
        accepted = choice >= 0
        J_new = np.where(accepted, J_cand[np.maximum(choice, 0), np.arange(B)], J)
        alpha = np.where(accepted, alphas[np.maximum(choice, 0)], np.nan)
        small = accepted & (J - J_new < tol * np.abs(J))
        level = np.where(accepted, np.maximum(level - 1, 0), np.where(active, level + 1, level))
        active = active & ~small & (lad[level] <= rho_max)
    return dict(rho=rho, J_nom=J_nom, level=level, active=active, J=J_new, alpha=alpha, accepted=accepted)


def states(seed, N, n_alpha, lad, rho_max, tol):
    """N random robots followed by the edge states: dict(level, active, J, J_cand (n_alpha, N'), choice, lq_status) and the names of the
    edge states in the order they were appended.  No state moves past the ladder's last entry (the entry point's precondition)."""
    rng = np.random.default_rng(seed)
    top = len(lad) - 1
    active = rng.random(N) < 0.7
    level = rng.integers(0, top + 1, N)
    J = np.abs(rng.standard_normal(N)) * 10.0 ** rng.integers(-3, 4, N)
    J[rng.random(N) < 0.05] *= -1.0
    # candidates near J, on either side, some equal, some far below (a decrease past tol |J|), a few not finite
    J_cand = J[None] * (1.0 - rng.choice([0.0, 1e-16, 1e-9, 1e-3, 0.5, -1e-3], (n_alpha, N)) * rng.random((n_alpha, N)))
    J_cand[rng.random((n_alpha, N)) < 0.05] = np.nan
    J_cand[rng.random((n_alpha, N)) < 0.02] = np.inf
    lq_status = np.where(rng.random(N) < 0.1, rng.integers(1, 9, N), 0)
    choice = np.where(active & (lq_status == 0) & (rng.random(N) < 0.6), rng.integers(0, n_alpha, N), -1)
    level = np.where((choice < 0) & active, np.minimum(level, top - 1), level)      # a rejection moves up: stay on the ladder
    s = dict(level=level, active=active, J=J, J_cand=J_cand, choice=choice, lq_status=lq_status)
    at_max = int(np.flatnonzero(lad == rho_max)[0])      # the ladder has rho_max as one of its entries
    edges = {
        "J = 0 with tol > 0, accepted at J_new = 0": dict(level=1, active=True, J=0.0, J_cand=0.0, choice=0, lq_status=0),
        "J_new = J exactly": dict(level=2, active=True, J=3.25, J_cand=3.25, choice=n_alpha - 1, lq_status=0),
        "J_new one ulp below J": dict(level=2, active=True, J=3.25, J_cand=np.nextafter(3.25, 0.0), choice=0, lq_status=0),
        "a rejection onto the last ladder entry": dict(level=top - 1, active=True, J=1.5, J_cand=2.0, choice=-1, lq_status=0),
        "accepted at the last ladder entry": dict(level=top, active=True, J=1.5, J_cand=0.5, choice=0, lq_status=0),
        "inactive at the last ladder entry": dict(level=top, active=False, J=1.5, J_cand=0.5, choice=-1, lq_status=0),
        "a rejection onto rho = rho_max exactly": dict(level=at_max - 1, active=True, J=1.5, J_cand=2.0, choice=-1, lq_status=0),
        "a rejection past rho_max": dict(level=at_max, active=True, J=1.5, J_cand=2.0, choice=-1, lq_status=0),
        "an acceptance down onto rho_max exactly": dict(level=at_max + 1, active=True, J=1.5, J_cand=1e-3, choice=0, lq_status=0),
        "a NaN J_cand on a rejected robot": dict(level=0, active=True, J=2.0, J_cand=np.nan, choice=-1, lq_status=0),
        "an inactive robot that is accepted nowhere": dict(level=3, active=False, J=2.0, J_cand=1.0, choice=-1, lq_status=0),
        "a backward pass that ended early": dict(level=0, active=True, J=2.0, J_cand=1.0, choice=-1, lq_status=5),
        "level 0 accepted stays at level 0": dict(level=0, active=True, J=2.0, J_cand=1e-9, choice=0, lq_status=0),
        "a negative J": dict(level=1, active=True, J=-2.0, J_cand=-2.5, choice=0, lq_status=0),
    }
    for e in edges.values():
        for key in ("level", "active", "J", "choice", "lq_status"):
            s[key] = np.append(s[key], e[key])
        s["J_cand"] = np.concatenate([s["J_cand"], np.full((n_alpha, 1), e["J_cand"])], axis=1)
    s["level"], s["choice"], s["lq_status"] = (s[k].astype(np.int64) for k in ("level", "choice", "lq_status"))
    s["active"] = s["active"].astype(bool)
    return s, list(edges)


# ---- the GPU cases ---------------------------------------------------------------------------------------------------------------------------
def args(c):
    return (c["model"], c["q1"], c["v1"], c["u"], c["h"], c["mu"])


def rollout_kw(which):
    """The varied rollout keywords of a case, as tests/test_gpu_plant_linesearch.py builds them: every column of θ on the tape; hopper_2D under a
    per-robot disturbance schedule held 7 steps, every hopper on a terrain of its own."""
    c = pgc.rollout_case(which)
    nw, nth = pgc.dims(c["model"])[4], pgc.dims(c["model"])[6]
    B = c["q1"].shape[0]
    w, w_hold, terrain = np.zeros((1, nw)), 1, c["terrain"]
    if which == "hopper_2D":
        w, w_hold, terrain = 1e-3 * np.random.default_rng(3).standard_normal((2, B, nw)), 7, ["flat_2D_lc", "sine3_2D_lc", "sine1_2D_lc"]
    return dict(terrain=terrain, w=w, w_hold=w_hold, grad_cols=nth)


CONTACT = dict(alphas=(1.0, 0.5, 0.25), rho0=1e-6, tol=0.0)      # the settings of the through-contact tests


@functools.lru_cache(maxsize=None)
def bookkeeping():
    """(case, (Q, R, Qf, x_goal, u_goal), the keywords of `plant.ilqr`) of the bookkeeping test: the hopper case with a goal per robot -
    robot 0's a millimetre along, robot 1's five centimetres, robot 2's thirty - under ONE step length, an Armijo factor near 1 (a step must
    deliver nearly all of the decrease its quadratic model promises), a tol that stops a robot whose accepted step takes less than nine tenths
    off its cost, and a rho_max between the ladder's entries 1 and 2 (two rejections in a row stop a robot).  On the device plant the host
    loop then runs three of its six iterations: robot 0 is accepted, rejected, accepted (small: stopped); robot 1 accepted, rejected,
    rejected (past rho_max: stopped); robot 2 accepted with a small decrease at once (stopped while the other two go on)."""
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, _, u_goal = plc.contact_cost()
    T = c["T"]
    goals = c["q1"] + np.array(BOOKKEEPING_GOALS)[:, None] * np.array([1.0, 0.0, 0.0, 0.0])
    x_goal = np.broadcast_to(np.concatenate([goals, goals], axis=1), (T + 1, 3, 8)).copy()
    return c, (Q, R, Qf, x_goal, u_goal), dict(BOOKKEEPING_KW)


BOOKKEEPING_GOALS = (0.001, 0.05, 0.3)
BOOKKEEPING_KW = dict(alphas=(1.0,), armijo=0.97, rho0=1e-3, rho_factor=100.0, rho_max=1.0, tol=0.9, max_iter=6)


def events(res, max_iter, rho0, rho_factor, rho_max, tol, **_):
    """Which bookkeeping events a run's history shows, by replaying the loop's rules on it (J0, J, accepted are the run's; level and active
    are not returned, so they are rebuilt): dict(up_then_down, small_beside_active, stopped_by_rho_max, early_end) of bools."""
    lad = ladder(rho0, rho_factor, max_iter)
    n_it, B = res.accepted.shape
    level, active, J = np.zeros(B, dtype=np.int64), np.ones(B, dtype=bool), res.J0
    seen = dict(up_then_down=False, small_beside_active=False, stopped_by_rho_max=False, early_end=False)
    went_up = np.zeros(B, dtype=bool)
    for i in range(n_it):
        assert active.any(), "the loop went on without an active robot"
        acc, J_new = res.accepted[i], res.J[i]
        assert np.array_equal(res.rho[i], lad[level]), "the history's rho is not the replay's"
        small = acc & (J - J_new < tol * np.abs(J))
        seen["up_then_down"] |= bool((went_up & acc).any())
        went_up = ~acc & active
        level = np.where(acc, np.maximum(level - 1, 0), np.where(active, level + 1, level))
        over = lad[level] > rho_max
        seen["stopped_by_rho_max"] |= bool((active & ~small & over).any())
        after = active & ~small & ~over
        seen["small_beside_active"] |= bool((active & small).any() and after.any())
        active, J = after, J_new
    seen["early_end"] = n_it < max_iter and not active.any()
    return seen
