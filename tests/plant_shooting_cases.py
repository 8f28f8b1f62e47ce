"""The cases of the multiple-shooting tests (tests/test_plant_shooting.py without a device, tests/test_gpu_plant_shooting.py on it; DESIGN.md
section 3, item 3l): the particles in flight of `plant_linesearch_cases.flight_case` (B 2, T 8, M 1, 2, 4, 8), the hoppers through contact of
`plant_gradient_cases.rollout_case` cut to T 12 (B 3, M 1, 2, 3, 4, 12) under per-robot friction, per-robot terrains and a per-robot
disturbance schedule held 5 steps - which divides no segment length -, and the wall quadruped (nu 12, B 1, T 2, M 1, 2).  M = T (L = 1) is
among the segmentations of each: the smallest shape at which node rows, the defect rows L and L + 1 and the time offset can be mixed up.
"""
import functools

import numpy as np

import plant_gradient_cases as pgc
import plant_linesearch_cases as plc
import plant_riccati_cases as prc
import plant_shooting_ref as psr

SEGMENTS = {"flight": (1, 2, 4, 8), "hopper_2D": (1, 2, 3, 4, 12), "centroidal_quadruped_wall": (1, 2)}
CASES = [(which, M) for which, Ms in SEGMENTS.items() for M in Ms]
HOLD_W = 5


@functools.lru_cache(maxsize=None)
def problem(which):
    """dict(model, q1, v1, u (T, B, nu), h, mu (B,), T, kw): kw the rollout keywords every call of the case shares (terrain, w, w_hold, grad_cols)."""
    if which == "flight":
        c = dict(plc.flight_case()[0])
        c["u"] = 0.05 * np.random.default_rng(11).standard_normal(c["u"].shape)
    else:
        c = dict(pgc.rollout_case(which))
    if which == "hopper_2D":
        c["T"], c["u"] = 12, np.ascontiguousarray(c["u"][:12])
    nw, nth = pgc.dims(c["model"])[4], pgc.dims(c["model"])[6]
    B = c["q1"].shape[0]
    kw = dict(terrain=c["terrain"], w=None, w_hold=1, grad_cols=nth)
    if which == "hopper_2D":
        kw.update(terrain=["flat_2D_lc", "sine3_2D_lc", "sine1_2D_lc"], w=1e-3 * np.random.default_rng(3).standard_normal((3, B, nw)), w_hold=HOLD_W)
    c["kw"] = kw
    return c


def nodes_of(q1, v1, h):
    """nodes (M, B, 2nq) from the segments' (q1, v1) (M, B, nq) as `rollout` forms its first two rows: [q1 - h v1; q1]."""
    return np.ascontiguousarray(np.concatenate([q1 - h * v1, q1], axis=2))


def displaced_starts(c, q, M, seed, size=1e-3):
    """(q1, v1) (M, B, nq) of M segments: segment 0 the case's own start, the others the sequential trajectory q's rows displaced by a seeded
    `size` - so that every defect is nonzero and node j is not where segment j - 1 ends."""
    T, h = c["T"], c["h"]
    L = T // M
    rng = np.random.default_rng([seed, M, T])
    q1, v1 = q[1:T + 1:L].copy(), (q[1:T + 1:L] - q[0:T:L]) / h
    q1[1:] += size * rng.standard_normal(q1[1:].shape)
    v1[1:] += 10.0 * size * rng.standard_normal(v1[1:].shape)
    q1[0], v1[0] = c["q1"], c["v1"]
    return q1, v1


def virtual_robots(c, q1, v1, M):
    """The arguments of `plant.rollout` for the M B virtual robots of a segmentation, built on the host: (positional, keywords).  Robot
    j B + b starts from segment j's (q1, v1) and reads, at its step l, robot b's rows of global step j L + l."""
    T, B, kw = c["T"], c["q1"].shape[0], c["kw"]
    L = T // M
    nq = q1.shape[2]
    out = dict(terrain=kw["terrain"], grad_cols=kw["grad_cols"])
    if isinstance(kw["terrain"], list):
        out["terrain"] = kw["terrain"] * M
    if kw["w"] is not None:
        rows = np.minimum(np.arange(T) // kw["w_hold"], kw["w"].shape[0] - 1)
        out.update(w=psr.spread(np.broadcast_to(kw["w"], (kw["w"].shape[0], B, kw["w"].shape[2]))[rows], M), w_hold=1)
    u = psr.spread(np.broadcast_to(c["u"], (T, B, c["u"].shape[-1])), M)
    return (c["model"], q1.reshape(M * B, nq), v1.reshape(M * B, nq), u, c["h"], np.tile(c["mu"], M)), out


def cost_of(c, seed=0, per_step=False):
    """(Q, R, Qf, x_goal (T + 1, B, n), u_goal (T, B, m)) for a case: random symmetric positive definite weights and goals per robot."""
    nq, nu = pgc.dims(c["model"])[:2]
    T, B = c["T"], c["q1"].shape[0]
    rng = np.random.default_rng([seed, nq, nu, T])
    Q, R, Qf = prc.weights(rng, 2 * nq, nu, T, per_step)
    x0 = np.concatenate([c["q1"], c["q1"]], axis=1)
    return Q, R, Qf, x0[None] + 0.05 * rng.standard_normal((T + 1, B, 2 * nq)), 0.5 * rng.standard_normal((T, B, nu))


def random_segments(rng, nq, nu, T, B, M, gap=1e-2):
    """(qs (L + 2, M B, nq), u (T, B, nu)) with no plant behind them: segments that nearly join, `gap` apart at the nodes."""
    L = T // M
    path = np.cumsum(0.1 * rng.standard_normal((T + 2, B, nq)), axis=0)
    qs = np.zeros((L + 2, M * B, nq))
    for j in range(M):
        qs[:, j * B:(j + 1) * B] = path[j * L:j * L + L + 2] + gap * rng.standard_normal((1, B, nq))
    return qs, rng.standard_normal((T, B, nu))
