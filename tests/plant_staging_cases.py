"""The optional staged arrays of the plant's stage entries (csrc/plant_staging.h), at the smallest shape that has more than one robot, step,
step length and iteration: two of the hoppers of `plant_gradient_cases.rollout_case("hopper_2D")` over T = 4 steps, two step lengths, two
iterations (two segments for multiple shooting).  An entry stages mu, w and the control limits only where they are given per robot - a
shared value rides in the call or in the plant workspace - and stages no limits at all where none are given.  So each entry is run

  shared against per robot     one mu, one w schedule and one row of (binding) limits for every robot, against the same values repeated B times;
  absent against infinite      no w and no limits, against no w and limits at -inf, +inf, which every entry defines as the unlimited call,

and every array either pair returns is compared bit for bit (`same_arrays`)."""
import dataclasses

import numpy as np

import plant_gradient_cases as pgc
import plant_linesearch_cases as plc

B, T, ALPHAS, ITERS, SEGMENTS = 2, 4, (1.0, 0.5), 2, 2
LOOP = dict(alphas=ALPHAS, max_iter=ITERS, rho0=1e-6, tol=0.0)


def hopper():
    """(model, q1, v1, u, h) of the first B hoppers over T steps, their shared friction, and the contact cost's weights with T + 1 goals."""
    c = pgc.rollout_case("hopper_2D")
    Q, R, Qf, x_goal, u_goal = plc.contact_cost()
    return (c["model"], c["q1"][:B], c["v1"][:B], c["u"][:T, :B], c["h"]), float(c["mu"][0]), (Q, R, Qf, x_goal[:T + 1], u_goal[:T])


def shared_and_per_robot(with_w=True):
    """Two keyword sets that state the same problem: (mu, dict(w=, u_lo=, u_hi=)) shared, and per robot.  The limits bind: the hoppers' leg
    force is 0.05 and 0.04 over these steps."""
    nu, nw = 2, 2
    mu = float(pgc.rollout_case("hopper_2D")["mu"][0])
    w = 1e-3 * np.random.default_rng(5).standard_normal((1, nw))
    lo, hi = np.array([-0.01, 0.0]), np.array([0.01, 0.045])
    one = dict(u_lo=lo, u_hi=hi)
    each = dict(u_lo=np.tile(lo, (B, 1)), u_hi=np.tile(hi, (B, 1)))
    if with_w:
        one["w"], each["w"] = w, np.tile(w[:, None, :], (1, B, 1))
    assert each["u_lo"].shape == (B, nu)
    return (mu, one), (np.full(B, mu), each)


def absent_and_infinite():
    nu = 2
    return dict(), dict(u_lo=np.full(nu, -np.inf), u_hi=np.full(nu, np.inf))


def arrays(res, prefix=""):
    """Every array a result holds, by name: its own fields, those of the results nested in it, and its tape's gradient status."""
    out = {}
    for f in dataclasses.fields(res):
        v = getattr(res, f.name)
        if isinstance(v, np.ndarray):
            out[prefix + f.name] = v
        elif dataclasses.is_dataclass(v):
            out.update(arrays(v, prefix + f.name + "."))
        elif hasattr(v, "grad_status"):
            out[prefix + f.name + ".grad_status"] = np.asarray(v.grad_status)
    return out


def same_arrays(a: dict, b: dict, what: str, least: int, extras=()):
    """b holds a's arrays bit for bit; what it holds beyond them is named in `extras` (the limited pass returns its mask, P0 and p0), and a
    mask among them is zero throughout."""
    assert set(a) <= set(b) and set(b) - set(a) <= set(extras) and len(a) >= least, f"{what}: {sorted(a)} against {sorted(b)}"
    for key in set(b) - set(a):
        assert np.isfinite(b[key]).all() and not (key.endswith("clamped") and np.any(b[key])), f"{what}: {key}"
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {key} {x.shape} {x.dtype} against {y.shape} {y.dtype}"
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs"


def loop_pairs(run, with_w=True):
    """run(mu, **kw) -> dict of arrays, for both pairs; returns the number of arrays compared."""
    (mu1, one), (muB, each) = shared_and_per_robot(with_w)
    shared, per_robot = run(mu1, **one), run(muB, **each)
    same_arrays(shared, per_robot, "shared against per robot", 8)
    none, inf = absent_and_infinite()
    absent, infinite = run(mu1, **none), run(mu1, **inf)
    same_arrays(absent, infinite, "no limits against infinite limits", 8, extras=("gains.clamped", "gains.P0", "gains.p0"))      # infinite limits never clamp
    limited = [k for k in absent if k in shared and shared[k].tobytes() != absent[k].tobytes()]
    assert limited, "the limits of the first pair bind nowhere: the pair would not see them"
    return len(shared) + len(absent)
