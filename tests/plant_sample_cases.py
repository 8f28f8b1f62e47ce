"""Restatements and cases shared by the tests of the sampling policy (tests/test_plant_sample.py without a device,
tests/test_gpu_plant_sample.py on it, scripts/closed_loop_sampling_mpc.py, scripts/plant_sample_ab.py): the rules of DESIGN.md section 3,
item 3k (csrc/plant_sample.h), in integer and float64 NumPy, every sum in the header's order.

`philox`, `deviate`, `eps`, `noise` restate the random bits and the deviate; `candidates` the candidate law; `update` eligibility, choice,
weights and the new plan (`math.exp` per element: the libm of the g++ build).  `compose` is the definition a control step is held to: the goal
window, the warm rows, the restated candidates, ONE `plant.rollout` of N B robots, `TrackingCost.evaluate`, the restated choice and update.
"""
import math

import numpy as np


M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
SQRT_1_5 = float.fromhex("0x1.3988e1409212ep+0")
assert SQRT_1_5 == math.sqrt(1.5)

# three known answers of Philox4x32-10: (counter, key, output)
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64: the four output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2      # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def deviate(words):
    """eps of the four output words: eight 16-bit fields, low half first, summed in order, then ONE product with sqrt(1.5) rounded."""
    s = np.zeros(np.shape(words[0]))
    for w in words:
        for f in (w & np.uint64(0xffff), w >> np.uint64(16)):
            s = s + ((f.astype(np.float64) + 0.5) * 2.0 ** -16 - 0.5)
    return s * SQRT_1_5


def eps(seed, draw, b, c, e):
    seed = np.asarray(seed, dtype=np.uint64)
    return deviate(philox(draw, b, c, e, seed & MASK, seed >> np.uint64(32)))


def draw_of(s, n_iter, it):
    return (int(s) * int(n_iter) + int(it)) & 0xffffffff


def noise_rows(H, noise_hold):
    return (H + noise_hold - 1) // noise_hold


def noise(seed, draw, B, N, n_rows, nu):
    """(n_rows, N, B, nu): entry (j, c, b, i) from the counter (draw, b, c, j nu + i)."""
    j, c, b, i = np.meshgrid(np.arange(n_rows), np.arange(N), np.arange(B), np.arange(nu), indexing="ij")
    return eps(seed, draw, b, c, j * nu + i)


def limit(u, lo, hi):
    return u if lo is None else np.where(u < lo, lo, np.where(u > hi, hi, u))


def candidates(u_nom, sigma, e, noise_hold, u_lo=None, u_hi=None):
    """u_nom (H, B, nu), sigma (nu,), e (n_rows, N, B, nu), limits (1 or B, nu) or None -> (H, N, B, nu); candidate 0 is u_nom itself."""
    H = u_nom.shape[0]
    rows = e[np.arange(H) // noise_hold]
    u = limit(u_nom[:, None] + np.asarray(sigma, dtype=np.float64) * rows, u_lo, u_hi)
    u[:, 0] = u_nom
    return u


def choice_of(J, ok):
    best = -1
    for c in range(len(J)):
        if ok[c] and (best < 0 or J[c] < J[best]):
            best = c
    return best


def update(u_nom, cand, J, conv, lam, u_lo=None, u_hi=None, raw=None, exp=math.exp):
    """u_nom (H, B, nu), cand (H, N, B, nu), J and conv (N, B) -> dict(ok (N, B), choice, n_eligible (B,), raw, weights (N, B), u_new, J_nom, J_best).
    raw (N, B): unnormalised weights to use in place of exp's (the device's own, for the link that is held bit for bit)."""
    H, N, B, nu = cand.shape
    ok = conv.astype(bool) & np.isfinite(J)
    out = dict(ok=ok, choice=np.zeros(B, dtype=np.int32), n_eligible=ok.sum(axis=0).astype(np.int32), raw=np.zeros((N, B)), weights=np.zeros((N, B)),
               u_new=u_nom.copy(), J_nom=J[0].copy(), J_best=J[0].copy())
    for b in range(B):
        ch = choice_of(J[:, b], ok[:, b])
        out["choice"][b] = ch
        if ch < 0:
            continue
        out["J_best"][b] = J[ch, b]
        if lam == 0.0:
            out["raw"][ch, b] = 1.0
            out["weights"][ch, b] = 1.0
            out["u_new"][:, b] = cand[:, ch, b]
            continue
        w = np.array([(exp(-((J[c, b] - J[ch, b]) / lam)) if ok[c, b] else 0.0) for c in range(N)]) if raw is None else raw[:, b].copy()
        S = 0.0
        for c in range(N):
            S = S + w[c]
        acc = np.zeros((H, nu))
        for c in range(N):
            acc = acc + w[c] * (cand[:, c, b] - u_nom[:, b])
        lo = None if u_lo is None else u_lo[0 if u_lo.shape[0] == 1 else b]
        hi = None if u_hi is None else u_hi[0 if u_hi.shape[0] == 1 else b]
        out["raw"][:, b] = w
        out["weights"][:, b] = w / S
        out["u_new"][:, b] = limit(u_nom[:, b] + acc / S, lo, hi)
    return out


def _limits(u_lo, u_hi, nu):
    if u_lo is None:
        return None, None
    return np.asarray(u_lo, dtype=np.float64).reshape(-1, nu), np.asarray(u_hi, dtype=np.float64).reshape(-1, nu)


def compose(plant, model, q1, v1, u_warm, h, mu, ref, s, H, N, sigma, *, noise_hold=1, lam=0.0, n_iter=1, seed=0, u_lo=None, u_hi=None, terrain=None,
            draws=None, raw=None, **kw):
    """Control step s by the calls that exist without the policy, from the warm start u_warm (H, B, nu).  draws: the n_iter counter words
    (default s n_iter + it); raw (n_iter, N, B): the device's unnormalised weights.  -> dict(u (B, nu), plan (H, B, nu), J0, J_nom, J_best,
    choice, n_eligible (n_iter, B), J, weights, raw, ok (n_iter, N, B), cand (n_iter, H, N, B, nu), converged (B,), traj: the last iteration's
    chosen candidate's (q, gamma, b, status, iters), candidate 0's where there is no choice)."""
    B, nq = q1.shape
    nu = u_warm.shape[2]
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (nu,))
    lo, hi = _limits(u_lo, u_hi, nu)
    cost = ref.window(s, H)
    tile = lambda a: a if a is None or a.ndim == 2 else np.tile(a, (1, N, 1))
    cost_nb = plant.TrackingCost(cost.Q, cost.R, cost.Qf, x_goal=tile(cost.x_goal), u_goal=tile(cost.u_goal))
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    mu_nb = mu if mu.size == 1 else np.tile(mu, N)
    ter_nb = terrain if terrain is None or isinstance(terrain, str) or len(terrain) == 1 else list(terrain) * N
    q1_nb, v1_nb = np.tile(q1, (N, 1)), np.tile(v1, (N, 1))
    plan = np.ascontiguousarray(u_warm, dtype=np.float64).copy()
    out = {k: [] for k in ("J_nom", "J_best", "choice", "n_eligible", "J", "weights", "raw", "cand", "ok")}
    for it in range(n_iter):
        draw = draw_of(s, n_iter, it) if draws is None else draws[it]
        cand = candidates(plan, sigma, noise(seed, draw, B, N, noise_rows(H, noise_hold), nu), noise_hold, lo, hi)
        r = plant.rollout(model, q1_nb, v1_nb, cand.reshape(H, N * B, nu), h, mu_nb, terrain=ter_nb, **kw)
        _, q, ua, gamma, bb, status, iters = r[:7]
        J = cost_nb.evaluate(q, ua)[0].reshape(N, B)
        conv = status.all(axis=0).reshape(N, B)
        up = update(plan, cand, J, conv, lam, lo, hi, raw=None if raw is None else raw[it])
        plan = up["u_new"]
        for k in ("J_nom", "J_best", "choice", "n_eligible", "weights", "raw", "ok"):
            out[k].append(up[k])
        out["J"].append(J); out["cand"].append(cand)
    out = {k: np.stack(v) for k, v in out.items()}
    pick = np.maximum(out["choice"][-1], 0) * B + np.arange(B)
    out.update(u=plan[0].copy(), plan=plan, J0=out["J_nom"][0].copy(), converged=out["choice"][-1] >= 0,
               traj=(q[:, pick], gamma[:, pick], bb[:, pick], status[:, pick], iters[:, pick]))
    return out


# ---- the settings of the device tests, fixed before their first run -----------------------------------------------------------------------------
# Test 1 (three hoppers, H 14, N 4): sigma chosen on the CPU plant (`plant_linesearch_cases._cpu_rollout`) so that at step 0 every robot has an
# eligible candidate with c >= 1: a tenth of the largest control of the rollout case's plan.
HOPPER_SIGMA_FRACTION = 0.1
# Test 9 and scripts/closed_loop_sampling_mpc.py: fixed on 2026-10-21 before the first run and not tuned afterwards
SCENE_SAMPLING = dict(n_samples=16, sigma_fraction=0.1, lam=0.0, n_iter=1, noise_hold=2, seed=1)


def hopper_sigma(c):
    return np.full(c["u"].shape[-1], HOPPER_SIGMA_FRACTION * np.abs(c["u"]).max())


def ulps(a, b):
    """The distance of float64 arrays in units in the last place of b (both finite and positive)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))
