"""Restatements and inputs of the tests of the clamped closed loop's derivative (tests/test_plant_clamp.py without a device,
tests/test_gpu_plant_clamp.py on it, scripts/plant_clamp_ab.py): the definition of DESIGN.md section 3, item 3i (csrc/plant_feedback.h),

    control i of step t of robot b is FREE when u_lo[b, i] < u_applied[t, b, i] < u_hi[b, i] and CLAMPED otherwise; the mask word of
    (t, b) has bit i set where control i is clamped; the limited law's derivative is the unlimited law's where free, exactly 0.0 where clamped,

the reverse chain of tests/plant_feedback_cases.py with the one statement the mask changes,

    gm = free ? v[2nq + i] : 0.0;  u_step[t][i] = gm;  gx = K[k]ᵀ gm  (everything behind it unchanged),

and the forward chain of tests/plant_tangent_cases.py with its one,

    δu_t[i] = free ? δū_t[i] + Σ_j K[k][i, j] δe[j] : 0.0,

each in longdouble (`_ld`), in float64 in the stated order (`_f64`) and in plain NumPy (`_np`), with the bounds built from the three
alone as in those files: 100 x max(d(np, ld), 2.2e-16) per output.  Blocks are `StepGradients.dz`: D (T, B, nr, n_cols), row-major; a
mask is (T, B) int words; Ks (T, B, nu, 2nq) the gain block each step applies."""
import numpy as np

import plant_adjoint_cases as pac
import plant_feedback_cases as pfc
import plant_tangent_cases as ptc

LD = np.longdouble
FACTOR = pac.FACTOR
OUTPUTS = pfc.OUTPUTS
TANGENT_OUTPUTS = ptc.OUTPUTS
STEPS_PER_LAUNCH = pfc.STEPS_PER_LAUNCH      # 2: a chunk boundary inside every rollout

# (nq, nu, nc, nb, nw) of the models whose shapes the host tests run: hopper_2D, pushbot (nu = 2 in this project's plant_model.h),
# walledcartpole (the model with ONE control) and centroidal_quadruped_wall (nu = 12: bit 11)
SHAPES = {"hopper_2D": (4, 2, 1, 2, 2), "pushbot": (2, 2, 2, 4, 2), "walledcartpole": (4, 1, 2, 4, 4), "centroidal_quadruped_wall": (18, 12, 8, 32, 3)}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------
def free(u: float, lo: float, hi: float) -> bool:
    """`plant_feedback_free` restated on Python floats."""
    return bool(lo < u and u < hi)


def clamped_words(u_applied, u_lo, u_hi):
    """The mask words element by element: u_applied (T, B, nu), u_lo, u_hi (nu,) or (B, nu) -> (T, B) int32."""
    ua = np.asarray(u_applied, dtype=np.float64)
    T, B, nu = ua.shape
    lo, hi = (np.broadcast_to(np.atleast_2d(np.asarray(a, dtype=np.float64)), (B, nu)) for a in (u_lo, u_hi))
    out = np.zeros((T, B), dtype=np.int32)
    for t in range(T):
        for b in range(B):
            word = 0
            for i in range(nu):
                if not free(float(ua[t, b, i]), float(lo[b, i]), float(hi[b, i])):
                    word |= 1 << i
            out[t, b] = word
    return out


def free_mask(mask, nu: int):
    """(T, B) words -> (T, B, nu) bools, True where the control is free."""
    mask = np.asarray(mask)
    return np.stack([((mask >> i) & 1) == 0 for i in range(nu)], axis=-1)


def count_bits(mask, nu: int) -> int:
    return int((~free_mask(mask, nu)).sum())


# ---- the reverse chain with a mask -----------------------------------------------------------------------------------------------------------
def _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask, dtype, product, pull):
    """`plant_feedback_cases._chain` with gm = free ? v : 0.0 in the place of v[c_u:c_w]; dict of OUTPUTS."""
    T, B, nr, n_cols = D.shape
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    fr = free_mask(mask, nu)
    zeros = lambda *s: np.zeros(s, dtype=dtype)
    gq = zeros(T + 2, B, nq) if gq is None else np.asarray(gq, dtype=dtype)
    gg = None if gg is None else np.asarray(gg, dtype=dtype)
    gb = None if gb is None else np.asarray(gb, dtype=dtype)
    nc = gg.shape[2] if gg is not None else (nr - nq - gb.shape[2] if gb is not None else 0)
    ns = dtype(n_sample)
    lam = gq.copy()
    u_step, xref_step = zeros(T, B, nu), zeros(T, B, 2 * nq)
    w_step = zeros(T, B, nw) if n_cols >= c_mu else None
    g_mu = zeros(B) if n_cols > c_mu else None
    g_h = zeros(B) if n_cols > c_h else None
    for r in range(B):
        for t in range(T - 1, -1, -1):
            a = zeros(nr)
            a[:nq] = lam[t + 2, r]
            if gg is not None:
                a[nq:nq + nc] = gg[t, r]
            if gb is not None:
                a[nr - gb.shape[2]:] = gb[t, r]
            v = product(np.asarray(D[t, r], dtype=dtype), a)
            lam[t + 1, r] = lam[t + 1, r] + v[nq:2 * nq]
            lam[t, r] = lam[t, r] + v[:nq]
            gm = np.where(fr[t, r], v[c_u:c_w], dtype(0.0))
            u_step[t, r] = gm
            if w_step is not None:
                w_step[t, r] = v[c_w:c_mu]
            if g_mu is not None:
                g_mu[r] = g_mu[r] + v[c_mu]
            if g_h is not None:
                g_h[r] = g_h[r] + v[c_h]
            gx = pull(np.asarray(Ks[t, r], dtype=dtype), gm)
            xref_step[t, r] = gx
            lam[t, r] = lam[t, r] - ns * gx[:nq]
            lam[t + 1, r] = (lam[t + 1, r] - (dtype(1.0) - ns) * gx[:nq]) - gx[nq:]
    return dict(g_q0=lam[0], g_q1=lam[1], u_step=u_step, w_step=w_step, g_mu=g_mu, g_h=g_h, xref_step=xref_step)


def chain_ld(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask):
    return _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask, LD, lambda Dt, a: (Dt * a[:, None]).sum(axis=0),
                  lambda K, gu: (K * gu[:, None]).sum(axis=0))


def chain_f64(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask):
    return _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask, np.float64, pac._ordered_product, pfc._ordered_pull)


def chain_np(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask):
    return _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask, np.float64, lambda Dt, a: Dt.T @ a, lambda K, gu: K.T @ gu)


def chain_bounds(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask):
    """(chain_ld, chain_f64, {output: 100 x max(d(chain_np, chain_ld), 2.2e-16)}): `plant_feedback_cases.bounds` with the mask."""
    args = (D, gq, gg, gb, nq, nu, nw, Ks, n_sample, mask)
    ld, f64, plain = chain_ld(*args), chain_f64(*args), chain_np(*args)
    return ld, f64, {k: FACTOR * max(pac.distance(plain[k], ld[k]), 2.2e-16) for k in OUTPUTS if ld[k] is not None}


# ---- the forward chain with a mask -----------------------------------------------------------------------------------------------------------
def _tangent(D, d, nq, nu, nw, nc, Ks, n_sample, mask, dtype, product, control):
    """`plant_tangent_cases._tangent` on a closed-loop tape with δu_t[i] = free ? control(...)[i] : 0.0; dict of TANGENT_OUTPUTS."""
    T, B, nr, n_cols = D.shape
    nth = 2 * nq + nu + nw + 2
    fr = free_mask(mask, nu)
    get = lambda k, shape: np.zeros(shape, dtype=dtype) if d.get(k) is None else np.asarray(d[k], dtype=dtype).reshape(shape)
    dq0, dq1 = get("dq0", (B, nq)), get("dq1", (B, nq))
    du, dw, dmu, dh = get("du_step", (T, B, nu)), get("dw_step", (T, B, nw)), get("dmu", (B,)), get("dh", (B,))
    dxr = get("dxref_step", (T, B, 2 * nq))
    q = np.zeros((T + 2, B, nq), dtype=dtype)
    gamma, b = np.zeros((T, B, nc), dtype=dtype), np.zeros((T, B, nr - nq - nc), dtype=dtype)
    ua = np.zeros((T, B, nu), dtype=dtype)
    q[0], q[1] = dq0, dq1
    ns = dtype(n_sample)
    for r in range(B):
        for t in range(T):
            x_state = np.concatenate([q[t + 1, r] - ns * (q[t + 1, r] - q[t, r]), q[t + 1, r]])
            e = dxr[t, r] - x_state
            u = np.where(fr[t, r], control(np.asarray(Ks[t, r], dtype=dtype), e, du[t, r]), dtype(0.0))
            ua[t, r] = u
            x = np.concatenate([q[t, r], q[t + 1, r], u, dw[t, r], dmu[r:r + 1], dh[r:r + 1]])
            assert x.shape == (nth,)
            y = product(np.asarray(D[t, r], dtype=dtype), x[:n_cols])
            q[t + 2, r], gamma[t, r], b[t, r] = y[:nq], y[nq:nq + nc], y[nq + nc:]
    return dict(q=q, gamma=gamma, b=b, u_applied=ua)


def tangent_ld(D, d, nq, nu, nw, nc, Ks, n_sample, mask):
    return _tangent(D, d, nq, nu, nw, nc, Ks, n_sample, mask, LD, lambda Dt, x: (Dt * x[None, :]).sum(axis=1),
                    lambda K, e, ub: ub + (K * e[None, :]).sum(axis=1))


def tangent_f64(D, d, nq, nu, nw, nc, Ks, n_sample, mask):
    return _tangent(D, d, nq, nu, nw, nc, Ks, n_sample, mask, np.float64, ptc._ordered_product, ptc._ordered_control)


def tangent_np(D, d, nq, nu, nw, nc, Ks, n_sample, mask):
    return _tangent(D, d, nq, nu, nw, nc, Ks, n_sample, mask, np.float64, lambda Dt, x: Dt @ x, lambda K, e, ub: ub + K @ e)


def tangent_bounds(D, d, nq, nu, nw, nc, Ks, n_sample, mask):
    """(tangent_ld, tangent_f64, {output: 100 x max(d(tangent_np, tangent_ld), 2.2e-16)}) of one direction."""
    args = (D, d, nq, nu, nw, nc, Ks, n_sample, mask)
    ld, f64, plain = tangent_ld(*args), tangent_f64(*args), tangent_np(*args)
    return ld, f64, {k: FACTOR * max(pac.distance(plain[k], ld[k]), 2.2e-16) for k in TANGENT_OUTPUTS}


def stacked(fn, D, dirs, *args):
    outs = [fn(D, d, *args) for d in dirs]
    return {k: np.stack([o[k] for o in outs]) for k in TANGENT_OUTPUTS}


# ---- duality: the inner products of the two chains and what their bounds allow ------------------------------------------------------------------
DUAL_PAIRS = (("g_q0", "dq0"), ("g_q1", "dq1"), ("u_step", "du_step"), ("w_step", "dw_step"), ("g_mu", "dmu"), ("g_h", "dh"), ("xref_step", "dxref_step"))


def duality(cots, fwd, rev, d, fwd_ld, fwd_bound, rev_ld, rev_bound):
    """(<cotangents, forward(d)>, <reverse(cotangents), d>, allowed difference) in longdouble: cots = (gq, gg, gb), fwd a forward result,
    rev a reverse one, d the direction; allowed = Σ_k bound_k max|ld_k| ‖partner_k‖₁ over the outputs of both chains - what the
    per-output bounds of each chain, built from its restatements alone, allow its inner product."""
    gq, gg, gb = cots
    L = lambda a: np.asarray(a, dtype=LD)
    lhs = (L(gq) * L(fwd["q"])).sum() + (L(gg) * L(fwd["gamma"])).sum() + (L(gb) * L(fwd["b"])).sum()
    rhs, allowed = LD(0.0), 0.0
    for k, name in DUAL_PAIRS:
        if rev.get(k) is None or d.get(name) is None:
            continue
        rhs = rhs + (L(rev[k]) * L(d[name]).reshape(np.shape(rev[k]))).sum()
        allowed += rev_bound[k] * float(np.abs(rev_ld[k]).max()) * float(np.abs(d[name]).sum())
    for k, c in (("q", gq), ("gamma", gg), ("b", gb)):
        allowed += fwd_bound[k] * float(np.abs(fwd_ld[k]).max()) * float(np.abs(c).sum())
    return lhs, rhs, allowed


# ---- random inputs for the host build ------------------------------------------------------------------------------------------------------------
MASKS = ("free", "clamped", "random")


def random_case(shape: str, T: int, mask_kind: str, B: int = 2, hold: int = 1, n_sample: float = 1.0, shared: bool = False, full: bool = True, seed: int = 0):
    """Random blocks, gains, a mask and both chains' inputs at a model's sizes: dict(nq, nu, nw, nc, nb, D (T, B, nr, n_cols), status,
    K (K_f, [B,] nu, 2nq), hold, n_sample, Ks (T, B, nu, 2nq), mask (T, B), cots (gq, gg, gb), d a direction).  full: every column of θ."""
    nq, nu, nc, nb, nw = SHAPES[shape]
    nr = nq + nc + nb
    n_cols = 2 * nq + nu + (nw + 2 if full else 0)
    rng = np.random.default_rng([sorted(SHAPES).index(shape), T, MASKS.index(mask_kind), hold, seed])
    D = rng.standard_normal((T, B, nr, n_cols)) / np.sqrt(n_cols)
    K_f = -(-T // hold)
    K = 0.3 * rng.standard_normal((K_f, nu, 2 * nq) if shared else (K_f, B, nu, 2 * nq))
    Ks, _ = pfc.per_step(dict(K=K, x_ref=np.zeros(K.shape[:-2] + (2 * nq,)), hold=hold), T, B)
    all_bits = (1 << nu) - 1
    mask = {"free": np.zeros((T, B), dtype=np.int32), "clamped": np.full((T, B), all_bits, dtype=np.int32),
            "random": rng.integers(0, all_bits + 1, (T, B)).astype(np.int32)}[mask_kind]
    cots = pac.random_cotangents(rng, T, B, nq, nc, nb)
    d = ptc.random_direction(rng, T, B, nq, nu, nw, n_cols, closed=True)
    return dict(nq=nq, nu=nu, nw=nw, nc=nc, nb=nb, D=D, status=np.ones((T, B), dtype=np.int32), K=K, hold=hold, n_sample=n_sample, Ks=Ks, mask=mask,
                cots=cots, d=d)


# ---- the device cases ------------------------------------------------------------------------------------------------------------------------------
# (case of plant_feedback_cases, variant, steps kept): B <= 3, T <= 12; pushbot and the wall at the trimmed shapes of
# tests/test_gpu_plant_boxqp.py's _loop_case (pushbot B 2 T 4, centroidal_quadruped_wall B 1 T 2)
DEVICE_CASES = {"hopper_2D-per_robot": ("hopper_2D", "per_robot", 12), "hopper_2D-held": ("hopper_2D", "held", 12), "pushbot": ("pushbot", "per_robot", 4),
                "centroidal_quadruped_wall": ("centroidal_quadruped_wall", "per_robot", 2)}


def device_case(name: str):
    """(case dict, feedback dict) cut to the steps kept; the arrays are views of the cached ones and read-only."""
    which, variant, T = DEVICE_CASES[name]
    c, f = dict(pfc.base_case(which)), dict(pfc.feedback(which, variant))
    T = min(T, c["T"])
    c.update(u=c["u"][:T], T=T)
    if f["K"].shape[0] > T:
        f.update(K=f["K"][:T], x_ref=f["x_ref"][:T])
    return c, f


def limits_from(ua0):
    """The limits of tests/test_gpu_plant_boxqp.py's test_limited_closed_loop, from the applied controls ua0 (T, B, nu) of the UNLIMITED loop
    of the same call: control 0 capped a quarter below what the law asks at step 0, control 1 (where there is one) finite limits one unit
    outside everything applied, the rest none."""
    T, B, nu = ua0.shape
    u_lo, u_hi = np.full((B, nu), -np.inf), np.full((B, nu), np.inf)
    u_hi[:, 0] = ua0[0, :, 0] - 0.25 * (np.abs(ua0[0, :, 0]) + 1e-3)
    if nu >= 2:
        u_lo[:, 1], u_hi[:, 1] = ua0[:, :, 1].min(axis=0) - 1.0, ua0[:, :, 1].max(axis=0) + 1.0
    return u_lo, u_hi
