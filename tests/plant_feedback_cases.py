"""Inputs and restatements of the closed-loop rollout tests (tests/test_plant_feedback.py without a device,
tests/test_gpu_plant_feedback.py on it, scripts/plant_feedback_ab.py): the definition of DESIGN.md section 3, item 3c
(csrc/plant_feedback.h), per robot and step t with feedback row k = min(t // hold_f, K_f - 1),

    x = [q[t+1] - n_sample (q[t+1] - q[t]); q[t+1]];  e = x_ref[k] - x;  u_t = ū_t + K[k] e      (ascending j from 0.0, no fused multiply-add)

and the reverse chain of tests/plant_adjoint_cases.py extended by its three statements,

    gx = K[k]ᵀ gu (ascending i from 0.0);  λ[t][:nq] -= n_sample gx[:nq];  λ[t+1] = (λ[t+1] - (1 - n_sample) gx[:nq]) - gx[nq:]

in longdouble (`chain_ld`), in float64 in the stated order (`chain_f64`) and in plain NumPy (`chain_np`), with, written independently,
the forward recursion of tangents under δu_t = δū_t + δK e - K δx + K δx_ref.  The seven cases make every step instance of
csrc/plant_ground.h run the branch; each is stepped on the CPU under the law (`cpu_closed_loop`) and every step of every variant
converges there (tests/test_plant_feedback.py asserts it).  Every reference is computed once per process and read-only."""
import functools
import os

import numpy as np

import plant_adjoint_cases as pac
import plant_gradient_cases as pgc

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
CASES = ("hopper_2D", "particle", "quadruped", "centroidal_quadruped_wall", "pushbot", "hopper_3D", "centroidal_quadruped_box")
GAIN_SCALE, OFFSET = 0.1, 1e-2
STEPS_PER_LAUNCH = 2            # a chunk boundary inside every rollout
OUTPUTS = pac.OUTPUTS + ("xref_step",)


@functools.lru_cache(maxsize=None)
def base_case(which: str):
    """The open-loop rollout a case starts from: `plant_gradient_cases.rollout_case` for its four, and three short ones - pushbot
    swinging into its right wall, hopper_3D over sine2_3D_lc from two knots of its forward gait, centroidal_quadruped_box from the middle
    of its gait."""
    if which in pgc.ROLLOUTS:
        return pgc.rollout_case(which)
    from contactimplicitmpc.jl_amd import gait_io
    if which == "pushbot":
        B, T, h = 2, 5, 0.02
        q1 = np.array([[0.30, 0.20], [-0.35, 0.10]])
        v1 = np.array([[1.5, 0.5], [-1.0, 0.2]])
        u = np.stack([np.array([[0.2, -0.1], [-0.3, 0.1]]) * (1.0 + 0.1 * t) for t in range(T)])
        return dict(model="pushbot", terrain=None, q1=q1, v1=v1, u=u, mu=np.array([0.5, 0.5]), h=h, T=T)
    if which == "hopper_3D":
        g, T = gait_io.load_joint_traj(os.path.join(HERE, "golden", "gaits", "hopper_3D_gait_forward.jld2")), 4
        k = np.array([0, 9])
        shift = np.zeros((2, 7)); shift[:, 0] = 0.13 * k; shift[:, 2] = 0.075
        u = np.stack([g.u[(k + t) % g.H] for t in range(T)])
        return dict(model="hopper_3D", terrain="sine2_3D_lc", q1=g.q[k + 1] + shift, v1=(g.q[k + 1] - g.q[k]) / g.h, u=u, mu=np.array([1.5, 1.5]),
                    h=g.h, T=T)
    if which == "centroidal_quadruped_box":
        g, T = gait_io.load_gait(os.path.join(HERE, "golden", "gaits", "step_over_box_v0.jld2")), 2
        k = np.array([g.H // 2])
        u = np.stack([g.u[(k + t) % g.H] for t in range(T)])
        return dict(model="centroidal_quadruped_box", terrain=None, q1=g.q[k + 1], v1=(g.q[k + 1] - g.q[k]) / g.h, u=u, mu=np.array([g.mu]), h=g.h, T=T)
    raise KeyError(which)


def cpu_plant(case):
    if case["model"] == "pushbot":
        import walled_ref
        return walled_ref.PLANTS["pushbot"]()
    if case["model"] == "hopper_3D":
        import hopper_3d_ref
        return hopper_3d_ref.Hopper3DPlant(case["terrain"])
    return pgc.cpu_plant(case)


# (name, per-robot schedule, n_sample, (K_f, hold_f) or None = one row per step)
VARIANTS = {"shared": (False, 1.0, None), "per_robot": (True, 4.0, None), "held": (True, 4.0, (2, 2))}


def variants(which: str):
    """The schedules a case runs: one shared with n_sample = 1, one per robot with n_sample = 4, and on hopper_2D (T = 14) one of
    K_f = 2 rows held for 2 steps, whose last row is held from step 2 on."""
    return ("shared", "per_robot", "held") if which == "hopper_2D" else ("shared", "per_robot")


def law(K, x_ref, q0, q1, ubar, n_sample):
    """(u_t, e) of one robot's step in float64 in the stated order: K (nu, 2nq), x_ref (2nq,)."""
    x = np.concatenate([q1 - n_sample * (q1 - q0), q1])
    e = x_ref - x
    s = np.zeros(K.shape[0])
    for j in range(K.shape[1]):
        s = s + K[:, j] * e[j]
    return ubar + s, e


def row_of(t: int, hold: int, K_f: int):
    return min(t // hold, K_f - 1)


def _step(P, q0, q1, u, nw, mu, h):
    from oracle import plant as pl
    return pgc.cpu_step_z(P, q0, q1, u, np.zeros(nw), mu, h, pl.SIM_OPTS)


@functools.lru_cache(maxsize=None)
def cpu_open_loop(which: str):
    """(status (T, B), q (T + 2, B, nq)) of the base case stepped on the CPU."""
    c = base_case(which)
    P = cpu_plant(c)
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    B, T, h = c["q1"].shape[0], c["T"], c["h"]
    st, q = np.zeros((T, B), dtype=bool), np.zeros((T + 2, B, nq))
    q[0], q[1] = c["q1"] - h * c["v1"], c["q1"]
    for b in range(B):
        for t in range(T):
            st[t, b], z, _ = _step(P, q[t, b], q[t + 1, b], c["u"][t, b], nw, c["mu"][b], h)
            q[t + 2, b] = z[:nq]
    st.setflags(write=False); q.setflags(write=False)
    return st, q


@functools.lru_cache(maxsize=None)
def feedback(which: str, variant: str):
    """dict(K (K_f, [B,] nu, 2nq), x_ref (K_f, [B,] 2nq), hold, n_sample) of a case's variant: K = 0.1 standard_normal, x_ref the
    open-loop CPU rollout's [q[t]; q[t + 1]] at the first step of each row plus a uniform offset of at most 1e-2, both seeded."""
    per_robot, n_sample, held = VARIANTS[variant]
    c = base_case(which)
    nq, nu = pgc.dims(c["model"])[:2]
    B, T = c["q1"].shape[0], c["T"]
    K_f, hold = held if held else (T, 1)
    rng = np.random.default_rng([CASES.index(which), sorted(VARIANTS).index(variant)])
    _, q = cpu_open_loop(which)
    rows = np.arange(K_f) * hold
    x = np.concatenate([q[rows], q[rows + 1]], axis=2)                         # (K_f, B, 2nq)
    if per_robot:
        K = GAIN_SCALE * rng.standard_normal((K_f, B, nu, 2 * nq))
        x_ref = x + OFFSET * rng.uniform(-1.0, 1.0, x.shape)
    else:
        K = GAIN_SCALE * rng.standard_normal((K_f, nu, 2 * nq))
        x_ref = x[:, 0] + OFFSET * rng.uniform(-1.0, 1.0, x[:, 0].shape)
    K.setflags(write=False); x_ref.setflags(write=False)
    return dict(K=K, x_ref=x_ref, hold=hold, n_sample=n_sample)


def per_step(fb, T: int, B: int):
    """The schedule spread over the steps: (K (T, B, nu, 2nq), x_ref (T, B, 2nq))."""
    K, xr = np.asarray(fb["K"]), np.asarray(fb["x_ref"])
    k = [row_of(t, fb["hold"], K.shape[0]) for t in range(T)]
    if K.ndim == 3:
        return np.broadcast_to(K[k][:, None], (T, B) + K.shape[1:]), np.broadcast_to(xr[k][:, None], (T, B, xr.shape[1]))
    return K[k], xr[k]


def law_on(q, ubar_step, fb):
    """The law restated on a trajectory q (T + 2, B, nq) and the open-loop controls (T, B, nu): (u_applied (T, B, nu), e (T, B, 2nq))."""
    T, B = ubar_step.shape[:2]
    Ks, xs = per_step(fb, T, B)
    u, e = np.zeros(ubar_step.shape), np.zeros((T, B, q.shape[2] * 2))
    for t in range(T):
        for b in range(B):
            u[t, b], e[t, b] = law(Ks[t, b], xs[t, b], q[t, b], q[t + 1, b], ubar_step[t, b], fb["n_sample"])
    return u, e


@functools.lru_cache(maxsize=None)
def cpu_closed_loop(which: str, variant: str):
    """The case stepped on the CPU under the law: (status (T, B), q (T + 2, B, nq), u_applied (T, B, nu))."""
    c, fb = base_case(which), feedback(which, variant)
    P = cpu_plant(c)
    nq, nu, nc, nb, nw = pgc.dims(c["model"])[:5]
    B, T, h = c["q1"].shape[0], c["T"], c["h"]
    Ks, xs = per_step(fb, T, B)
    st, q, ua = np.zeros((T, B), dtype=bool), np.zeros((T + 2, B, nq)), np.zeros((T, B, nu))
    q[0], q[1] = c["q1"] - h * c["v1"], c["q1"]
    for b in range(B):
        for t in range(T):
            ua[t, b], _ = law(Ks[t, b], xs[t, b], q[t, b], q[t + 1, b], c["u"][t, b], fb["n_sample"])
            st[t, b], z, _ = _step(P, q[t, b], q[t + 1, b], ua[t, b], nw, c["mu"][b], h)
            q[t + 2, b] = z[:nq]
    return st, q, ua


# ---- the reverse chain with the feedback statements ----------------------------------------------------------------------------------------
def _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, dtype, product, pull):
    """`plant_adjoint_cases._chain` with the three statements after v = D_tᵀ a; Ks (T, B, nu, 2nq) the step's gain block,
    `pull(K (nu, 2nq), gu (nu,)) -> gx (2nq,)`.  dict of OUTPUTS."""
    T, B, nr, n_cols = D.shape
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
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
            u_step[t, r] = v[c_u:c_w]
            if w_step is not None:
                w_step[t, r] = v[c_w:c_mu]
            if g_mu is not None:
                g_mu[r] = g_mu[r] + v[c_mu]
            if g_h is not None:
                g_h[r] = g_h[r] + v[c_h]
            gx = pull(np.asarray(Ks[t, r], dtype=dtype), v[c_u:c_w])
            xref_step[t, r] = gx
            lam[t, r] = lam[t, r] - ns * gx[:nq]
            lam[t + 1, r] = (lam[t + 1, r] - (dtype(1.0) - ns) * gx[:nq]) - gx[nq:]
    return dict(g_q0=lam[0], g_q1=lam[1], u_step=u_step, w_step=w_step, g_mu=g_mu, g_h=g_h, xref_step=xref_step)


def _ordered_pull(K, gu):
    s = np.zeros(K.shape[1], dtype=K.dtype)
    for i in range(K.shape[0]):
        s = s + K[i] * gu[i]
    return s


def chain_ld(D, gq, gg, gb, nq, nu, nw, Ks, n_sample):
    return _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, LD, lambda Dt, a: (Dt * a[:, None]).sum(axis=0), lambda K, gu: (K * gu[:, None]).sum(axis=0))


def chain_f64(D, gq, gg, gb, nq, nu, nw, Ks, n_sample):
    return _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, np.float64, pac._ordered_product, _ordered_pull)


def chain_np(D, gq, gg, gb, nq, nu, nw, Ks, n_sample):
    return _chain(D, gq, gg, gb, nq, nu, nw, Ks, n_sample, np.float64, lambda Dt, a: Dt.T @ a, lambda K, gu: K.T @ gu)


def bounds(D, gq, gg, gb, nq, nu, nw, Ks, n_sample):
    """`plant_adjoint_cases.bounds` for the extended chain: (chain_ld, chain_f64, {output: 100 x max(d(chain_np, chain_ld), 2.2e-16)})."""
    args = (D, gq, gg, gb, nq, nu, nw, Ks, n_sample)
    ld, f64, plain = chain_ld(*args), chain_f64(*args), chain_np(*args)
    return ld, f64, {k: pac.FACTOR * max(pac.distance(plain[k], ld[k]), 2.2e-16) for k in OUTPUTS if ld[k] is not None}


def forward_tangent(D, dq0, dq1, dubar, nq, nu, nw, Ks, es, n_sample, dK=None, dxref=None, dmu=None):
    """Tangents pushed FORWARD through a closed-loop rollout, in longdouble, written independently of the chains: per step
    δx = [δq[t+1] - n_sample (δq[t+1] - δq[t]); δq[t+1]],  δu_t = δū_t + δK_t e_t - K_t δx + K_t δx_ref,t,
    [δq[t+2]; δγ; δb] = D_t [δq[t]; δq[t+1]; δu_t; 0 (w); δμ; 0 (h)].  Ks, dK (T, B, nu, 2nq), es, dxref (T, B, 2nq).
    Returns (δq (T + 2, B, nq), δγb (T, B, nr - nq))."""
    T, B, nr, n_cols = D.shape
    nth = 2 * nq + nu + nw + 2
    dq, dgb = np.zeros((T + 2, B, nq), dtype=LD), np.zeros((T, B, nr - nq), dtype=LD)
    dq[0], dq[1] = dq0, dq1
    ns = LD(n_sample)
    for t in range(T):
        for r in range(B):
            K = np.asarray(Ks[t, r], dtype=LD)
            dx = np.concatenate([dq[t + 1, r] - ns * (dq[t + 1, r] - dq[t, r]), dq[t + 1, r]])
            du = np.asarray(dubar[t, r], dtype=LD) - K @ dx
            if dK is not None:
                du = du + np.asarray(dK[t, r], dtype=LD) @ np.asarray(es[t, r], dtype=LD)
            if dxref is not None:
                du = du + K @ np.asarray(dxref[t, r], dtype=LD)
            th = np.zeros(nth, dtype=LD)
            th[:nq], th[nq:2 * nq], th[2 * nq:2 * nq + nu] = dq[t, r], dq[t + 1, r], du
            if dmu is not None:
                th[nth - 2] = dmu[r]
            out = np.asarray(D[t, r], dtype=LD) @ th[:n_cols]
            dq[t + 2, r], dgb[t, r] = out[:nq], out[nq:]
    return dq, dgb


def fold_gains(u_step, es, K_f: int, hold: int, shared: bool, scale: float):
    """The gradient of the gain rows, element by element: entry (i, j) of row k takes u_step[t, b, i] es[t, b, j] of the steps (and, shared,
    the robots) that read the row, added in ascending (t, b), the sum divided by `scale`."""
    T, B, nu = u_step.shape
    n2 = es.shape[2]
    out = np.zeros((K_f, nu, n2) if shared else (K_f, B, nu, n2))
    for k in range(K_f):
        for r in ([None] if shared else range(B)):
            for i in range(nu):
                for j in range(n2):
                    s = 0.0
                    for t in range(T):
                        if row_of(t, hold, K_f) != k:
                            continue
                        for rb in (range(B) if shared else [r]):
                            s = s + u_step[t, rb, i] * es[t, rb, j]
                    if shared:
                        out[k, i, j] = s / scale
                    else:
                        out[k, r, i, j] = s / scale
    return out


def fold_rows(g_step, K_f: int, hold: int, shared: bool):
    """The gradient of x_ref from xref_step, element by element: row k takes the steps (and, shared, the robots) that read it, in
    ascending (t, b)."""
    T, B, n = g_step.shape
    out = np.zeros((K_f, n) if shared else (K_f, B, n))
    for k in range(K_f):
        for r in ([None] if shared else range(B)):
            for j in range(n):
                s = 0.0
                for t in range(T):
                    if row_of(t, hold, K_f) != k:
                        continue
                    for rb in (range(B) if shared else [r]):
                        s = s + g_step[t, rb, j]
                if shared:
                    out[k, j] = s
                else:
                    out[k, r, j] = s
    return out
