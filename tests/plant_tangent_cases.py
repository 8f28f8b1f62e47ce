"""Restatements shared by the forward-tangent tests (tests/test_plant_tangent.py without a device, tests/test_gpu_plant_tangent.py on it,
scripts/plant_tangent_ab.py): the definition of DESIGN.md section 3, item 3d (csrc/plant_tangent.h), per robot and direction

    δq[0] = dq0, δq[1] = dq1
    for t = 0 .. T-1:  closed loop: δe = δxref_t - [δq[t+1] - n_sample (δq[t+1] - δq[t]); δq[t+1]];  δu_t = δū_t + K_t δe   (ascending j from 0.0)
                       open loop:   δu_t = δū_t
                       x = [δq[t]; δq[t+1]; δu_t; δw_t; δμ; δh] cut to n_cols;  y = D_t x   (ascending c from 0.0, one product and one sum per term)
                       δq[t+2] = y[:nq];  δγ[t] = y[nq:nq+nc];  δb[t] = y[nq+nc:]

three times - in longdouble (`tangent_ld`), in float64 in the order the definition states (`tangent_f64`: every term one rounded
product and one rounded sum; the loop runs over the terms, NumPy's elementwise operations over the outputs) and in plain float64 NumPy
with `@` (`tangent_np`) -, and, element by element, what `RolloutTape.jvp`'s arguments mean in those per-step terms (`step_inputs`).
Blocks are `StepGradients.dz`: D (T, B, nr, n_cols), row-major.  One direction per call; `stacked` runs several.

A direction is a dict with any of dq0, dq1 (B, nq), du_step (T, B, nu), dw_step (T, B, nw), dmu, dh (B,), dxref_step (T, B, 2nq); a key
left out is zeros.  A closed-loop chain takes loop = (Ks (T, B, nu, 2nq) the gain block each step applies, n_sample)."""
import numpy as np

import plant_adjoint_cases as pac

LD = np.longdouble
FACTOR = pac.FACTOR
OUTPUTS = ("q", "gamma", "b", "u_applied")


def _tangent(D, d, nq, nu, nw, nc, loop, dtype, product, control):
    """The recursion with `product(D_t (nr, n_cols), x (n_cols,)) -> y (nr,)` and `control(K (nu, 2nq), e (2nq,), ubar (nu,)) -> u`."""
    T, B, nr, n_cols = D.shape
    nth = 2 * nq + nu + nw + 2
    get = lambda k, shape: np.zeros(shape, dtype=dtype) if d.get(k) is None else np.asarray(d[k], dtype=dtype).reshape(shape)
    dq0, dq1 = get("dq0", (B, nq)), get("dq1", (B, nq))
    du, dw, dmu, dh = get("du_step", (T, B, nu)), get("dw_step", (T, B, nw)), get("dmu", (B,)), get("dh", (B,))
    dxr = get("dxref_step", (T, B, 2 * nq))
    q = np.zeros((T + 2, B, nq), dtype=dtype)
    gamma, b = np.zeros((T, B, nc), dtype=dtype), np.zeros((T, B, nr - nq - nc), dtype=dtype)
    ua = None if loop is None else np.zeros((T, B, nu), dtype=dtype)
    q[0], q[1] = dq0, dq1
    for r in range(B):
        for t in range(T):
            u = du[t, r]
            if loop is not None:
                Ks, n_sample = loop
                ns = dtype(n_sample)
                x_state = np.concatenate([q[t + 1, r] - ns * (q[t + 1, r] - q[t, r]), q[t + 1, r]])
                e = dxr[t, r] - x_state
                u = control(np.asarray(Ks[t, r], dtype=dtype), e, u)
                ua[t, r] = u
            x = np.concatenate([q[t, r], q[t + 1, r], u, dw[t, r], dmu[r:r + 1], dh[r:r + 1]])
            assert x.shape == (nth,)
            y = product(np.asarray(D[t, r], dtype=dtype), x[:n_cols])
            q[t + 2, r], gamma[t, r], b[t, r] = y[:nq], y[nq:nq + nc], y[nq + nc:]
    return dict(q=q, gamma=gamma, b=b, u_applied=ua)


def _ordered_product(Dt, x):
    """y[r] = Σ_c D[r, c] x[c], ascending c from 0.0, every term one rounded product and one rounded sum."""
    y = np.zeros(Dt.shape[0], dtype=Dt.dtype)
    for c in range(Dt.shape[1]):
        y = y + Dt[:, c] * x[c]
    return y


def _ordered_control(K, e, ubar):
    s = np.zeros(K.shape[0], dtype=K.dtype)
    for j in range(K.shape[1]):
        s = s + K[:, j] * e[j]
    return ubar + s


def tangent_ld(D, d, nq, nu, nw, nc, loop=None):
    return _tangent(D, d, nq, nu, nw, nc, loop, LD, lambda Dt, x: (Dt * x[None, :]).sum(axis=1), lambda K, e, ub: ub + (K * e[None, :]).sum(axis=1))


def tangent_f64(D, d, nq, nu, nw, nc, loop=None):
    return _tangent(D, d, nq, nu, nw, nc, loop, np.float64, _ordered_product, _ordered_control)


def tangent_np(D, d, nq, nu, nw, nc, loop=None):
    return _tangent(D, d, nq, nu, nw, nc, loop, np.float64, lambda Dt, x: Dt @ x, lambda K, e, ub: ub + K @ e)


def stacked(fn, D, dirs, nq, nu, nw, nc, loop=None):
    """`fn` on each direction of a list, every output stacked on a leading axis."""
    outs = [fn(D, d, nq, nu, nw, nc, loop) for d in dirs]
    return {k: None if outs[0][k] is None else np.stack([o[k] for o in outs]) for k in OUTPUTS}


def bounds(D, d, nq, nu, nw, nc, loop=None):
    """(tangent_ld, tangent_f64, {output: 100 x max(d(tangent_np, tangent_ld), 2.2e-16)}) of one direction: the bound of every output,
    relative to that output's max|tangent_ld|, built from the restatements alone."""
    ld, f64, plain = (fn(D, d, nq, nu, nw, nc, loop) for fn in (tangent_ld, tangent_f64, tangent_np))
    return ld, f64, {k: FACTOR * max(pac.distance(plain[k], ld[k]), 2.2e-16) for k in OUTPUTS if ld[k] is not None}


# ---- what the arguments of RolloutTape.jvp mean per step, element by element -----------------------------------------------------------------
def row_of(t: int, hold: int, K: int):
    return min(t // hold, K - 1)


def spread_rows(d, T: int, B: int, hold: int, scale: float = 1.0):
    """A schedule tangent d (K, n) shared or (K, B, n) on its steps: (T, B, n), step t of robot b taking d[row_of(t)][b] / scale."""
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros((T, B, d.shape[-1]))
    for t in range(T):
        for b in range(B):
            for i in range(d.shape[-1]):
                out[t, b, i] = (d[row_of(t, hold, d.shape[0]), i] if d.ndim == 2 else d[row_of(t, hold, d.shape[0]), b, i]) / scale
    return out


def spread_gain_rows(dK, fb_err, hold: int, scale: float):
    """What a tangent of the gain rows dK (K_f, nu, 2nq) or (K_f, B, nu, 2nq) adds to δū_t: (T, B, nu), Σ_j (dK[k][i, j] / scale) fb_err[t, b, j],
    ascending j from 0.0."""
    dK = np.asarray(dK, dtype=np.float64)
    T, B, n2 = fb_err.shape
    out = np.zeros((T, B, dK.shape[-2]))
    for t in range(T):
        k = row_of(t, hold, dK.shape[0])
        for b in range(B):
            Kk = dK[k] if dK.ndim == 3 else dK[k, b]
            for i in range(Kk.shape[0]):
                s = 0.0
                for j in range(n2):
                    s = s + (Kk[i, j] / scale) * fb_err[t, b, j]
                out[t, b, i] = s
    return out


def step_inputs(T, B, h, v1, N_sample=1, w_hold=1, dq1=None, dv1=None, du=None, dw=None, dmu=None, dh=None, dK=None, dx_ref=None, fb_hold=1,
                fb_err=None):
    """One direction in the arguments of `rollout_tape` (each in the shape the caller gave them) as a direction of the chain:
    dq1 = δq1, dq0 = (δq1 - h δv1) - δh v1; δū_t = δu[k] / N_sample (+ (δK[k] / N_sample) fb_err[t]); δw_t = δw[k_w]; one δμ, one δh for
    every robot; δx_ref rows by the feedback schedule's hold."""
    nq = v1.shape[1]
    z = np.zeros((B, nq))
    q1 = z if dq1 is None else np.broadcast_to(np.asarray(dq1, dtype=np.float64), (B, nq))
    vv = z if dv1 is None else np.broadcast_to(np.asarray(dv1, dtype=np.float64), (B, nq))
    hh = np.zeros(B) if dh is None else np.broadcast_to(np.asarray(dh, dtype=np.float64), (B,))
    d = dict(dq1=q1.copy(), dq0=(q1 - h * vv) - hh[:, None] * v1)
    if du is not None or dK is not None:
        d["du_step"] = np.zeros((T, B, np.shape(dK)[-2])) if du is None else spread_rows(du, T, B, N_sample, N_sample)
        if dK is not None:
            d["du_step"] = d["du_step"] + spread_gain_rows(dK, fb_err, fb_hold, N_sample)
    if dw is not None:
        d["dw_step"] = spread_rows(dw, T, B, w_hold)
    if dmu is not None:
        d["dmu"] = np.broadcast_to(np.asarray(dmu, dtype=np.float64).reshape(-1), (B,)).copy()
    if dh is not None:
        d["dh"] = hh.copy()
    if dx_ref is not None:
        d["dxref_step"] = spread_rows(dx_ref, T, B, fb_hold)
    return d


def random_direction(rng, T, B, nq, nu, nw, n_cols, closed=False):
    """A direction of the chain with every input the columns reach."""
    c_u, c_w, c_mu, c_h = pac.columns(nq, nu, nw)
    d = dict(dq0=rng.standard_normal((B, nq)), dq1=rng.standard_normal((B, nq)), du_step=rng.standard_normal((T, B, nu)))
    if n_cols >= c_mu:
        d["dw_step"] = rng.standard_normal((T, B, nw))
    if n_cols > c_mu:
        d["dmu"] = rng.standard_normal(B)
    if n_cols > c_h:
        d["dh"] = rng.standard_normal(B)
    if closed:
        d["dxref_step"] = rng.standard_normal((T, B, 2 * nq))
    return d
