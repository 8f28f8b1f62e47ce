"""Restatements shared by the reverse-chain tests (tests/test_plant_adjoint.py without a device, tests/test_gpu_plant_adjoint.py on it,
scripts/plant_adjoint_ab.py): the definition of DESIGN.md section 3, item 3b (csrc/plant_adjoint.h), per robot

    λ[0..T+1] = gq
    for t = T-1 .. 0:  a = [λ[t+2]; gγ[t]; gb[t]];  v = D_tᵀ a;  λ[t+1] += v[nq:2nq];  λ[t] += v[0:nq]
                       g_u_step[t] = v[2nq:2nq+nu];  g_w_step[t] = v[w columns];  g_μ += v[μ column];  g_h += v[h column]
    g_q0 = λ[0], g_q1 = λ[1]

three times - in longdouble (`chain_ld`), in float64 in the order the definition states, one product and one sum per term
(`chain_f64`), and in plain float64 NumPy with `@` (`chain_np`) -, the fold of per-step control gradients onto schedule rows (`fold_u`),
and, written independently of all of them, the forward recursion of tangents (`forward_tangent`).  Blocks are `StepGradients.dz`:
D (T, B, nr, n_cols), row-major."""
import numpy as np

LD = np.longdouble
FACTOR = 100.0
OUTPUTS = ("g_q0", "g_q1", "u_step", "w_step", "g_mu", "g_h")


def columns(nq, nu, nw):
    """(first u column, first w column, the μ column, the h column) of θ = [q0; q1; u1; w1; μ; h]."""
    return 2 * nq, 2 * nq + nu, 2 * nq + nu + nw, 2 * nq + nu + nw + 1


def _chain(D, gq, gg, gb, nq, nu, nw, dtype, product):
    """The recursion with `product(D_t (nr, n_cols), a (nr,)) -> v (n_cols,)`; cotangents None = zeros.  dict of OUTPUTS, an output
    whose columns D does not reach being None."""
    T, B, nr, n_cols = D.shape
    nc_nb = nr - nq
    c_u, c_w, c_mu, c_h = columns(nq, nu, nw)
    zeros = lambda *s: np.zeros(s, dtype=dtype)
    gq = zeros(T + 2, B, nq) if gq is None else np.asarray(gq, dtype=dtype)
    gg = None if gg is None else np.asarray(gg, dtype=dtype)
    gb = None if gb is None else np.asarray(gb, dtype=dtype)
    nc = gg.shape[2] if gg is not None else (nc_nb - gb.shape[2] if gb is not None else 0)
    lam = gq.copy()
    u_step = zeros(T, B, nu)
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
    return dict(g_q0=lam[0], g_q1=lam[1], u_step=u_step, w_step=w_step, g_mu=g_mu, g_h=g_h)


def _ordered_product(Dt, a):
    """v[c] = Σ_r D[r, c] a[r], ascending r from 0.0, every term one rounded product and one rounded sum."""
    nr, n_cols = Dt.shape
    v = np.zeros(n_cols, dtype=Dt.dtype)
    for c in range(n_cols):
        s = Dt.dtype.type(0.0)
        for r in range(nr):
            s = s + Dt[r, c] * a[r]
        v[c] = s
    return v


def chain_ld(D, gq, gg, gb, nq, nu, nw):
    return _chain(D, gq, gg, gb, nq, nu, nw, LD, lambda Dt, a: (Dt * a[:, None]).sum(axis=0))


def chain_f64(D, gq, gg, gb, nq, nu, nw):
    return _chain(D, gq, gg, gb, nq, nu, nw, np.float64, _ordered_product)


def chain_np(D, gq, gg, gb, nq, nu, nw):
    return _chain(D, gq, gg, gb, nq, nu, nw, np.float64, lambda Dt, a: Dt.T @ a)


def distance(got, ref):
    """max|got - ref| / max|ref| in longdouble (0 / 0 = 0)."""
    ref = np.asarray(ref, dtype=LD)
    d, m = float(np.abs(np.asarray(got, dtype=LD) - ref).max()), float(np.abs(ref).max())
    return 0.0 if d == 0.0 else d / m if m > 0.0 else float("inf")


def bounds(D, gq, gg, gb, nq, nu, nw):
    """(chain_ld, chain_f64, {output: 100 x max(d(chain_np, chain_ld), 2.2e-16)}) of one set of blocks and cotangents: the bound of
    every output, built from the restatements alone."""
    ld, f64, plain = chain_ld(D, gq, gg, gb, nq, nu, nw), chain_f64(D, gq, gg, gb, nq, nu, nw), chain_np(D, gq, gg, gb, nq, nu, nw)
    bound = {k: FACTOR * max(distance(plain[k], ld[k]), 2.2e-16) for k in OUTPUTS if ld[k] is not None}
    return ld, f64, bound


def schedule_row(t: int, hold: int, K: int):
    return min(t // hold, K - 1)


def fold_u(u_step, K: int, N_sample: int, shared: bool):
    """The gradient of the nominal controls from the per-step ones: element by element, step t lands on row min(t // N_sample, K - 1)
    (and every robot on the one row when the schedule is shared), added in ascending (t, b) order, the sum divided by N_sample."""
    T, B, nu = u_step.shape
    out = np.zeros((K, nu) if shared else (K, B, nu))
    for i in range(nu):
        for k in range(K):
            for r in ([None] if shared else range(B)):
                s = 0.0
                for t in range(T):
                    if schedule_row(t, N_sample, K) != k:
                        continue
                    for rb in (range(B) if shared else [r]):
                        s = s + u_step[t, rb, i]
                if shared:
                    out[k, i] = s / N_sample
                else:
                    out[k, r, i] = s / N_sample
    return out


def forward_tangent(D, dq0, dq1, du_step, nq, nu, nw, dw_step=None, dmu=None, dh=None):
    """Tangents pushed FORWARD through the blocks, in longdouble: δθ_t = [δq[t]; δq[t+1]; δu_t; δw_t; δμ; δh] (cut to the columns D has),
    [δq[t+2]; δγ[t]; δb[t]] = D_t δθ_t.  dq0, dq1 (B, nq), du_step (T, B, nu), dw_step (T, B, nw), dmu, dh (B,); None = zeros.
    Returns (δq (T + 2, B, nq), δγb (T, B, nr - nq)): the rows of γ and b together, in the blocks' order."""
    T, B, nr, n_cols = D.shape
    nth = 2 * nq + nu + nw + 2
    dq = np.zeros((T + 2, B, nq), dtype=LD)
    dgb = np.zeros((T, B, nr - nq), dtype=LD)
    dq[0], dq[1] = dq0, dq1
    for t in range(T):
        for r in range(B):
            th = np.zeros(nth, dtype=LD)
            th[:nq], th[nq:2 * nq], th[2 * nq:2 * nq + nu] = dq[t, r], dq[t + 1, r], du_step[t, r]
            if dw_step is not None:
                th[2 * nq + nu:2 * nq + nu + nw] = dw_step[t, r]
            if dmu is not None:
                th[nth - 2] = dmu[r]
            if dh is not None:
                th[nth - 1] = dh[r]
            dzt = np.asarray(D[t, r], dtype=LD) @ th[:n_cols]
            dq[t + 2, r], dgb[t, r] = dzt[:nq], dzt[nq:]
    return dq, dgb


def random_cotangents(rng, T, B, nq, nc, nb):
    return rng.standard_normal((T + 2, B, nq)), rng.standard_normal((T, B, nc)), rng.standard_normal((T, B, nb))
