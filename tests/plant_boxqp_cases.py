"""Restatements shared by the tests of the limited LQ backward pass (tests/test_plant_boxqp.py without a device, tests/test_gpu_plant_boxqp.py
on it): the definition of DESIGN.md section 3, item 3g (csrc/plant_boxqp.h inside the BOX chain of csrc/plant_riccati.h).  At every walk step
the chain of `plant_riccati_cases` forms Qu, Quu, Qux and G = Quu + ρ_b I, then with lo = u_lo − u_nom[t, b], hi = u_hi − u_nom[t, b]:

    projected Newton on min ½ x'Gx + Qu'x, lo ≤ x ≤ hi, from x = limit(k of the walk step before)      (not run when every bound is infinite)
    c = {i : (x_i = lo_i and g_i > 0) or (x_i = hi_i and g_i < 0)}, g = Qu + G x;  f the rest
    G_ff [K_f | y] = [Qux_f | Qu_f + G_fc x_c],  K rows of c = 0,  k_f = limit(−y),  k_c = x_c

three times, as `plant_riccati_cases` states the unlimited pass:
  `lq_box_f64`  in float64 in the ORDER the headers state (every sum one ascending chain, the elimination of `prc._solve_kernel_order` on the
                free rows and columns): what the host build and the kernel must give bit for bit;
  `lq_box_ld`   the same algorithm in longdouble on the DENSE A_t, B_t with `gains_ref.solve_ld`, `gains_ref.mm_ld`;
  `lq_box_np`   the dense algorithm in plain float64 NumPy (`@`, `numpy.linalg.solve`);
and `brute_force`, which shares nothing with them: all 3^m assignments of (free, at lo, at hi) in longdouble, the one that is feasible with
the right gradient signs.  Each lq_* returns prc's dict plus `clamped` (keep, B) ints, bit i = control i clamped; with trace=[] also one
record per walk step (b, t, G, Qu, lo, hi, k, mask)."""
import itertools

import numpy as np

import gains_ref as gr
import plant_adjoint_cases as pac
import plant_riccati_cases as prc

LD = np.longdouble
OUTPUTS = prc.OUTPUTS
# the constants of csrc/plant_boxqp.h
MAX_ITER, MIN_GRAD, ARMIJO, STEP_DEC, MIN_STEP = 100, 1e-8, 0.1, 0.6, 1e-22


def limit(u, lo, hi):
    """plant_feedback_limit, elementwise: lo where u < lo, hi where u > hi, u otherwise (a NaN u passes through)."""
    u, lo, hi = np.broadcast_arrays(np.asarray(u), np.asarray(lo), np.asarray(hi))
    return np.where(u < lo, lo, np.where(u > hi, hi, u))


def _row(a, b):
    a = np.asarray(a)
    return a[0 if a.shape[0] == 1 else b]


def _limits(u_lo, u_hi, u_nom, t, b, m, dtype):
    if u_lo is None:
        return np.full(m, -np.inf, dtype=dtype), np.full(m, np.inf, dtype=dtype)
    un = np.asarray(u_nom[t, b], dtype=np.float64)      # one rounded float64 difference each, in every restatement
    lo = np.asarray(_row(np.atleast_2d(u_lo), b), dtype=np.float64) - un
    hi = np.asarray(_row(np.atleast_2d(u_hi), b), dtype=np.float64) - un
    return lo.astype(dtype), hi.astype(dtype)


def _mask(c):
    return int(sum(1 << int(i) for i in np.flatnonzero(c)))


# ---- the float64 step in the order of csrc/plant_boxqp.h ------------------------------------------------------------------------------------
def _value(G, Qu, v):
    y = prc._osum(np.zeros(len(v)), G, v)
    a = b = 0.0
    for i in range(len(v)):
        a = a + float(v[i]) * float(y[i])
    for i in range(len(v)):
        b = b + float(Qu[i]) * float(v[i])
    return 0.5 * a + b


def box_step_f64(G, F, Qu, lo, hi, k_prev):
    """One walk step: G (m, m) with ρ on its diagonal, F = [Qux | Qu] (m, n + 1).  -> (X (m, n + 1) = [K | ·], k (m), clamped (m) bools, ok,
    iterations); ok False: the chain ends here."""
    m, n = len(G), F.shape[1] - 1
    x = limit(np.zeros(m) if k_prev is None else k_prev, lo, hi).astype(np.float64)
    c = np.zeros(m, dtype=bool)
    its = 0
    if not (np.all(lo == -np.inf) and np.all(hi == np.inf)):
        floor = MIN_GRAD * (1.0 + float(np.max(np.nan_to_num(np.abs(Qu), nan=0.0), initial=0.0)))
        done = False
        for _ in range(MAX_ITER):
            g = Qu + prc._osum(np.zeros(m), G, x)
            c = ((x == lo) & (g > 0.0)) | ((x == hi) & (g < 0.0))
            f = np.flatnonzero(~c)
            gmax = 0.0
            for i in f:
                a = abs(float(g[i]))
                if not a <= gmax:
                    gmax = a
            if len(f) == 0 or gmax <= floor:
                done = True
                break
            its += 1
            sol = prc._solve_kernel_order(G[np.ix_(f, f)], -g[f][:, None])
            if sol is None:
                return None, None, c, False, its
            d = np.zeros(m)
            d[f] = sol[:, 0]
            sdg = 0.0
            for i in f:
                sdg = sdg + float(d[i]) * float(g[i])
            if not sdg < 0.0:
                return None, None, c, False, its
            fo, step, took = _value(G, Qu, x), 1.0, False
            while step >= MIN_STEP:
                xc = limit(x + step * d, lo, hi)
                if _value(G, Qu, xc) - fo <= ARMIJO * (step * sdg):
                    took = True
                    break
                step = step * STEP_DEC
            if not took:
                return None, None, c, False, its
            x = xc
        if not done:
            return None, None, c, False, its
    f, cl = np.flatnonzero(~c), np.flatnonzero(c)
    y = np.array(F[:, n], dtype=np.float64)
    for j in cl:
        y = y + G[:, j] * x[j]
    X = np.zeros((m, n + 1))
    if len(f):
        sol = prc._solve_kernel_order(G[np.ix_(f, f)], np.concatenate([F[f, :n], y[f][:, None]], axis=1))
        if sol is None:
            return None, None, c, False, its
        X[f] = sol
    k = np.where(c, x, limit(-X[:, n], lo, hi))
    return X, k, c, True, its


def lq_box_f64(D, status, nq, nu, Q, R, Qf, q, r, rho=0.0, u_lo=None, u_hi=None, u_nom=None, keep=None, trace=None):
    T, B = D.shape[:2]
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    Q, R, Qf = (np.asarray(M, dtype=np.float64) for M in (Q, R, Qf))
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64).reshape(-1), (B,)) if np.size(rho) in (1, B) else None
    out = prc._empty(T, B, n, m, keep, True, np.float64)
    out["clamped"] = np.zeros((keep, B), dtype=np.int32)
    out["iterations"] = np.zeros((T, B), dtype=np.int32)
    out["n_cut"][:] = (np.asarray(status) == 0).sum(axis=0)
    Z, at = np.zeros, prc._at
    with np.errstate(all="ignore"):
        for b in range(B):
            P, p = Qf.copy(), np.array(q[T, b], dtype=np.float64)
            dV1 = dV2 = 0.0
            fail, kv = 0, None
            for s in range(1, T + 1):
                t = T - s
                Dx, Du = np.asarray(D[t, b, :nq, :n], dtype=np.float64), np.asarray(D[t, b, :nq, n:n + m], dtype=np.float64)
                Qt, Rt = at(Q, t, 2), at(R, t, 2)
                BtP = prc._osum(Z((m, n)), Du.T, P[nq:, :])
                V = prc._osum(np.concatenate([Z((m, m + nq)), BtP[:, :nq]], axis=1), BtP[:, nq:], np.concatenate([Du, Dx], axis=1))
                Quu = Rt + V[:, :m]
                G = Quu.copy()
                G[np.arange(m), np.arange(m)] = np.diag(Quu) + rho[b]
                rt = np.asarray(r[t, b], dtype=np.float64)
                Qu = rt + prc._osum(Z(m), Du.T, p[nq:])
                F = np.concatenate([V[:, m:], Qu[:, None]], axis=1)
                lo, hi = _limits(u_lo, u_hi, u_nom, t, b, m, np.float64)
                X, kv, c, ok, its = box_step_f64(G, F, Qu, lo, hi, kv)
                out["iterations"][t, b] = its
                if not ok:
                    fail = s
                    break
                K = X[:, :n]
                ok = np.isfinite(X).all()
                Dcl = Dx - prc._osum(Z((nq, n)), Du, K)
                RK = prc._osum(Z((m, n)), Rt, K)
                T1 = prc._osum(np.concatenate([Z((n, nq)), P[:, :nq]], axis=1), P[:, nq:], Dcl)
                Pn = (Qt + prc._osum(Z((n, n)), K.T, RK)) + prc._osum(np.concatenate([Z((nq, n)), T1[:nq]], axis=0), Dcl.T, T1[nq:])
                ok = ok and np.isfinite(Pn).all()
                dV1 = dV1 + float(prc._osum(Z(1), kv[None, :], Qu)[0])
                dV2 = dV2 + 0.5 * float(prc._osum(Z(1), kv[None, :], prc._osum(Z(m), Quu, kv))[0])
                Duk, Rk = prc._osum(Z(nq), Du, kv), prc._osum(Z(m), Rt, kv)
                sv = prc._osum(Z(n), P[:, nq:], Duk) + p
                pn = ((np.asarray(q[t, b], dtype=np.float64) - prc._osum(Z(n), K.T, rt)) - prc._osum(Z(n), K.T, Rk)) + \
                    prc._osum(np.concatenate([Z(nq), sv[:nq]]), Dcl.T, sv[nq:])
                ok = ok and np.isfinite(pn).all()
                if not ok:
                    fail = s
                    break
                if trace is not None:
                    trace.append(dict(b=b, t=t, G=G, Qu=Qu, lo=lo, hi=hi, k=kv.copy(), K=K.copy(), mask=_mask(c)))
                P, p = Pn, pn
                if t < keep:
                    out["K"][t, b], out["k"][t, b], out["clamped"][t, b] = K, kv, _mask(c)
            if fail:
                prc._fail(out, b, fail)
                out["clamped"][:, b] = 0
            else:
                out["P0"][b], out["p0"][b], out["dV"][b] = P, p, (dV1, dV2)
    return out


# ---- the dense algorithm in longdouble and in plain NumPy -----------------------------------------------------------------------------------
def _box_step_dense(G, Qux, Qu, lo, hi, k_prev, dtype, mm, solve):
    m = len(G)
    x = limit(np.zeros(m, dtype=dtype) if k_prev is None else k_prev, lo, hi).astype(dtype)
    c = np.zeros(m, dtype=bool)
    value = lambda v: dtype(0.5) * mm(v, mm(G, v)) + mm(Qu, v)
    if not (np.all(lo == -np.inf) and np.all(hi == np.inf)):
        floor = dtype(MIN_GRAD) * (1 + np.max(np.abs(Qu)))
        for _ in range(MAX_ITER):
            g = Qu + mm(G, x)
            c = ((x == lo) & (g > 0)) | ((x == hi) & (g < 0))
            f = np.flatnonzero(~c)
            if len(f) == 0 or np.max(np.abs(g[f])) <= floor:
                break
            d = np.zeros(m, dtype=dtype)
            d[f] = solve(G[np.ix_(f, f)], -g[f])
            sdg = mm(d, g)
            assert sdg < 0, "the dense restatement met a direction that is no descent direction"
            fo, step = value(x), dtype(1.0)
            while True:
                xc = limit(x + step * d, lo, hi).astype(dtype)
                if value(xc) - fo <= dtype(ARMIJO) * (step * sdg):
                    break
                step = step * dtype(STEP_DEC)
                assert step >= MIN_STEP
            x = xc
        else:
            raise AssertionError("the dense restatement did not converge")
    f, cl = np.flatnonzero(~c), np.flatnonzero(c)
    K, k = np.zeros(Qux.shape, dtype=dtype), x.copy()
    if len(f):
        y = Qu[f] + (mm(G[np.ix_(f, cl)], x[cl]) if len(cl) else 0)
        X = solve(G[np.ix_(f, f)], np.concatenate([Qux[f], y[:, None]], axis=1))
        K[f] = X[:, :-1]
        k[f] = limit(-X[:, -1], lo[f], hi[f])
    return K, k, c


def _dense_box(D, status, nq, nu, Q, R, Qf, q, r, rho, u_lo, u_hi, u_nom, keep, dtype, mm, solve):
    T, B = D.shape[:2]
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    Q, R, Qf = (np.asarray(M, dtype=dtype) for M in (Q, R, Qf))
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64).reshape(-1), (B,))
    out = prc._empty(T, B, n, m, keep, True, dtype)
    out["clamped"] = np.zeros((keep, B), dtype=np.int32)
    out["n_cut"][:] = (np.asarray(status) == 0).sum(axis=0)
    half = dtype(0.5)
    for b in range(B):
        P, p, dV, kv = Qf.copy(), np.asarray(q[T, b], dtype=dtype), np.zeros(2, dtype=dtype), None
        for s in range(1, T + 1):
            t = T - s
            A, Bm = prc.dense_AB(D[t, b], nq, nu, dtype)
            Qt, Rt = prc._at(Q, t, 2), prc._at(R, t, 2)
            BtP = mm(Bm.T, P)
            Quu = Rt + mm(BtP, Bm)
            rt = np.asarray(r[t, b], dtype=dtype)
            Qu = rt + mm(Bm.T, p)
            lo, hi = _limits(u_lo, u_hi, u_nom, t, b, m, dtype)
            K, kv, c = _box_step_dense(Quu + dtype(rho[b]) * np.eye(m, dtype=dtype), mm(BtP, A), Qu, lo, hi, kv, dtype, mm, solve)
            Acl = A - mm(Bm, K)
            dV[0] += mm(kv, Qu)
            dV[1] += half * mm(kv, mm(Quu, kv))
            p = np.asarray(q[t, b], dtype=dtype) - mm(K.T, rt) - mm(K.T, mm(Rt, kv)) + mm(Acl.T, mm(P, mm(Bm, kv)) + p)
            P = Qt + mm(K.T, mm(Rt, K)) + mm(Acl.T, mm(P, Acl))
            if t < keep:
                out["K"][t, b], out["k"][t, b], out["clamped"][t, b] = K, kv, _mask(c)
        out["P0"][b], out["p0"][b], out["dV"][b] = P, p, dV
    return out


def lq_box_ld(D, status, nq, nu, Q, R, Qf, q, r, rho=0.0, u_lo=None, u_hi=None, u_nom=None, keep=None):
    return _dense_box(D, status, nq, nu, Q, R, Qf, q, r, rho, u_lo, u_hi, u_nom, keep, LD, gr.mm_ld, gr.solve_ld)


def lq_box_np(D, status, nq, nu, Q, R, Qf, q, r, rho=0.0, u_lo=None, u_hi=None, u_nom=None, keep=None):
    return _dense_box(D, status, nq, nu, Q, R, Qf, q, r, rho, u_lo, u_hi, u_nom, keep, np.float64, lambda X, Y: X @ Y, np.linalg.solve)


def bounds(*args, **kw):
    """(lq_box_ld, lq_box_f64, {output: 100 x max(d(lq_box_np, lq_box_ld), 2.2e-16)}), the rule of `plant_riccati_cases.bounds`."""
    ld, f64, plain = (fn(*args, **kw) for fn in (lq_box_ld, lq_box_f64, lq_box_np))
    return ld, f64, {k: prc.FACTOR * max(pac.distance(plain[k], ld[k]), 2.2e-16) for k in OUTPUTS}


# ---- the oracle that shares nothing: every active set ------------------------------------------------------------------------------------------
def brute_force(G, Qu, lo, hi):
    """All 3^m assignments (free, at lo, at hi) in longdouble: the (x, mask) that is feasible, with g = Qu + G x zero on the free set (by the
    solve), g > 0 at lo and g < 0 at hi.  Exactly one for a G with a positive definite symmetric part."""
    m = len(G)
    G, Qu, lo, hi = (np.asarray(a, dtype=LD) for a in (G, Qu, lo, hi))
    found = []
    for assign in itertools.product((0, 1, 2), repeat=m):
        a = np.array(assign)
        if np.any((a == 1) & ~np.isfinite(lo)) or np.any((a == 2) & ~np.isfinite(hi)):
            continue
        x = np.where(a == 1, lo, np.where(a == 2, hi, LD(0)))
        f, cl = np.flatnonzero(a == 0), np.flatnonzero(a != 0)
        if len(f):
            rhs = -(Qu[f] + (gr.mm_ld(G[np.ix_(f, cl)], x[cl]) if len(cl) else 0))
            x[f] = gr.solve_ld(G[np.ix_(f, f)], rhs)
        g = Qu + gr.mm_ld(G, x)
        if np.all(x >= lo) and np.all(x <= hi) and np.all(g[a == 1] > 0) and np.all(g[a == 2] < 0):
            found.append((x, _mask(a != 0)))
    return found


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
# name: (nq, nu, nr, n_cols, T, B, dict(rho, per_step, shared limits, keep))
SHAPES = {
    "nu 2, one step": (2, 2, 5, 7, 1, 1, dict(rho=0.0)),
    "nu 2, six steps, two robots, a rho each": (2, 2, 5, 7, 6, 2, dict(rho=(0.0, 0.5))),
    "nu 3, strided block, per-step weights, shared limits, keep 5": (3, 3, 7, 10, 14, 2, dict(rho=0.25, per_step=True, shared=True, keep=5)),
    "nu 8, the quadruped's sizes": (11, 8, 23, 32, 4, 2, dict(rho=(1e-3, 0.0))),
    "nu 12, the largest model": (18, 12, 58, 53, 3, 2, dict(rho=1e-3)),
}


def case(name, seed=0, tight=1.0, symmetric=False):
    """Synthetic blocks and non-symmetric weights as `test_plant_riccati._case`, and limits placed from the UNLIMITED pass: u_nom = 0.1 h ξ,
    u_lo = −tight h, u_hi = +tight h with h the median |k| of the unlimited chain (per robot, or of all with shared limits), so that some
    but not all controls clamp.  The weights are `prc.weights` plus a small non-symmetric part (G = Quu + ρ I is not symmetric, and nothing
    symmetrizes it); symmetric=True leaves that part out, for the identities that hold for symmetric weights alone.  -> (D, status, (nq, nu, Q, R, Qf, q, r), dict(rho, u_lo, u_hi, u_nom, keep))."""
    nq, nu, nr, n_cols, T, B, o = SHAPES[name]
    n, m = 2 * nq, nu
    rng = np.random.default_rng([seed, sorted(SHAPES).index(name), 77])
    D = rng.standard_normal((T, B, nr, n_cols)) / np.sqrt(n_cols)
    status = np.ones((T, B), dtype=np.int32)
    Q, R, Qf = prc.weights(rng, n, m, T, o.get("per_step", False))
    skew = 0.0 if symmetric else 1.0      # the draws are made either way, so that both variants share everything else
    Q, R, Qf = Q + skew * 1e-3 * rng.standard_normal(Q.shape), R + skew * 1e-4 * rng.standard_normal(R.shape), Qf + skew * 1e-3 * rng.standard_normal(Qf.shape)
    q, r = rng.standard_normal((T + 1, B, n)), rng.standard_normal((T, B, m))
    rho = np.asarray(o["rho"], dtype=np.float64).reshape(-1)
    free = prc.lq_f64(D, status, nq, nu, Q, R, Qf, q=q, r=r, rho=float(rho[0]))
    h = np.median(np.abs(free["k"]), axis=(0, 2))                    # (B,)
    if o.get("shared"):
        h = np.full(B, np.median(np.abs(free["k"])))
    u_nom = 0.1 * h[None, :, None] * rng.standard_normal((T, B, m))
    u_lo, u_hi = -tight * h[:, None] * np.ones((B, m)), tight * h[:, None] * np.ones((B, m))
    if o.get("shared"):
        u_lo, u_hi = u_lo[:1], u_hi[:1]
    return D, status, (nq, nu, Q, R, Qf, q, r), dict(rho=rho if rho.size > 1 else float(rho[0]), u_lo=u_lo, u_hi=u_hi, u_nom=u_nom, keep=o.get("keep"))


def clamped_counts(clamped, nu):
    """Per robot, how many (step, control) pairs are clamped: (B,)."""
    return np.array([[bin(int(v)).count("1") for v in row] for row in np.asarray(clamped).T]).sum(axis=1)


# ---- limited iLQR on the CPU plant ------------------------------------------------------------------------------------------------------------
def _cpu_rollout_limited(case, P, u_bar, u_lo, u_hi, K=None, x_ref=None):
    """`plant_linesearch_cases._cpu_rollout` under the limited law: u_t = limit(ū_t + K_t (x_ref[t] − x_t)), limits (1 or B, nu)."""
    import plant_gradient_cases as pgc
    from oracle import plant as pl
    nq, nu, nc, nb, nw, nz, nth, nr = pgc.dims(case["model"])
    B, T, h = case["q1"].shape[0], case["T"], case["h"]
    q, ua = np.zeros((T + 2, B, nq)), np.zeros((T, B, nu))
    st, Z, TH = np.zeros((T, B), dtype=bool), np.zeros((T, B, nz)), np.zeros((T, B, nth))
    for b in range(B):
        q[0, b], q[1, b] = case["q1"][b] - h * case["v1"][b], case["q1"][b]
        for t in range(T):
            u = np.array(u_bar[t, b], dtype=np.float64)
            if K is not None:
                x = np.concatenate([q[t + 1, b] - 1.0 * (q[t + 1, b] - q[t, b]), q[t + 1, b]])
                e = x_ref[t, b] - x
                s = np.zeros(nu)
                for j in range(2 * nq):
                    s = s + K[t, b, :, j] * e[j]
                u = u + s
            u = limit(u, _row(u_lo, b), _row(u_hi, b))
            ua[t, b] = u
            st[t, b], Z[t, b], TH[t, b] = pgc.cpu_step_z(P, q[t, b], q[t + 1, b], u, np.zeros(nw), case["mu"][b], h, pl.SIM_OPTS)
            q[t + 2, b] = Z[t, b, :nq]
    return q, ua, st, Z, TH


def projected_gradient_ld(D, u, lin_q, lin_r, nq, nu, u_lo, u_hi):
    """The gradient of J with respect to every control of the horizon through the linearized steps, by the longdouble adjoint chain
    λ_T = q_T, g_t = r_t + B_t'λ_{t+1}, λ_t = q_t + A_t'λ_{t+1}, projected on the box: an entry on its lower limit with g > 0 or on its upper
    limit with g < 0 counts as zero.  -> (T, B, nu) longdouble."""
    T, B = u.shape[:2]
    g = np.zeros((T, B, nu), dtype=LD)
    for b in range(B):
        lam = np.asarray(lin_q[T, b], dtype=LD)
        for t in range(T - 1, -1, -1):
            A, Bm = prc.dense_AB(D[t, b], nq, nu, LD)
            g[t, b] = np.asarray(lin_r[t, b], dtype=LD) + gr.mm_ld(Bm.T, lam)
            lam = np.asarray(lin_q[t, b], dtype=LD) + gr.mm_ld(A.T, lam)
    lo, hi = np.atleast_2d(u_lo)[None], np.atleast_2d(u_hi)[None]
    held = ((u == lo) & (g > 0)) | ((u == hi) & (g < 0))
    return np.where(held, LD(0), g)


def ilqr_cpu_box(case, Q, R, Qf, x_goal, u_goal, alphas, n_iter, u_lo, u_hi, rho=0.0, armijo=1e-4):
    """`plant_linesearch_cases.ilqr_cpu` under control limits: the initial controls clipped into the box, the
    backward pass `lq_box_f64` about the nominal's controls, the candidates' rows limit(u + α k) under the limited law.  A list with one dict
    per iteration: J_nom, J_new, accepted, u, q, clamped, pg (max |projected gradient| about the nominal the iteration STARTED from), and
    after the last one `pg_end` about the final nominal."""
    import plant_gradient_cases as pgc
    import plant_linesearch_cases as plc
    nq, nu = pgc.dims(case["model"])[:2]
    P = pgc.cpu_plant(case)
    B, T = case["q1"].shape[0], case["T"]
    lo, hi = np.atleast_2d(np.asarray(u_lo, dtype=np.float64)), np.atleast_2d(np.asarray(u_hi, dtype=np.float64))
    u0 = limit(np.broadcast_to(case["u"], (T, B, nu)), lo[None], hi[None])
    q, ua, st, Z, TH = _cpu_rollout_limited(case, P, u0, lo, hi)
    J, lq, lr = plc.cost_f64(q, ua, Q, R, Qf, x_goal, u_goal)
    blocks = lambda Z, TH: np.array([[np.asarray(r["ld"], dtype=np.float64) for r in row] for row in pgc.rollout_references(case, Z, TH, pgc.REG, 2 * nq + nu)])
    out = []
    for _ in range(n_iter):
        D = blocks(Z, TH)
        pg = float(np.abs(projected_gradient_ld(D, ua, lq, lr, nq, nu, lo, hi)).max())
        g = lq_box_f64(D, st.astype(np.int32), nq, nu, Q, R, Qf, lq, lr, rho=rho, u_lo=lo, u_hi=hi, u_nom=ua)
        x_ref = np.concatenate([q[1:T + 1] - 1.0 * (q[1:T + 1] - q[:T]), q[1:T + 1]], axis=2)
        cands = [_cpu_rollout_limited(case, P, limit(plc.candidate_controls(ua, a, g["k"]), lo[None], hi[None]), lo, hi, g["K"], x_ref) for a in alphas]
        Jc = np.array([plc.cost_f64(c[0], c[1], Q, R, Qf, x_goal, u_goal)[0] for c in cands])
        ok = np.array([[plc.acceptable(cands[c][2][:, b].all(), Jc[c, b], J[b], armijo, alphas[c], g["dV"][b, 0], g["dV"][b, 1]) for b in range(B)]
                       for c in range(len(alphas))])
        choice = np.array([plc.choose(Jc[:, b], ok[:, b]) for b in range(B)])
        it = dict(J_nom=J.copy(), J=Jc, ok=ok, choice=choice, dV=g["dV"], clamped=g["clamped"], status=g["status"], accepted=choice >= 0, pg=pg)
        nq_, nua, nst, nZ, nTH = (np.array(a) for a in (q, ua, st, Z, TH))
        for b in range(B):
            if choice[b] >= 0:
                cq, cu, cs, cZ, cT = cands[choice[b]]
                nq_[:, b], nua[:, b], nst[:, b], nZ[:, b], nTH[:, b] = cq[:, b], cu[:, b], cs[:, b], cZ[:, b], cT[:, b]
        q, ua, st, Z, TH = nq_, nua, nst, nZ, nTH
        J, lq, lr = plc.cost_f64(q, ua, Q, R, Qf, x_goal, u_goal)
        it.update(u=ua.copy(), q=q.copy(), J_new=J.copy())
        out.append(it)
    out[-1]["pg_end"] = float(np.abs(projected_gradient_ld(blocks(Z, TH), ua, lq, lr, nq, nu, lo, hi)).max())
    return out


FLIGHT_ALPHAS, FLIGHT_ITERATIONS, FLIGHT_FRACTION = (1.0, 0.5, 0.25), 2, 0.5


def flight_limits():
    """The flight case of `plant_linesearch_cases` with a thrust limit that binds: per particle ±FLIGHT_FRACTION of the largest |u| its
    unlimited LQ step asks for (one full step of `ilqr_cpu`), the same for its three controls.  -> (u_lo, u_hi), each (B, 3)."""
    import plant_linesearch_cases as plc
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    free = plc.ilqr_cpu(case, Q, R, Qf, x_goal, u_goal, (1.0,), 1)[0]
    bound = FLIGHT_FRACTION * np.abs(free["u"]).max(axis=(0, 2))
    hi = np.repeat(bound[:, None], 3, axis=1)
    return -hi, hi


def flight_cpu():
    """FLIGHT_ITERATIONS iterations of `ilqr_cpu_box` on the flight case under `flight_limits`: the list of its iterations."""
    import plant_linesearch_cases as plc
    case, Q, R, Qf, x_goal, u_goal = plc.flight_case()
    u_lo, u_hi = flight_limits()
    return ilqr_cpu_box(case, Q, R, Qf, x_goal, u_goal, FLIGHT_ALPHAS, FLIGHT_ITERATIONS, u_lo, u_hi)
