"""Restatements of csrc/plant_shooting.h shared by tests/test_plant_shooting.py (without a device) and
tests/test_gpu_plant_shooting.py (on it).

Layout: T = M L; segment j of robot b is virtual robot r = j B + b of a rollout of M B robots for L steps, qs (L + 2, M B, nq); node j is
[qs[0, r]; qs[1, r]]; step l of segment j is global step j L + l.

    stage_states   x_t = [qs[l, r]; qs[l + 1, r]] of the segment that owns step t (t < T), x_T = [qs[L, r]; qs[L + 1, r]] of the last
    defects        d_j = [qs[L, (j-1) B + b]; qs[L + 1, (j-1) B + b]] - node j, j = 1 .. M-1;  D = the running sum of |d_j[i]|, ascending j then i
    cost_f64       the tracking cost on those states in float64 in the ORDER the header states (plant_cost.h's chains, J ascending in global t)
    cost_ld        the same in longdouble, whichever order NumPy takes
    merit          phi = J + weight D, one rounded product and one rounded sum
    spread / stitch   (T, B, ...) rows to the virtual robots' (L, M B, ...) and back
"""
import numpy as np

import plant_adjoint_cases as pac
import plant_linesearch_cases as plc

LD = np.longdouble
FACTOR = pac.FACTOR


def spread(a, M):
    """(T, B, ...) in global layout -> (L, M B, ...): row l of virtual robot j B + b is row j L + l of robot b."""
    a = np.asarray(a)
    T, B = a.shape[:2]
    L = T // M
    return np.ascontiguousarray(np.moveaxis(a.reshape((M, L, B) + a.shape[2:]), 0, 1).reshape((L, M * B) + a.shape[2:]))


def stitch(a, M):
    """(L, M B, ...) of the virtual robots -> (T, B, ...) in global layout."""
    a = np.asarray(a)
    L, MB = a.shape[:2]
    B = MB // M
    return np.ascontiguousarray(np.moveaxis(a.reshape((L, M, B) + a.shape[2:]), 1, 0).reshape((M * L, B) + a.shape[2:]))


def stage_states(qs, M, dtype=np.float64):
    """x (T + 1, B, 2nq): the state every stage of the cost is taken on."""
    qs = np.asarray(qs, dtype=dtype)
    L, B = qs.shape[0] - 2, qs.shape[1] // M
    x = stitch(np.concatenate([qs[:L], qs[1:L + 1]], axis=2), M)
    last = np.concatenate([qs[L, (M - 1) * B:], qs[L + 1, (M - 1) * B:]], axis=1)
    return np.concatenate([x, last[None]], axis=0)


def defects(qs, M, dtype=np.float64):
    """d (M - 1, B, 2nq)."""
    qs = np.asarray(qs, dtype=dtype)
    L, B, nq = qs.shape[0] - 2, qs.shape[1] // M, qs.shape[2]
    d = np.zeros((M - 1, B, 2 * nq), dtype=dtype)
    for j in range(1, M):
        prev, own = slice((j - 1) * B, j * B), slice(j * B, (j + 1) * B)
        d[j - 1, :, :nq] = qs[L, prev] - qs[0, own]
        d[j - 1, :, nq:] = qs[L + 1, prev] - qs[1, own]
    return d


def defect_sum(d):
    """D (B,): one running sum from 0.0 in ascending j, then i."""
    D = np.zeros(d.shape[1], dtype=d.dtype)
    for j in range(d.shape[0]):
        for i in range(d.shape[2]):
            D = D + np.abs(d[j, :, i])
    return D


def _cost_on_states(x, u, Q, R, Qf, x_goal, u_goal):
    """`plant_linesearch_cases.cost_f64` on given states x (T + 1, B, n) in place of a trajectory's consecutive rows: the same chains."""
    T = u.shape[0]
    ex, eu = x - np.asarray(x_goal, dtype=np.float64), np.asarray(u, dtype=np.float64) - np.asarray(u_goal, dtype=np.float64)
    Qs, Rs = plc._stack(Q, Qf, T, np.float64), plc._steps(R, T, np.float64)

    def matvec(Ms, e):
        out = np.zeros_like(e)
        for j in range(e.shape[2]):
            out = out + Ms[:, None, :, j] * e[:, :, j, None]
        return out

    def dot(a, b):
        s = np.zeros(a.shape[:2])
        for i in range(a.shape[2]):
            s = s + a[:, :, i] * b[:, :, i]
        return s
    qx, ru = matvec(Qs, ex), matvec(Rs, eu)
    lx, lu = 0.5 * dot(ex, qx), 0.5 * dot(eu, ru)
    J = lx[0] + lu[0]
    for t in range(1, T):
        J = J + (lx[t] + lu[t])
    J = J + lx[T]
    return J, qx, ru


def cost_f64(qs, u, M, Q, R, Qf, x_goal, u_goal):
    """(J (B,), D (B,), defects, lin_q (T + 1, B, n), lin_r (T, B, m)) in the header's order."""
    d = defects(qs, M)
    J, lq, lr = _cost_on_states(stage_states(qs, M), u, Q, R, Qf, x_goal, u_goal)
    return J, defect_sum(d), d, lq, lr


def cost_ld(qs, u, M, Q, R, Qf, x_goal, u_goal, dtype=LD):
    """The same outputs in longdouble (dtype=np.float64: plain NumPy), whichever order NumPy takes."""
    T = u.shape[0]
    x = stage_states(qs, M, dtype)
    ex, eu = x - np.asarray(x_goal, dtype=dtype), np.asarray(u, dtype=dtype) - np.asarray(u_goal, dtype=dtype)
    Qs, Rs = plc._stack(Q, Qf, T, dtype), plc._steps(R, T, dtype)
    qx, ru = np.einsum("tij,tbj->tbi", Qs, ex), np.einsum("tij,tbj->tbi", Rs, eu)
    J = dtype(0.5) * (np.einsum("tbi,tbi->b", ex, qx) + np.einsum("tbi,tbi->b", eu, ru))
    d = defects(qs, M, dtype)
    return J, np.abs(d).sum(axis=(0, 2)), d, qx, ru


NAMES = ("J", "D", "defects", "lin_q", "lin_r")


def cost_bounds(*case):
    """(cost_ld's outputs, cost_f64's, {name: FACTOR x max(d(plain NumPy, cost_ld), 2.2e-16)}), the bounds relative to max|cost_ld|, as
    `plant_linesearch_cases.cost_bounds` builds them: from the restatements alone."""
    ld, f64, plain = cost_ld(*case), cost_f64(*case), cost_ld(*case, dtype=np.float64)
    dist = lambda a, ref: pac.distance(a, ref) if np.size(ref) else 0.0      # M = 1 has no defect
    return dict(zip(NAMES, ld)), dict(zip(NAMES, f64)), {k: FACTOR * max(dist(plain[i], ld[i]), 2.2e-16) for i, k in enumerate(NAMES)}


def merit(J, weight, D):
    return np.asarray(J, dtype=np.float64) + np.asarray(weight, dtype=np.float64) * np.asarray(D, dtype=np.float64)


# ---- the backward pass with defects (csrc/plant_riccati.h: THE DEFECT HOOK) --------------------------------------------------------------------
def lq_shoot_f64(D, status, nq, nu, Q, R, Qf, q, r, rho, defects, seg_len, keep=None):
    """`plant_riccati_cases.lq_f64` with linear terms, a rho per robot ((B,) or a number) and the hook: at the top of the walk step of t, if
    t + 1 is a node j = (t + 1) / seg_len, p <- p + P d_j, (P d)[c] one running sum over ascending k from 0.0.  No limits: with every limit
    infinite the limited chain runs these statements.  The dict of `lq_f64`."""
    import plant_riccati_cases as prc
    T, B = D.shape[:2]
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (B,))
    Q, R, Qf = (np.asarray(M, dtype=np.float64) for M in (Q, R, Qf))
    out = prc._empty(T, B, n, m, keep, True, np.float64)
    out["n_cut"][:] = (np.asarray(status) == 0).sum(axis=0)
    Z, osum = np.zeros, prc._osum
    with np.errstate(all="ignore"):
        for b in range(B):
            P, p = Qf.copy(), np.array(q[T, b], dtype=np.float64)
            dV1 = dV2 = 0.0
            fail = 0
            for s in range(1, T + 1):
                t = T - s
                if t + 1 < T and (t + 1) % seg_len == 0:
                    p = p + osum(Z(n), P, np.asarray(defects[(t + 1) // seg_len - 1, b], dtype=np.float64))
                Dx, Du = np.asarray(D[t, b, :nq, :n], dtype=np.float64), np.asarray(D[t, b, :nq, n:n + m], dtype=np.float64)
                Qt, Rt = prc._at(Q, t, 2), prc._at(R, t, 2)
                BtP = osum(Z((m, n)), Du.T, P[nq:, :])
                V = osum(np.concatenate([Z((m, m + nq)), BtP[:, :nq]], axis=1), BtP[:, nq:], np.concatenate([Du, Dx], axis=1))
                Quu = Rt + V[:, :m]
                G = Quu.copy()
                G[np.arange(m), np.arange(m)] = np.diag(Quu) + rho[b]
                rt = np.asarray(r[t, b], dtype=np.float64)
                Qu = rt + osum(Z(m), Du.T, p[nq:])
                X = prc._solve_kernel_order(G, np.concatenate([V[:, m:], Qu[:, None]], axis=1))
                if X is None:
                    fail = s
                    break
                K, kv = X[:, :n], -X[:, n]
                ok = np.isfinite(X).all()
                Dcl = Dx - osum(Z((nq, n)), Du, K)
                RK = osum(Z((m, n)), Rt, K)
                T1 = osum(np.concatenate([Z((n, nq)), P[:, :nq]], axis=1), P[:, nq:], Dcl)
                Pn = (Qt + osum(Z((n, n)), K.T, RK)) + osum(np.concatenate([Z((nq, n)), T1[:nq]], axis=0), Dcl.T, T1[nq:])
                dV1 = dV1 + float(osum(Z(1), kv[None, :], Qu)[0])
                dV2 = dV2 + 0.5 * float(osum(Z(1), kv[None, :], osum(Z(m), Quu, kv))[0])
                Duk, Rk = osum(Z(nq), Du, kv), osum(Z(m), Rt, kv)
                sv = osum(Z(n), P[:, nq:], Duk) + p
                pn = ((np.asarray(q[t, b], dtype=np.float64) - osum(Z(n), K.T, rt)) - osum(Z(n), K.T, Rk)) + \
                    osum(np.concatenate([Z(nq), sv[:nq]]), Dcl.T, sv[nq:])
                if not (ok and np.isfinite(Pn).all() and np.isfinite(pn).all()):
                    fail = s
                    break
                P, p = Pn, pn
                if t < keep:
                    out["K"][t, b], out["k"][t, b] = K, kv
            if fail:
                prc._fail(out, b, fail)
            else:
                out["P0"][b], out["p0"][b], out["dV"][b] = P, p, (dV1, dV2)
    return out


def node_defect(defects, seg_len, t1, b, n, dtype):
    """d of state t1 (1 .. T): the defect of node t1 / seg_len where t1 is a node before T, zeros otherwise."""
    T = (defects.shape[0] + 1) * seg_len
    if t1 < T and t1 % seg_len == 0:
        return np.asarray(defects[t1 // seg_len - 1, b], dtype=dtype)
    return np.zeros(n, dtype=dtype)


def forward_linear(D, b, nq, nu, K, k, defects, seg_len, dtype=LD):
    """The linear forward pass of robot b at alpha = 1: dx_0 = 0, du_t = k_t - K_t dx_t, dx_{t+1} = A_t dx_t + B_t du_t + d_{t+1}.
    (du (T, m), dx (T + 1, n)) in `dtype`, whichever order NumPy takes."""
    import plant_riccati_cases as prc
    T, n = D.shape[0], 2 * nq
    dx, du = np.zeros((T + 1, n), dtype=dtype), np.zeros((T, nu), dtype=dtype)
    for t in range(T):
        A, Bm = prc.dense_AB(D[t, b], nq, nu, dtype)
        du[t] = np.asarray(k[t, b], dtype=dtype) - np.asarray(K[t, b], dtype=dtype) @ dx[t]
        dx[t + 1] = A @ dx[t] + Bm @ du[t] + node_defect(defects, seg_len, t + 1, b, n, dtype)
    return du, dx


def lq_optimum_defects_ld(D, b, nq, nu, Q, R, Qf, lin_q, lin_r, defects, seg_len):
    """`plant_linesearch_cases.lq_optimum_ld` with the defect right-hand side: robot b's minimizer of the quadratic model subject to
    dx_{t+1} = A_t dx_t + B_t du_t + d_{t+1}, dx_0 = 0, as one dense KKT system in longdouble.  (du (T, m), dx (T + 1, n), the value)."""
    import gains_ref as gr
    import plant_riccati_cases as prc
    T, n, m = D.shape[0], 2 * nq, nu
    Qs, Rs = plc._stack(Q, Qf, T, LD), plc._steps(R, T, LD)
    nx, nuu = T * n, T * m
    N = nx + nuu
    H, g, E, rhs = np.zeros((N, N), dtype=LD), np.zeros(N, dtype=LD), np.zeros((nx, N), dtype=LD), np.zeros(nx, dtype=LD)
    for t in range(1, T + 1):
        s = slice((t - 1) * n, t * n)
        H[s, s] = LD(0.5) * (Qs[t] + Qs[t].T)
        g[s] = np.asarray(lin_q[t, b], dtype=LD)
        rhs[s] = node_defect(defects, seg_len, t, b, n, LD)
    for t in range(T):
        s = slice(nx + t * m, nx + (t + 1) * m)
        H[s, s] = LD(0.5) * (Rs[t] + Rs[t].T)
        g[s] = np.asarray(lin_r[t, b], dtype=LD)
        A, Bm = prc.dense_AB(D[t, b], nq, nu, LD)
        E[t * n:(t + 1) * n, t * n:(t + 1) * n] = np.eye(n, dtype=LD)
        if t > 0:
            E[t * n:(t + 1) * n, (t - 1) * n:t * n] = -A
        E[t * n:(t + 1) * n, s] = -Bm
    KKT = np.block([[H, E.T], [E, np.zeros((nx, nx), dtype=LD)]])
    y = gr.solve_ld(KKT, np.concatenate([-g, rhs])[:, None])[:N, 0]
    return y[nx:].reshape(T, m), np.concatenate([np.zeros((1, n), dtype=LD), y[:nx].reshape(T, n)]), g @ y + LD(0.5) * (y @ (H @ y))


def last_place(rng, a):
    """A copy of `a` with every entry moved one place up or down, by a seeded coin."""
    a = np.asarray(a, dtype=np.float64)
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


# ---- the linear forward pass (csrc/plant_shooting.h: THE LINEAR FORWARD PASS) -----------------------------------------------------------------
def forward_f64(D, nq, nu, K, k, Q, R, Qf, lin_q, lin_r, defects, seg_len):
    """`plant_shoot_forward_chain` in float64 in the ORDER the header states: (dx_nodes (M - 1, B, n), du (T, B, m), dJ (B, 2))."""
    import plant_riccati_cases as prc
    T, B = D.shape[:2]
    n, m, M = 2 * nq, nu, D.shape[0] // seg_len
    Q, R, Qf = (np.asarray(A, dtype=np.float64) for A in (Q, R, Qf))
    Z, osum = np.zeros, prc._osum
    dot = lambda a, b: float(osum(Z(1), np.asarray(a, dtype=np.float64)[None, :], np.asarray(b, dtype=np.float64))[0])
    dxn, du, dJ = Z((M - 1, B, n)), Z((T, B, m)), Z((B, 2))
    for b in range(B):
        x, a1, a2 = Z(n), 0.0, 0.0
        for t in range(T):
            Dx, Du = np.asarray(D[t, b, :nq, :n], dtype=np.float64), np.asarray(D[t, b, :nq, n:n + m], dtype=np.float64)
            u = np.asarray(k[t, b], dtype=np.float64) - osum(Z(m), np.asarray(K[t, b], dtype=np.float64), x)
            qx, ru = osum(Z(n), prc._at(Q, t, 2), x), osum(Z(m), prc._at(R, t, 2), u)
            xn = np.concatenate([x[nq:], osum(osum(Z(nq), Dx, x), Du, u)])
            if t + 1 < T and (t + 1) % seg_len == 0:
                xn = xn + np.asarray(defects[(t + 1) // seg_len - 1, b], dtype=np.float64)
                dxn[(t + 1) // seg_len - 1, b] = xn
            a1 = a1 + (dot(lin_q[t, b], x) + dot(lin_r[t, b], u))
            a2 = a2 + (0.5 * dot(x, qx) + 0.5 * dot(u, ru))
            du[t, b], x = u, xn
        dJ[b] = a1 + dot(lin_q[T, b], x), a2 + 0.5 * dot(x, osum(Z(n), Qf, x))
    return dxn, du, dJ


def model_terms_ld(D, b, nq, nu, K, k, Q, R, Qf, lin_q, lin_r, defects, seg_len):
    """(dJ1, dJ2) of robot b in longdouble from `forward_linear`'s dx, du, whichever order NumPy takes."""
    T = D.shape[0]
    du, dx = forward_linear(D, b, nq, nu, K, k, defects, seg_len)
    Qs, Rs = plc._stack(Q, Qf, T, LD), plc._steps(R, T, LD)
    d1 = (np.asarray(lin_q[:, b], dtype=LD) * dx).sum() + (np.asarray(lin_r[:, b], dtype=LD) * du).sum()
    d2 = LD(0.5) * (np.einsum("ti,tij,tj->", dx, Qs, dx) + np.einsum("ti,tij,tj->", du, Rs, du))
    return d1, d2, du, dx


# ---- the line search's rules (csrc/plant_shooting.h: ACCEPTANCE) ------------------------------------------------------------------------------
def acceptable(converged, phi, phi_nom, armijo, alpha, dJ1, dJ2, weight, D_nom):
    with np.errstate(all="ignore"):
        return bool(converged) and bool(np.isfinite(phi)) and bool(phi <= phi_nom + armijo * (alpha * (dJ1 - weight * D_nom) + (alpha * alpha) * dJ2))


def linesearch_rules(alphas, weight, conv, J, D, phi_nom, D_nom, dJ, armijo):
    """(phi (n_alpha, B), ok (n_alpha, B), choice (B,)) of candidates with costs J, defect sums D and convergence conv (n_alpha, B) each."""
    na, B = J.shape
    weight = np.broadcast_to(np.asarray(weight, dtype=np.float64), (B,))
    phi = np.asarray(J, dtype=np.float64) + weight[None, :] * np.asarray(D, dtype=np.float64)
    ok = np.array([[acceptable(conv[c, b], phi[c, b], phi_nom[b], armijo, np.float64(alphas[c]), dJ[b, 0], dJ[b, 1], weight[b], D_nom[b]) for b in range(B)]
                   for c in range(na)])
    return phi, ok, np.array([plc.choose(phi[:, b], ok[:, b]) for b in range(B)])
