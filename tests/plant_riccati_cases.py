"""Restatements shared by the LQ-backward-pass tests (tests/test_plant_riccati.py without a device, tests/test_gpu_plant_riccati.py on it,
scripts/plant_riccati_ab.py): the definition of DESIGN.md section 3, item 3e (csrc/plant_riccati.h).  Per robot, with x_t = [q[t]; q[t+1]]
(n = 2nq), u_t (m = nu) and the tape block D_t:  A_t = [0 I; D1 D2], B_t = [0; Du], D1 = D_t[:nq, :nq], D2 = D_t[:nq, nq:2nq],
Du = D_t[:nq, 2nq:2nq+nu];  P = Q_f, p = q_T and for the walk steps s = 1 .. laps T, t = (laps T - s) mod T:

    Qu = r_t + B'p    Quu = R_t + B'PB    Qux = B'PA    G = Quu + ρ I    K_t = G⁻¹ Qux    k_t = -(G⁻¹ Qu)
    dV1 += k_t'Qu     dV2 += ½ k_t'Quu k_t      Acl = A - B K_t
    p <- q_t - K_t'r_t - K_t'(R_t k_t) + Acl'(P (B k_t) + p)          P <- Q_t + K_t'R_t K_t + Acl'P Acl      (not symmetrized)

three times:
  `lq_ld`   in longdouble on the DENSE A_t, B_t, with `gains_ref.solve_ld` and `gains_ref.mm_ld`: nothing of the block structure;
  `lq_np`   the same dense recursion in plain float64 NumPy (`@`, `numpy.linalg.solve`);
  `lq_f64`  in float64 in the ORDER csrc/plant_riccati.h states: products over the nonzero blocks alone, every element one running sum in
            ascending index that starts from the identity block's entry where it has one and from 0.0 otherwise, each term one rounded
            product and one rounded sum; the elimination of tvlqr_kernel (l = a_ik (1 / a_kk)); a zero or non-finite pivot or a non-finite
            K, k, P, p ends the robot's chain with status = the walk step and zero outputs.
Blocks are `StepGradients.dz`: D (T, B, nr, n_cols) row-major.  Q (n, n) or (T, n, n), R (m, m) or (T, m, m), Qf (n, n), q (T+1, B, n),
r (T, B, m).  Each returns a dict: K (keep, B, m, n), k (keep, B, m), P0 (B, n, n), p0 (B, n), dV (B, 2) (k, p0, dV None without q, r),
status (B,), n_cut (B,)."""
import numpy as np

import gains_ref as gr
import plant_adjoint_cases as pac

LD = np.longdouble
FACTOR = pac.FACTOR
OUTPUTS = ("K", "k", "P0", "p0", "dV")


def dense_AB(Dt, nq, nu, dtype=np.float64):
    """A_t (2nq, 2nq), B_t (2nq, nu) of one block Dt (nr, n_cols)."""
    n = 2 * nq
    Dt = np.asarray(Dt, dtype=dtype)
    A = np.zeros((n, n), dtype=dtype)
    A[:nq, nq:] = np.eye(nq, dtype=dtype)
    A[nq:, :] = Dt[:nq, :n]
    Bm = np.zeros((n, nu), dtype=dtype)
    Bm[nq:, :] = Dt[:nq, n:n + nu]
    return A, Bm


def _at(M, t, nd):
    return M if M.ndim == nd else M[t]


def _empty(T, B, n, m, keep, lin, dtype):
    out = dict(K=np.zeros((keep, B, m, n), dtype=dtype), P0=np.zeros((B, n, n), dtype=dtype), k=None, p0=None, dV=None,
               status=np.zeros(B, dtype=np.int32), n_cut=np.zeros(B, dtype=np.int32))
    if lin:
        out.update(k=np.zeros((keep, B, m), dtype=dtype), p0=np.zeros((B, n), dtype=dtype), dV=np.zeros((B, 2), dtype=dtype))
    return out


def _fail(out, b, s):
    out["status"][b] = s
    for key in OUTPUTS:
        if out[key] is not None:
            if key in ("K", "k"):
                out[key][:, b] = 0
            else:
                out[key][b] = 0


def _dense(D, status, nq, nu, Q, R, Qf, q, r, rho, laps, keep, dtype, mm, solve):
    T, B = D.shape[:2]
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    lin = q is not None
    assert lin == (r is not None) and (laps == 1 or not lin)
    Q, R, Qf = (np.asarray(M, dtype=dtype) for M in (Q, R, Qf))
    out = _empty(T, B, n, m, keep, lin, dtype)
    out["n_cut"][:] = (np.asarray(status) == 0).sum(axis=0)
    half, rho_ = dtype(0.5), dtype(rho)
    for b in range(B):
        P = Qf.copy()
        p = np.asarray(q[T, b], dtype=dtype) if lin else None
        dV = np.zeros(2, dtype=dtype)
        steps = laps * T
        for s in range(1, steps + 1):
            t = (steps - s) % T
            A, Bm = dense_AB(D[t, b], nq, nu, dtype)
            Qt, Rt = _at(Q, t, 2), _at(R, t, 2)
            BtP = mm(Bm.T, P)
            Quu = Rt + mm(BtP, Bm)
            rhs = mm(BtP, A)
            if lin:
                rt = np.asarray(r[t, b], dtype=dtype)
                Qu = rt + mm(Bm.T, p)
                rhs = np.concatenate([rhs, Qu[:, None]], axis=1)
            try:
                with np.errstate(all="ignore"):
                    X = solve(Quu + rho_ * np.eye(m, dtype=dtype), rhs)
            except np.linalg.LinAlgError:
                X = np.full_like(rhs, np.nan)
            K = X[:, :n]
            Acl = A - mm(Bm, K)
            Pn = Qt + mm(K.T, mm(Rt, K)) + mm(Acl.T, mm(P, Acl))
            ok = np.isfinite(K.astype(np.float64)).all() and np.isfinite(Pn.astype(np.float64)).all()
            if lin:
                kv = -X[:, n]
                dV[0] += mm(kv, Qu)
                dV[1] += half * mm(kv, mm(Quu, kv))
                pn = np.asarray(q[t, b], dtype=dtype) - mm(K.T, rt) - mm(K.T, mm(Rt, kv)) + mm(Acl.T, mm(P, mm(Bm, kv)) + p)
                ok = ok and np.isfinite(kv.astype(np.float64)).all() and np.isfinite(pn.astype(np.float64)).all()
                p = pn
            if not ok:
                _fail(out, b, s)
                break
            P = Pn
            if s > steps - T and t < keep:
                out["K"][t, b] = K
                if lin:
                    out["k"][t, b] = kv
        else:
            out["P0"][b] = P
            if lin:
                out["p0"][b], out["dV"][b] = p, dV
    return out


def lq_ld(D, status, nq, nu, Q, R, Qf, q=None, r=None, rho=0.0, laps=1, keep=None):
    return _dense(D, status, nq, nu, Q, R, Qf, q, r, rho, laps, keep, LD, gr.mm_ld, gr.solve_ld)


def lq_np(D, status, nq, nu, Q, R, Qf, q=None, r=None, rho=0.0, laps=1, keep=None):
    return _dense(D, status, nq, nu, Q, R, Qf, q, r, rho, laps, keep, np.float64, lambda X, Y: X @ Y, np.linalg.solve)


# ---- the float64 chain in the order of csrc/plant_riccati.h ---------------------------------------------------------------------------------
def _osum(init, X, Y):
    """C = init + Σ_k X[:, k] Y[k, :], ascending k, every term one rounded product and one rounded sum (NumPy's elementwise operations run
    over the outputs, the loop over the terms).  Y a vector: C a vector."""
    C = np.array(init, dtype=np.float64)
    for k in range(X.shape[1]):
        C = C + (X[:, k] * Y[k] if Y.ndim == 1 else X[:, k, None] * Y[None, k, :])
    return C


def _solve_kernel_order(G, F):
    """G \\ F as the chain eliminates: the first largest |entry| of the column, l = a_ik (1 / a_kk), a_ij -= l a_kj, then
    x_k = (f_k - Σ_{j > k} u_kj x_j) / u_kk with ascending j.  None: a zero or non-finite pivot."""
    G, F = G.copy(), F.copy()
    m = len(G)
    for k in range(m):
        col = np.abs(G[k:, k])
        p = k + (int(np.argmax(np.isnan(col))) if np.isnan(col).any() else int(np.argmax(col)))
        if p != k:
            G[[k, p]] = G[[p, k]]
            F[[k, p]] = F[[p, k]]
        pv = G[k, k]
        if not (abs(pv) > 0.0 and np.isfinite(pv)):
            return None
        l = G[k + 1:, k] * (1.0 / pv)
        G[k + 1:, k + 1:] = G[k + 1:, k + 1:] - l[:, None] * G[k, k + 1:][None, :]
        F[k + 1:] = F[k + 1:] - l[:, None] * F[k][None, :]
    for k in range(m - 1, -1, -1):
        a = F[k].copy()
        for j in range(k + 1, m):
            a = a - G[k, j] * F[j]
        F[k] = a / G[k, k]
    return F


def lq_f64(D, status, nq, nu, Q, R, Qf, q=None, r=None, rho=0.0, laps=1, keep=None):
    T, B = D.shape[:2]
    n, m = 2 * nq, nu
    keep = T if keep is None else keep
    lin = q is not None
    assert lin == (r is not None) and (laps == 1 or not lin)
    Q, R, Qf = (np.asarray(M, dtype=np.float64) for M in (Q, R, Qf))
    out = _empty(T, B, n, m, keep, lin, np.float64)
    out["n_cut"][:] = (np.asarray(status) == 0).sum(axis=0)
    Z = np.zeros
    with np.errstate(all="ignore"):
        for b in range(B):
            P = Qf.copy()
            p = np.array(q[T, b], dtype=np.float64) if lin else None
            dV1 = dV2 = 0.0
            steps = laps * T
            fail = 0
            for s in range(1, steps + 1):
                t = (steps - s) % T
                Dx, Du = np.asarray(D[t, b, :nq, :n], dtype=np.float64), np.asarray(D[t, b, :nq, n:n + m], dtype=np.float64)
                Qt, Rt = _at(Q, t, 2), _at(R, t, 2)
                BtP = _osum(Z((m, n)), Du.T, P[nq:, :])                                                  # Du'[P21 P22]
                V = _osum(np.concatenate([Z((m, m + nq)), BtP[:, :nq]], axis=1), BtP[:, nq:], np.concatenate([Du, Dx], axis=1))
                Quu = Rt + V[:, :m]
                G = Quu.copy()
                G[np.arange(m), np.arange(m)] = np.diag(Quu) + rho
                F = V[:, m:]
                if lin:
                    rt = np.asarray(r[t, b], dtype=np.float64)
                    Qu = rt + _osum(Z(m), Du.T, p[nq:])
                    F = np.concatenate([F, Qu[:, None]], axis=1)
                X = _solve_kernel_order(G, F)
                if X is None:
                    fail = s
                    break
                K = X[:, :n]
                ok = np.isfinite(X).all()
                Dcl = Dx - _osum(Z((nq, n)), Du, K)
                RK = _osum(Z((m, n)), Rt, K)
                T1 = _osum(np.concatenate([Z((n, nq)), P[:, :nq]], axis=1), P[:, nq:], Dcl)              # [0 P11; 0 P21] + [P12; P22] Dcl
                Pn = (Qt + _osum(Z((n, n)), K.T, RK)) + _osum(np.concatenate([Z((nq, n)), T1[:nq]], axis=0), Dcl.T, T1[nq:])
                ok = ok and np.isfinite(Pn).all()
                if lin:
                    kv = -X[:, n]
                    dV1 = dV1 + float(_osum(Z(1), kv[None, :], Qu)[0])
                    dV2 = dV2 + 0.5 * float(_osum(Z(1), kv[None, :], _osum(Z(m), Quu, kv))[0])
                    Duk, Rk = _osum(Z(nq), Du, kv), _osum(Z(m), Rt, kv)
                    sv = _osum(Z(n), P[:, nq:], Duk) + p
                    pn = ((np.asarray(q[t, b], dtype=np.float64) - _osum(Z(n), K.T, rt)) - _osum(Z(n), K.T, Rk)) + \
                        _osum(np.concatenate([Z(nq), sv[:nq]]), Dcl.T, sv[nq:])
                    ok = ok and np.isfinite(pn).all()
                    p = pn
                if not ok:
                    fail = s
                    break
                P = Pn
                if s > steps - T and t < keep:
                    out["K"][t, b] = K
                    if lin:
                        out["k"][t, b] = kv
            if fail:
                _fail(out, b, fail)
            else:
                out["P0"][b] = P
                if lin:
                    out["p0"][b], out["dV"][b] = p, (dV1, dV2)
    return out


def bounds(D, status, nq, nu, Q, R, Qf, q=None, r=None, rho=0.0, laps=1, keep=None):
    """(lq_ld, lq_f64, {output: 100 x max(d(lq_np, lq_ld), 2.2e-16)}): the bound of every output, relative to that output's max|lq_ld|,
    built from the restatements alone."""
    ld, f64, plain = (fn(D, status, nq, nu, Q, R, Qf, q, r, rho, laps, keep) for fn in (lq_ld, lq_f64, lq_np))
    return ld, f64, {k: FACTOR * max(pac.distance(plain[k], ld[k]), 2.2e-16) for k in OUTPUTS if ld[k] is not None}


def weights(rng, n, m, T=None, per_step=False):
    """Random symmetric positive definite Q (n, n) or (T, n, n), R alike, and Qf."""
    def spd(k, scale):
        M = rng.standard_normal((k, k))
        return scale * (M @ M.T / k + np.eye(k))
    if per_step:
        return np.stack([spd(n, 1.0) for _ in range(T)]), np.stack([spd(m, 0.1) for _ in range(T)]), spd(n, 2.0)
    return spd(n, 1.0), spd(m, 0.1), spd(n, 2.0)


def closed_loop_product(D, K, nq, nu, b, dtype=LD):
    """Π_t (A_t - B_t K_t), t = T-1 .. 0 from the left, of robot b in longdouble: what `transition()` of the tape rolled out under K gives."""
    n = 2 * nq
    Phi = np.eye(n, dtype=dtype)
    for t in range(D.shape[0]):
        A, Bm = dense_AB(D[t, b], nq, nu, dtype)
        Phi = gr.mm_ld(A - gr.mm_ld(Bm, np.asarray(K[t, b], dtype=dtype)), Phi)
    return Phi
