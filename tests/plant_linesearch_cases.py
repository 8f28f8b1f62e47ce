"""Restatements shared by the line-search tests (tests/test_plant_linesearch.py without a device, tests/test_gpu_plant_linesearch.py on it,
scripts/plant_linesearch_ab.py): the definition of DESIGN.md section 3, item 3f (csrc/plant_cost.h).

The tracking cost of trajectories q (T + 2, B, nq) with applied controls u (T, B, nu), x_t = [q[t]; q[t+1]]:

    ex = x_t - x_goal_t   qx_t = Q_t ex   eu = u_t - u_goal_t   ru_t = R_t eu   l_t = 0.5 (ex'qx_t) + 0.5 (eu'ru_t)   l_T = 0.5 ex'(Qf ex)
    J = ((l_0 + l_1) + ...) + l_T,   lin_q[t] = qx_t,   lin_r[t] = ru_t

three times: `cost_f64` in float64 in the ORDER the header states (every sum ascending from 0.0, one rounded product and one rounded sum per
term); `cost_np` in plain float64 NumPy (einsum); `cost_ld` in longdouble, with the analytic gradient 0.5 (Q + Q') ex, 0.5 (R + R') eu.
Q (n, n) or (T, n, n), R (m, m) or (T, m, m), Qf (n, n), x_goal (T + 1, 1 or B, n), u_goal (T, 1 or B, m).

The rules: `acceptable`, `choose` and `candidate_controls` restate plant_candidate_acceptable, plant_linesearch_choice and
plant_candidate_control.  `ilqr_cpu` is the loop of `plant.ilqr` on the CPU plant of tests/plant_gradient_cases.py (`cpu_step_z`, the blocks of
`rollout_references`, `plant_riccati_cases.lq_f64`), and `lq_optimum_ld` the longdouble KKT solve of the LQ problem a backward pass solves.
"""
import functools

import numpy as np

import gains_ref as gr
import plant_adjoint_cases as pac
import plant_gradient_cases as pgc
import plant_riccati_cases as prc

LD = np.longdouble
FACTOR = pac.FACTOR


def _steps(M, T, dtype):
    """(T, k, k) from one block or T of them."""
    M = np.asarray(M, dtype=dtype)
    return np.broadcast_to(M, (T,) + M.shape[-2:]) if M.ndim == 2 else M


def _stack(Q, Qf, T, dtype):
    return np.concatenate([_steps(Q, T, dtype), np.asarray(Qf, dtype=dtype)[None]], axis=0)


def _errors(q, u, x_goal, u_goal, dtype):
    q, u = np.asarray(q, dtype=dtype), np.asarray(u, dtype=dtype)
    x = np.concatenate([q[:-1], q[1:]], axis=2)
    return x - np.asarray(x_goal, dtype=dtype), u - np.asarray(u_goal, dtype=dtype)


def cost_f64(q, u, Q, R, Qf, x_goal, u_goal):
    """(J (B,), lin_q (T + 1, B, n), lin_r (T, B, m)) in the header's order."""
    T = u.shape[0]
    ex, eu = _errors(q, u, x_goal, u_goal, np.float64)
    Qs, Rs = _stack(Q, Qf, T, np.float64), _steps(R, T, np.float64)

    def matvec(Ms, e):      # out[t, b, i] = sum_j Ms[t, i, j] e[t, b, j], ascending j from 0.0
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


def cost_np(q, u, Q, R, Qf, x_goal, u_goal, dtype=np.float64):
    """The same in whichever order NumPy takes: (J, lin_q, lin_r, gradient of J in x, gradient of J in u)."""
    T = u.shape[0]
    ex, eu = _errors(q, u, x_goal, u_goal, dtype)
    Qs, Rs = _stack(Q, Qf, T, dtype), _steps(R, T, dtype)
    qx, ru = np.einsum("tij,tbj->tbi", Qs, ex), np.einsum("tij,tbj->tbi", Rs, eu)
    J = dtype(0.5) * (np.einsum("tbi,tbi->b", ex, qx) + np.einsum("tbi,tbi->b", eu, ru))
    gx = dtype(0.5) * (qx + np.einsum("tji,tbj->tbi", Qs, ex))
    gu = dtype(0.5) * (ru + np.einsum("tji,tbj->tbi", Rs, eu))
    return J, qx, ru, gx, gu


def cost_ld(q, u, Q, R, Qf, x_goal, u_goal):
    return cost_np(q, u, Q, R, Qf, x_goal, u_goal, dtype=LD)


def cost_bounds(q, u, Q, R, Qf, x_goal, u_goal):
    """(cost_ld's (J, lin_q, lin_r), cost_f64's, {name: FACTOR x max(d(cost_np, cost_ld), 2.2e-16)}), the bounds relative to max|cost_ld|, as
    `plant_riccati_cases.bounds` builds them."""
    ld, f64, plain = cost_ld(q, u, Q, R, Qf, x_goal, u_goal), cost_f64(q, u, Q, R, Qf, x_goal, u_goal), cost_np(q, u, Q, R, Qf, x_goal, u_goal)
    names = ("J", "lin_q", "lin_r")
    return dict(zip(names, ld)), dict(zip(names, f64)), {k: FACTOR * max(pac.distance(plain[i], ld[i]), 2.2e-16) for i, k in enumerate(names)}


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------
def acceptable(converged, J, J_nom, armijo, alpha, dV1, dV2):
    with np.errstate(all="ignore"):
        return bool(converged) and bool(np.isfinite(J)) and bool(J <= J_nom + armijo * (alpha * dV1 + (alpha * alpha) * dV2))


def choose(J, ok):
    """The acceptable candidate of least J, the lower index on a tie; -1 if none."""
    best = -1
    for c in range(len(J)):
        if ok[c] and (best < 0 or J[c] < J[best]):
            best = c
    return best


def candidate_controls(u_nom, alpha, k):
    return np.asarray(u_nom, dtype=np.float64) + np.float64(alpha) * np.asarray(k, dtype=np.float64)


# ---- the LQ optimum by a KKT solve --------------------------------------------------------------------------------------------------------
def lq_optimum_ld(D, b, nq, nu, Q, R, Qf, lin_q, lin_r):
    """Robot b's minimizer of  Σ_t lin_q[t]'δx_t + ½ δx_t'Q_t δx_t + lin_r[t]'δu_t + ½ δu_t'R_t δu_t  (terminal Qf, lin_q[T]) subject to
    δx_{t+1} = A_t δx_t + B_t δu_t, δx_0 = 0, with A_t, B_t of the blocks D (T, B, nr, n_cols): one dense KKT system in longdouble.
    Returns (δu (T, m), δx (T + 1, n), the optimal value)."""
    T, n, m = D.shape[0], 2 * nq, nu
    Qs, Rs = _stack(Q, Qf, T, LD), _steps(R, T, LD)
    nx, nuu = T * n, T * m                      # δx_1 .. δx_T, δu_0 .. δu_{T-1}
    N = nx + nuu
    H, g, E = np.zeros((N, N), dtype=LD), np.zeros(N, dtype=LD), np.zeros((nx, N), dtype=LD)
    for t in range(1, T + 1):
        s = slice((t - 1) * n, t * n)
        H[s, s] = LD(0.5) * (Qs[t] + Qs[t].T)
        g[s] = np.asarray(lin_q[t, b], dtype=LD)
    for t in range(T):
        s = slice(nx + t * m, nx + (t + 1) * m)
        H[s, s] = LD(0.5) * (Rs[t] + Rs[t].T)
        g[s] = np.asarray(lin_r[t, b], dtype=LD)
        A, Bm = prc.dense_AB(D[t, b], nq, nu, LD)
        E[t * n:(t + 1) * n, t * n:(t + 1) * n] = np.eye(n, dtype=LD)      # δx_{t+1} - A_t δx_t - B_t δu_t = 0
        if t > 0:
            E[t * n:(t + 1) * n, (t - 1) * n:t * n] = -A
        E[t * n:(t + 1) * n, s] = -Bm
    KKT = np.block([[H, E.T], [E, np.zeros((nx, nx), dtype=LD)]])
    sol = gr.solve_ld(KKT, np.concatenate([-g, np.zeros(nx, dtype=LD)])[:, None])[:, 0]
    y = sol[:N]
    value = g @ y + LD(0.5) * (y @ (H @ y))
    return y[nx:].reshape(T, m), np.concatenate([np.zeros((1, n), dtype=LD), y[:nx].reshape(T, n)]), value


# ---- iLQR on the CPU plant ----------------------------------------------------------------------------------------------------------------
def _cpu_rollout(case, P, u_bar, K=None, x_ref=None):
    """The case's robots stepped on the CPU under u_t = ū_t (+ K_t (x_ref[t] − x_t), the law of plant_feedback.h with n_sample 1.0):
    (q (T + 2, B, nq), u_applied, status, Z, TH)."""
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
            ua[t, b] = u
            st[t, b], Z[t, b], TH[t, b] = pgc.cpu_step_z(P, q[t, b], q[t + 1, b], u, np.zeros(nw), case["mu"][b], h, pl.SIM_OPTS)
            q[t + 2, b] = Z[t, b, :nq]
    return q, ua, st, Z, TH


def ilqr_cpu(case, Q, R, Qf, x_goal, u_goal, alphas, n_iter, rho=0.0, armijo=1e-4):
    """`plant.ilqr` with a constant rho on the CPU plant: a list with one dict per iteration - J_nom, J (n_alpha, B), ok, choice, dV, u_nom, k, D
    (the blocks about the nominal, longdouble solves rounded to float64), lin_q, lin_r, u (the controls after it), q, accepted, J_new."""
    nq, nu = pgc.dims(case["model"])[:2]
    P = pgc.cpu_plant(case)
    B, T = case["q1"].shape[0], case["T"]
    u0 = np.broadcast_to(case["u"], (T, B, nu))
    q, ua, st, Z, TH = _cpu_rollout(case, P, u0)
    J, lq, lr = cost_f64(q, ua, Q, R, Qf, x_goal, u_goal)
    out = []
    for _ in range(n_iter):
        refs = pgc.rollout_references(case, Z, TH, pgc.REG, 2 * nq + nu)
        D = np.array([[np.asarray(refs[t, b]["ld"], dtype=np.float64) for b in range(B)] for t in range(T)])
        g = prc.lq_f64(D, st.astype(np.int32), nq, nu, Q, R, Qf, q=lq, r=lr, rho=rho)
        x_ref = np.concatenate([q[1:T + 1] - 1.0 * (q[1:T + 1] - q[:T]), q[1:T + 1]], axis=2)
        cands = [_cpu_rollout(case, P, candidate_controls(ua, a, g["k"]), g["K"], x_ref) for a in alphas]
        Jc = np.array([cost_f64(c[0], c[1], Q, R, Qf, x_goal, u_goal)[0] for c in cands])
        ok = np.array([[acceptable(cands[c][2][:, b].all(), Jc[c, b], J[b], armijo, alphas[c], g["dV"][b, 0], g["dV"][b, 1]) for b in range(B)]
                       for c in range(len(alphas))])
        choice = np.array([choose(Jc[:, b], ok[:, b]) for b in range(B)])
        it = dict(J_nom=J.copy(), J=Jc, ok=ok, choice=choice, dV=g["dV"], u_nom=ua.copy(), k=g["k"], D=D, lin_q=lq, lin_r=lr, accepted=choice >= 0)
        nq_, nua, nst, nZ, nTH = (np.array(a) for a in (q, ua, st, Z, TH))
        for b in range(B):
            if choice[b] >= 0:
                cq, cu, cs, cZ, cT = cands[choice[b]]
                nq_[:, b], nua[:, b], nst[:, b], nZ[:, b], nTH[:, b] = cq[:, b], cu[:, b], cs[:, b], cZ[:, b], cT[:, b]
        q, ua, st, Z, TH = nq_, nua, nst, nZ, nTH
        J, lq, lr = cost_f64(q, ua, Q, R, Qf, x_goal, u_goal)
        it.update(u=ua.copy(), q=q.copy(), J_new=J.copy())
        out.append(it)
    return out


# ---- the two iLQR cases of the GPU tests ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flight_case():
    """Two particles released 1 m above flat ground, T = 8: they never touch it, so the plant is linear up to the interior point's
    κ-smoothing, and one full iLQR step lands on the LQ optimum.  (case, Q, R, Qf, x_goal, u_goal)."""
    T, B, h = 8, 2, 0.01
    case = dict(model="particle", terrain="flat_3D_lc", q1=np.array([[0.0, 0.0, 1.0], [0.1, -0.2, 1.0]]), v1=np.array([[0.2, 0.0, 0.0], [0.0, 0.1, 0.3]]),
                u=np.zeros((T, B, 3)), mu=np.array([0.5, 0.5]), h=h, T=T)
    rng = np.random.default_rng(5)
    Q, R, Qf = prc.weights(rng, 6, 3)
    goal = np.array([0.05, -0.05, 1.02])
    x_goal = np.broadcast_to(np.concatenate([goal, goal]), (T + 1, 1, 6)).copy()
    return case, Q, 0.01 * R, Qf, x_goal, np.zeros((T, 1, 3))


@functools.lru_cache(maxsize=None)
def flight_gaps_cpu():
    """One full step (alpha 1, rho 0) of `ilqr_cpu` on the flight case against the longdouble LQ optimum on the nominal's own blocks:
    (max|u_new − (u_nom + δu*)| / max|δu*| over the robots, max|(J_new − J_nom) − (dV1 + dV2)| / |dV1 + dV2|)."""
    case, Q, R, Qf, x_goal, u_goal = flight_case()
    it = ilqr_cpu(case, Q, R, Qf, x_goal, u_goal, (1.0,), 1)[0]
    return flight_gaps(it["D"], it["u_nom"], it["u"], it["lin_q"], it["lin_r"], it["J_nom"], it["J_new"], it["dV"], Q, R, Qf)


def flight_gaps(D, u_nom, u_new, lin_q, lin_r, J_nom, J_new, dV, Q, R, Qf):
    nq, nu = 3, 3
    gu = gj = 0.0
    for b in range(u_nom.shape[1]):
        du, _, _ = lq_optimum_ld(D, b, nq, nu, Q, R, Qf, lin_q, lin_r)
        gu = max(gu, float(np.abs(np.asarray(u_new[:, b], dtype=LD) - (np.asarray(u_nom[:, b], dtype=LD) + du)).max() / np.abs(du).max()))
        pred = LD(dV[b, 0]) + LD(dV[b, 1])
        gj = max(gj, float(abs((LD(J_new[b]) - LD(J_nom[b])) - pred) / abs(pred)))
    return gu, gj


@functools.lru_cache(maxsize=None)
def contact_cost():
    """The cost of the through-contact test on the hopper_2D rollout case: hold the body where it starts, 5 cm further along, with a cheap
    control.  (Q, R, Qf, x_goal, u_goal)."""
    c = pgc.rollout_case("hopper_2D")
    T = c["T"]
    goal = c["q1"][0] + np.array([0.05, 0.0, 0.0, 0.0])
    Q = np.diag(np.tile([1.0, 1.0, 1.0, 1.0], 2))
    return Q, 1e-2 * np.eye(2), 10.0 * Q, np.broadcast_to(np.concatenate([goal, goal]), (T + 1, 1, 8)).copy(), np.zeros((T, 1, 2))
