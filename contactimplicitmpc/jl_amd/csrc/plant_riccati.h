// The LQ backward pass over a rollout's tape (DESIGN.md sections 3, item 3e, and 5.5): time-varying LQR gains, and with linear cost
// terms the feedforward, along the trajectory the robots took.  Per robot, with the state x_t = [q[t]; q[t+1]] (n = 2nq) and the
// control u_t (m = nu), the step matrices come from the tape block D_t (nr x n_cols, column-major), D = D_t[0:nq, 0:2nq] = [D1 D2],
// Du = D_t[0:nq, 2nq:2nq+nu]:
//
//   A_t = [0 I; D1 D2]      B_t = [0; Du]            (a step with gradient status 0 has D_t = 0: A_t = [0 I; 0 0], B_t = 0; the chain
//                                                     walks through it and n_cut counts it, as plant_adjoint.h does)
//   P = Q_f, p = q_T; for the walk steps s = 1 .. laps T, t = (laps T - s) mod T:
//     Qu  = r_t + B'p         Quu = R_t + B'PB         Qux = B'PA         G = Quu + rho I
//     K_t = G^-1 Qux          k_t = -(G^-1 Qu)         (LU with partial pivoting, the first largest |entry|, as tvlqr_kernel)
//     dV1 += k_t'Qu           dV2 += 0.5 (k_t'(Quu k_t))
//     Acl = A - B K_t = [0 I; Dcl],  Dcl = D - Du K_t
//     p <- ((q_t - K_t'r_t) - K_t'(R_t k_t)) + Acl'(P (B k_t) + p)
//     P <- (Q_t + K_t'(R_t K_t)) + Acl'(P Acl)          (not symmetrized, as gains.jl:10-11 and tvlqr_kernel)
//   K_t, k_t of the last lap with t < n_keep are kept; P0, p0 are P, p after the last step.  Without q, r: no Qu, k, dV, p.
//
// THE ORDERING RULE.  Every product runs over the nonzero structure alone; with P in nq x nq blocks [P11 P12; P21 P22] and
// T1 = P Acl in blocks alike, the block products that exist are
//     B'P    = Du'[P21 P22]                                                     (m x n, depth nq)
//     B'PB   = (B'P)[:, nq:] Du         B'PA = [0 (B'P)[:, :nq]] + (B'P)[:, nq:] D     (depth nq)
//     P Acl  = [0 P11; 0 P21] + [P12; P22] Dcl                                  (n x n, depth nq)
//     Acl'T1 = [0 0; T1_11 T1_12] + Dcl'[T1_21 T1_22]                           (n x n, depth nq)
//     B'p = Du'p[nq:],  B k = [0; Du k],  P (B k) = [P12; P22] (Du k),  Acl's = [0; s[:nq]] + Dcl's[nq:]
// and K'(R K), R K, Du K, K'r, K'(R k), R k, Quu k, k'Qu run over m.  Every output element is ONE running sum in ascending index:
// it starts from the identity block's entry where the element has one (the entry of the other factor that the 1 selects: it is the
// first nonzero term of the dense chain), from 0.0 otherwise, and each further term is one rounded product and one rounded sum,
// contraction off.  For finite inputs that is the dense chain k = 0 .. n-1 with its exact zero terms left out, at half the work.
// Sums of several parts are taken left to right as bracketed above; the elimination is tvlqr_kernel's (l = a_ik (1 / a_kk),
// a_ij -= l a_kj; back-substitution s -= u_kj x_j ascending j, then s / u_kk).  The chain does not depend on the team, the batch, or
// which robots ride along.
//
// THE DEFECT HOOK (multiple shooting; plant_shooting.h): with defects d_j (j = 1 .. M-1, 2nq numbers each) at
// the nodes t = j seg_len, the dynamics about the segments' trajectories are dx_{t+1} = A dx_t + B du_t + d_{t+1} at a node, and the affine
// term moves the value's linear term: at the top of the walk step of t, if t + 1 is a node,  p <- p + P d.  P d has no zero structure:
// (P d)[c] = sum_k P[c, k] d[k] is ONE running sum over k = 0 .. n-1 ascending from 0.0, one rounded product and one rounded sum per term,
// and p[c] + (P d)[c] one more rounded sum.  The hook is compiled into the SHOOT chain alone; every other instantiation keeps its
// statements, and with them its instructions.
//
// A zero or non-finite pivot, or a non-finite K, k, P or p, ends the robot's chain: status[b] = the 1-based walk step s, and the
// robot's outputs are zeros.  Other robots are unaffected.
//
// The chain of one robot is stated here ONCE for a team of workers, like plant_adjoint.h and plant_tangent.h: plant_riccati_kernel
// (plant_riccati.hip) runs it with a workgroup of four wavefronts, a host program (tests/native/plant_riccati_check.cpp) with a team
// of one, statement for statement.  Team: rank(), size(), sync(), and the two-phase fetch of a block's corner:
// fetch_issue(src, rows, cols, ld) starts reading the rows x cols corner of a column-major block with leading dimension ld,
// fetch_commit(dst, src, rows, cols, ld) leaves it packed (leading dimension rows) in dst.  Only the nq x (2nq + nu) corner of D_t is
// read, and it is double-buffered against the next step's.
#pragma once
#include <cmath>
#include <cstddef>

#include "plant_boxqp.h"

// no contraction in this header's arithmetic: a * b + c rounds twice
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define PRIC_HD __host__ __device__
#else
#define PRIC_HD
#endif
#ifdef __clang__
#define PRIC_UNROLL _Pragma("unroll")
#define PRIC_UNROLL2 _Pragma("unroll 2")
#else
#define PRIC_UNROLL
#define PRIC_UNROLL2
#endif

namespace cimpc {

// Every pointer in the memory the team reads (device memory for the kernel).  dz: T x B x (nr x n_cols) column-major, status T x B.
// Q: n_Q x (n x n), R: n_R x (m x m), column-major, shared by the robots, one (n_Q, n_R = 1) or one per step; Qf n x n.
// q: (T+1) x B x n (q[T] = q_T), r: T x B x m: both or neither.  Out: K n_keep x B x (m x n column-major);
// k n_keep x B x m, P0 B x (n x n), p0 B x n, dV B x 2: null = not asked for (k, p0, dV need q, r); status B, n_cut B.
struct PlantRiccati {
    const double* dz;
    const int* tape_status;
    const double *Q, *Qf, *R, *q, *r;
    double *K, *k, *P0, *p0, *dV;
    int *status, *n_cut;
    int B, T, nq, nu, nr, n_cols, laps, n_Q, n_R, n_keep;
    double rho;
    // the limited pass (plant_boxqp.h), read by the BOX chain alone: u_lo, u_hi n_lim x m (n_lim 1 or B; null:
    // no limits), u_nom T x B x m the tape's applied controls, rho_b n_rho (1 or B) regularizations (null: rho), clamped n_keep x B
    const double *u_lo = nullptr, *u_hi = nullptr, *u_nom = nullptr, *rho_b = nullptr;
    int* clamped = nullptr;
    int n_lim = 1, n_rho = 1;
    // the defect hook, read by the SHOOT chain alone: defects (T / seg_len - 1) x B x n, the defect of node j = 1 .. at step j seg_len
    const double* defects = nullptr;
    int seg_len = 0;
};

// ---- the plan: what a robot's chain needs of the team's shared memory ---------------------------------------------------------------
//   P, T1 (n x n each); the corner in use and the one in flight (nq x (n + m) each); Dcl and its transpose (nq x n each); Du'
//   (m x nq); B'P, K', R K (m x n each); F = [Qux | Qu] then [K | G^-1 Qu] (m x (n + 1)); G, R (m x m each);
//   vectors: p, s (n each), Qu, k, R k (m each), Du k (nq), dV (2), the flag of a non-finite entry (1) and one of padding
PRIC_HD constexpr size_t plant_riccati_work_doubles(int nq, int nu) {
    const size_t n = (size_t)2 * nq, m = (size_t)nu, h = (size_t)nq;
    return 2 * n * n + 2 * h * (n + m) + 2 * h * n + m * h + 3 * m * n + m * (n + 1) + 2 * m * m + 2 * n + 3 * m + h + 4;
}
constexpr size_t PLANT_RIC_MAX_LDS = 160 * 1024;      // of a gfx950 CU
constexpr size_t plant_riccati_lds(int nq, int nu) { return plant_riccati_work_doubles(nq, nu) * sizeof(double); }
constexpr bool plant_riccati_fits(int nq, int nu) { return nq >= 1 && nu >= 1 && plant_riccati_lds(nq, nu) <= PLANT_RIC_MAX_LDS; }
static_assert(plant_riccati_lds(18, 12) == 63920, "centroidal_quadruped_wall (n = 36, m = 12), the largest: 62 KB, two workgroups a CU");
static_assert(plant_riccati_lds(11, 8) == 24984, "quadruped (n = 22, m = 8): 24 KB");
// the limited chain: plant_boxqp.h's work behind the unlimited chain's
PRIC_HD constexpr size_t plant_riccati_box_work_doubles(int nq, int nu) { return plant_riccati_work_doubles(nq, nu) + plant_boxqp_work_doubles(nu); }
constexpr size_t plant_riccati_box_lds(int nq, int nu) { return plant_riccati_box_work_doubles(nq, nu) * sizeof(double); }
static_assert(plant_riccati_box_lds(18, 12) == 65760 && 2 * plant_riccati_box_lds(18, 12) <= PLANT_RIC_MAX_LDS,
              "the largest model with limits: 64 KB, still two workgroups a CU");
static_assert(plant_riccati_box_lds(11, 8) == 25960, "quadruped with limits: 25 KB");
// the chain with the defect hook: the limited chain's work and the node's defect (n) behind it
PRIC_HD constexpr size_t plant_riccati_shoot_work_doubles(int nq, int nu) { return plant_riccati_box_work_doubles(nq, nu) + (size_t)2 * nq; }
constexpr size_t plant_riccati_shoot_lds(int nq, int nu) { return plant_riccati_shoot_work_doubles(nq, nu) * sizeof(double); }
static_assert(plant_riccati_shoot_lds(18, 12) == 66048 && 2 * plant_riccati_shoot_lds(18, 12) <= PLANT_RIC_MAX_LDS,
              "the largest model with limits and defects: 64.5 KB, still two workgroups a CU");
static_assert(plant_riccati_fits(18, 12) && plant_riccati_fits(11, 8) && plant_riccati_fits(1, 1) && !plant_riccati_fits(60, 12), "the plan's limits");

PRIC_HD inline bool plant_riccati_bad_pivot(double pv) { return !(std::fabs(pv) > 0.0) || !std::isfinite(pv); }
// |a| beats |b| in a pivot search: larger, or not a number (which then stays: the pivot test refuses it)
PRIC_HD inline bool plant_riccati_pivot_beats(double a, double b) { return a > b || (a != a && b == b); }

// the team of one: a host caller.  Its copy happens at commit time.
struct PlantRiccatiSolo {
    PRIC_HD int rank() const { return 0; }
    PRIC_HD int size() const { return 1; }
    PRIC_HD void sync() const {}
    PRIC_HD void fetch_issue(const double*, int, int, int) {}
    PRIC_HD void fetch_commit(double* dst, const double* src, int rows, int cols, int ld) {
        for (int c = 0; c < cols; ++c)
            for (int r = 0; r < rows; ++r) dst[c * rows + r] = src[(size_t)c * ld + r];
    }
};

// C(r, c) = init(r, c) + sum_k X(r, k) Y(k, c), k ascending, for a rows x cols result; a TR x TC tile of it per member, as
// tile_product of gains.hip: TR + TC reads feed TR TC multiply-adds and the tile's sums are independent chains.  Every operand is
// stored so that X(r, k) runs over consecutive words with r, i.e. with the lane.  Two calls with equal rows and cols give an element
// to the same member.
template <int TR, int TC, class Team, class FI, class FX, class FY, class FOUT>
PRIC_HD inline void plant_riccati_product(const Team& team, int rows, int cols, int depth, FI init, FX X, FY Y, FOUT out) {
    const int tr = (rows + TR - 1) / TR, tc = (cols + TC - 1) / TC;
    for (int e = team.rank(); e < tr * tc; e += team.size()) {
        const int r0 = (e % tr) * TR, c0 = (e / tr) * TC;
        int ri[TR], ci[TC];
PRIC_UNROLL
        for (int i = 0; i < TR; ++i) ri[i] = r0 + i < rows ? r0 + i : rows - 1;      // a tile over the edge repeats the last row / column and drops it
PRIC_UNROLL
        for (int j = 0; j < TC; ++j) ci[j] = c0 + j < cols ? c0 + j : cols - 1;
        double acc[TR][TC];
PRIC_UNROLL
        for (int i = 0; i < TR; ++i)
PRIC_UNROLL
            for (int j = 0; j < TC; ++j) acc[i][j] = init(ri[i], ci[j]);
PRIC_UNROLL2
        for (int k = 0; k < depth; ++k) {
            double x[TR], y[TC];
PRIC_UNROLL
            for (int i = 0; i < TR; ++i) x[i] = X(ri[i], k);
PRIC_UNROLL
            for (int j = 0; j < TC; ++j) y[j] = Y(k, ci[j]);
PRIC_UNROLL
            for (int i = 0; i < TR; ++i)
PRIC_UNROLL
                for (int j = 0; j < TC; ++j) acc[i][j] += x[i] * y[j];
        }
PRIC_UNROLL
        for (int i = 0; i < TR; ++i)
PRIC_UNROLL
            for (int j = 0; j < TC; ++j)
                if (r0 + i < rows && c0 + j < cols) out(r0 + i, c0 + j, acc[i][j]);
    }
}

// The chain of robot rb.  work: shared by the team, plant_riccati_work_doubles(nq, nu).  LIN: the linear terms are compiled in (the
// caller has L.q and L.r non-null and L.laps == 1).  BOX (with LIN): the limited pass of plant_boxqp.h stands where the unlimited solve
// does, work is plant_riccati_box_work_doubles(nq, nu), rho is the robot's own and clamped is written.  All matrices column-major.
// SHOOT (with BOX): the defect hook is compiled in, L.defects and L.seg_len are read, work is plant_riccati_shoot_work_doubles(nq, nu).
template <bool LIN, bool BOX = false, bool SHOOT = false, class Team>
PRIC_HD inline void plant_riccati_chain_as(const PlantRiccati& L, int rb, double* work, Team& team) {
    const int me = team.rank(), np = team.size();
    const int nq = L.nq, n = 2 * nq, m = L.nu, B = L.B, T = L.T, nr = L.nr, nc = n + m, fw = n + (LIN ? 1 : 0);
    const size_t blk = (size_t)nr * L.n_cols;
    double* P = work;                        // n x n
    double* T1 = P + n * n;                  // n x n: P Acl
    double* Dc[2] = {T1 + n * n, T1 + n * n + nq * nc};      // nq x (n + m): [D1 D2 Du] of the step in use / in flight
    double* Dcl = Dc[1] + nq * nc;           // nq x n: D - Du K
    double* DclT = Dcl + nq * n;             // n x nq: its transpose
    double* DuT = DclT + nq * n;             // m x nq
    double* BtP = DuT + m * nq;              // m x n
    double* KT = BtP + m * n;                // n x m: K'
    double* RK = KT + m * n;                 // m x n
    double* F = RK + m * n;                  // m x (n + 1): [Qux | Qu], then [K | G^-1 Qu]
    double* G = F + m * (n + 1);             // m x m: Quu + rho I, then its LU factors
    double* Rm = G + m * m;                  // m x m
    double* pv_ = Rm + m * m;                // p (n)
    double* sv = pv_ + n;                    // s = P (B k) + p (n)
    double* Qu = sv + n;                     // m
    double* kv = Qu + m;                     // m
    double* Rk = kv + m;                     // m
    double* Duk = Rk + m;                    // nq
    double* dV = Duk + nq;                   // 2
    double* flag = dV + 2;                   // 1: a member met a non-finite entry
    auto block = [&](int t) { return L.dz + ((size_t)t * B + rb) * blk; };
    const auto zero = [](int, int) { return 0.0; };
    const int steps = L.laps * T;
    static_assert(LIN || !BOX, "the limited pass needs the linear terms");
    static_assert(BOX || !SHOOT, "the defect hook stands in the limited chain");
    double rho_box = 0.0;                    // BOX: the robot's own rho
    PlantBoxQPWork box{};
    if constexpr (BOX) {
        rho_box = L.rho_b ? L.rho_b[L.n_rho == 1 ? 0 : rb] : L.rho;
        box = plant_boxqp_carve(work + plant_riccati_work_doubles(nq, m), m);
    }

    for (int e = me; e < n * n; e += np) P[e] = L.Qf[e];
    if constexpr (LIN) {
        for (int e = me; e < n; e += np) pv_[e] = L.q[((size_t)T * B + rb) * n + e];
        if (me == 0) { dV[0] = 0.0; dV[1] = 0.0; }
    }
    if (me == 0) {
        int cut = 0;
        for (int t = 0; t < T; ++t) cut += L.tape_status[(size_t)t * B + rb] == 0 ? 1 : 0;
        L.n_cut[rb] = cut;
        flag[0] = 0.0;
    }
    team.fetch_issue(block(T - 1), nq, nc, nr);
    team.fetch_commit(Dc[0], block(T - 1), nq, nc, nr);
    team.sync();

    int fail = 0;                            // the walk step that ended the chain: the same word for every member
    for (int s = 1; s <= steps && !fail; ++s) {
        const int t = (steps - s) % T, tn = (steps - s - 1 + T) % T;
        const bool last_lap = s > steps - T;
        const double* D = Dc[(s - 1) & 1];   // [D1 D2] nq x n, then Du nq x m
        const double* Du = D + nq * n;
        const double* Qt = L.Q + (L.n_Q == 1 ? 0 : (size_t)t * n * n);
        const double* Rt = L.R + (L.n_R == 1 ? 0 : (size_t)t * m * m);
        const double* qt = LIN ? L.q + ((size_t)t * B + rb) * n : nullptr;
        const double* rt = LIN ? L.r + ((size_t)t * B + rb) * m : nullptr;
        bool finite = true;                  // of the entries of K, k, P and p this member computes
        if (s < steps) team.fetch_issue(block(tn), nq, nc, nr);      // in flight while step t is worked
        if constexpr (SHOOT) {               // t + 1 a node: p <- p + P d, the defect staged behind the box QP's work
            if (t + 1 < T && (t + 1) % L.seg_len == 0) {
                double* dn = work + plant_riccati_box_work_doubles(nq, m);
                const double* d = L.defects + ((size_t)((t + 1) / L.seg_len - 1) * B + rb) * n;
                for (int e = me; e < n; e += np) dn[e] = d[e];
                team.sync();
                for (int c = np - 1 - me; c < n; c += np) {
                    double a = 0.0;
                    for (int k = 0; k < n; ++k) a += P[k * n + c] * dn[k];
                    pv_[c] = pv_[c] + a;
                }
                team.sync();
            }
        }
        for (int e = me; e < nq * m; e += np) DuT[(e % nq) * m + e / nq] = Du[e];
        for (int e = me; e < m * m; e += np) Rm[e] = Rt[e];
        team.sync();
        // B'P = Du'[P21 P22]
        plant_riccati_product<2, 3>(team, m, n, nq, zero, [&](int i, int k) { return DuT[k * m + i]; },
                                    [&](int k, int c) { return P[c * n + nq + k]; }, [&](int i, int c, double v) { BtP[c * m + i] = v; });
        if constexpr (LIN)                   // Qu = r + Du'p[nq:], from the far end of the team
            for (int i = np - 1 - me; i < m; i += np) {
                double a = 0.0;
                for (int k = 0; k < nq; ++k) a += DuT[k * m + i] * pv_[nq + k];
                const double v = rt[i] + a;
                Qu[i] = v;
                F[n * m + i] = v;
            }
        team.sync();
        // G = (R + (B'P)[:, nq:] Du) + rho I | Qux = [0 (B'P)[:, :nq]] + (B'P)[:, nq:] [D1 D2]
        plant_riccati_product<2, 3>(team, m, m + n, nq, [&](int i, int c) { return c >= m + nq ? BtP[(c - m - nq) * m + i] : 0.0; },
                                    [&](int i, int k) { return BtP[(nq + k) * m + i]; },
                                    [&](int k, int c) { return c < m ? Du[c * nq + k] : D[(c - m) * nq + k]; },
                                    [&](int i, int c, double v) {
                                        if (c < m) {
                                            const double quu = Rm[c * m + i] + v;
                                            G[c * m + i] = i == c ? quu + (BOX ? rho_box : L.rho) : quu;
                                            if constexpr (LIN) RK[c * m + i] = quu;      // Quu, kept for dV2 (R K is formed after it)
                                        } else F[(c - m) * m + i] = v;
                                    });
        team.sync();
        if constexpr (BOX) {                 // the box QP and the final solve on its free set: plant_boxqp.h
            const size_t lim = (size_t)(L.n_lim == 1 ? 0 : rb) * m;
            if (!plant_boxqp_step(team, m, n, G, F, Qu, kv, KT, box, L.u_lo ? L.u_lo + lim : nullptr, L.u_lo ? L.u_hi + lim : nullptr,
                                  L.u_lo ? L.u_nom + ((size_t)t * B + rb) * m : nullptr, s == 1, &finite)) { fail = s; break; }
        } else {
            for (int k = 0; k < m; ++k) {        // G [K | x] = [Qux | Qu], LU with partial pivoting; every member finds the pivot
                double best = -1.0;
                int p = k;
                for (int i = k; i < m; ++i) {
                    const double v = std::fabs(G[k * m + i]);
                    if (plant_riccati_pivot_beats(v, best)) { best = v; p = i; }
                }
                team.sync();
                if (p != k)
                    for (int j = k + me; j < m + fw; j += np) {
                        double* col = j < m ? G + j * m : F + (j - m) * m;
                        const double v = col[k]; col[k] = col[p]; col[p] = v;
                    }
                team.sync();
                const double pv = G[k * m + k];
                if (plant_riccati_bad_pivot(pv)) { fail = s; break; }      // the same word for every member: all leave together
                const double rp = 1.0 / pv;
                for (int e = me; e < (m - k - 1) * (m + fw - k - 1); e += np) {      // (i, j), i fastest
                    const int i = k + 1 + e % (m - k - 1), j = k + 1 + e / (m - k - 1);
                    const double l = G[k * m + i] * rp;
                    double* col = j < m ? G + j * m : F + (j - m) * m;
                    col[i] -= l * col[k];
                }
                team.sync();
            }
        }
        if (fail) break;
        if constexpr (!BOX) {
            for (int c = me; c < fw; c += np) {  // U K = F, a column per member
                double* col = F + c * m;
                for (int k = m - 1; k >= 0; --k) {
                    double a = col[k];
                    for (int j = k + 1; j < m; ++j) a -= G[j * m + k] * col[j];
                    a /= G[k * m + k];
                    col[k] = a;
                    finite = finite && std::isfinite(a);
                    if (c < n) KT[k * n + c] = a;
                    else kv[k] = -a;
                }
            }
        }
        team.sync();
        // Dcl = D - Du K (both orientations) and R K; with linear terms dV, Du k and R k, from the far end of the team
        plant_riccati_product<2, 3>(team, nq, n, m, zero, [&](int r, int i) { return Du[i * nq + r]; }, [&](int i, int c) { return F[c * m + i]; },
                                    [&](int r, int c, double v) { const double d = D[c * nq + r] - v; Dcl[c * nq + r] = d; DclT[r * n + c] = d; });
        if constexpr (LIN) {
            for (int w = np - 1 - me; w < 1 + nq + m; w += np) {
                if (w == 0) {                // dV1 += k'Qu, dV2 += 0.5 (k'(Quu k)): Quu sits in RK until the product below
                    double a = 0.0;
                    for (int i = 0; i < m; ++i) a += kv[i] * Qu[i];
                    dV[0] += a;
                    double b = 0.0;
                    for (int i = 0; i < m; ++i) {
                        double y = 0.0;
                        for (int j = 0; j < m; ++j) y += RK[j * m + i] * kv[j];
                        b += kv[i] * y;
                    }
                    dV[1] += 0.5 * b;
                } else if (w <= nq) {        // Du k
                    double a = 0.0;
                    for (int j = 0; j < m; ++j) a += Du[j * nq + (w - 1)] * kv[j];
                    Duk[w - 1] = a;
                } else {                     // R k
                    double a = 0.0;
                    for (int j = 0; j < m; ++j) a += Rm[j * m + (w - 1 - nq)] * kv[j];
                    Rk[w - 1 - nq] = a;
                }
            }
            team.sync();                     // dV has read Quu
        }
        plant_riccati_product<2, 3>(team, m, n, m, zero, [&](int i, int j) { return Rm[j * m + i]; }, [&](int j, int c) { return F[c * m + j]; },
                                    [&](int i, int c, double v) { RK[c * m + i] = v; });
        if (last_lap && t < L.n_keep) {
            for (int e = me; e < m * n; e += np) L.K[((size_t)t * B + rb) * m * n + e] = F[e];
            if constexpr (LIN) if (L.k) for (int e = me; e < m; e += np) L.k[((size_t)t * B + rb) * m + e] = kv[e];
            if constexpr (BOX) if (L.clamped && me == 0) L.clamped[(size_t)t * B + rb] = box.idx[m + 1];
        }
        team.sync();
        // T1 = P Acl = [0 P11; 0 P21] + [P12; P22] Dcl; with linear terms s = [P12; P22] (Du k) + p
        plant_riccati_product<2, 3>(team, n, n, nq, [&](int r, int c) { return c >= nq ? P[(c - nq) * n + r] : 0.0; },
                                    [&](int r, int k) { return P[(nq + k) * n + r]; }, [&](int k, int c) { return Dcl[c * nq + k]; },
                                    [&](int r, int c, double v) { T1[c * n + r] = v; });
        if constexpr (LIN)
            for (int j = np - 1 - me; j < n; j += np) {
                double a = 0.0;
                for (int k = 0; k < nq; ++k) a += P[(nq + k) * n + j] * Duk[k];
                sv[j] = a + pv_[j];
            }
        team.sync();
        // P <- (Q + K'(R K)) + Acl'T1, Acl'T1 = [0 0; T1_11 T1_12] + Dcl'[T1_21 T1_22]: two sums, as tvlqr_kernel; an element stays with its member
        plant_riccati_product<2, 3>(team, n, n, m, zero, [&](int r, int i) { return KT[i * n + r]; }, [&](int i, int c) { return RK[c * m + i]; },
                                    [&](int r, int c, double v) { P[c * n + r] = Qt[c * n + r] + v; });
        plant_riccati_product<2, 3>(team, n, n, nq, [&](int r, int c) { return r >= nq ? T1[c * n + r - nq] : 0.0; },
                                    [&](int r, int k) { return DclT[k * n + r]; }, [&](int k, int c) { return T1[c * n + nq + k]; },
                                    [&](int r, int c, double v) { const double a = P[c * n + r] + v; P[c * n + r] = a; finite = finite && std::isfinite(a); });
        if constexpr (LIN) {
            // p <- ((q - K'r) - K'(R k)) + Acl's, Acl's = [0; s[:nq]] + Dcl's[nq:]; p's readers (s) are done: sync above
            for (int c = np - 1 - me; c < n; c += np) {
                double a = 0.0, b = 0.0;
                for (int i = 0; i < m; ++i) a += KT[i * n + c] * rt[i];
                for (int i = 0; i < m; ++i) b += KT[i * n + c] * Rk[i];
                double d = c >= nq ? sv[c - nq] : 0.0;
                for (int k = 0; k < nq; ++k) d += DclT[k * n + c] * sv[nq + k];
                const double v = ((qt[c] - a) - b) + d;
                pv_[c] = v;
                finite = finite && std::isfinite(v);
            }
        }
        if (!finite) flag[0] = 1.0;
        if (s < steps) team.fetch_commit(Dc[s & 1], block(tn), nq, nc, nr);      // its last reader left it at the end of step s - 1
        team.sync();
        if (flag[0] != 0.0) fail = s;        // the same word for every member
    }

    // the robot's outputs: P0, p0, dV and its status; a chain that ended early leaves zeros everywhere
    if (fail) {
        for (size_t e = me; e < (size_t)L.n_keep * m * n; e += np) L.K[((e / ((size_t)m * n)) * B + rb) * m * n + e % ((size_t)m * n)] = 0.0;
        if (L.k) for (int e = me; e < L.n_keep * m; e += np) L.k[((size_t)(e / m) * B + rb) * m + e % m] = 0.0;
        if constexpr (BOX) if (L.clamped) for (int e = me; e < L.n_keep; e += np) L.clamped[(size_t)e * B + rb] = 0;
    }
    if (L.P0) for (int e = me; e < n * n; e += np) L.P0[(size_t)rb * n * n + e] = fail ? 0.0 : P[e];
    if constexpr (LIN) {
        if (L.p0) for (int e = me; e < n; e += np) L.p0[(size_t)rb * n + e] = fail ? 0.0 : pv_[e];
        if (L.dV) for (int e = me; e < 2; e += np) L.dV[(size_t)rb * 2 + e] = fail ? 0.0 : dV[e];
    }
    if (me == 0) L.status[rb] = fail;
}

// The chain of robot rb, with or without linear terms by what L carries.
template <class Team>
PRIC_HD inline void plant_riccati_chain(const PlantRiccati& L, int rb, double* work, Team& team) {
    if (L.q && L.r) plant_riccati_chain_as<true>(L, rb, work, team);
    else plant_riccati_chain_as<false>(L, rb, work, team);
}

}  // namespace cimpc
