// The reverse chain of a rollout over its step gradients (DESIGN.md sections 3, item 3b, and 5.5): from cotangents of the trajectory
// to the gradient of a loss with respect to the initial states, the controls, the disturbances, friction and the time step.
//
//   lambda[0 .. T+1] = gq
//   for t = T-1 .. 0:   a = [lambda[t+2]; ggamma[t]; gb[t]]                      (nr = nq + nc + nb)
//                       v[c] = sum_{r = 0 .. nr-1} D_t[r, c] a[r]                 ascending r from 0.0, one product and one sum per term
//                       lambda[t+1] += v[nq : 2nq];  lambda[t] += v[0 : nq]      lambda[t] = (gq[t] + v_t[0:nq]) + v_{t-1}[nq:2nq]
//                       g_u_step[t] = v[2nq : 2nq+nu];  g_w_step[t] = v[w columns];  g_mu += v[mu column];  g_h += v[h column]
//   g_q0 = lambda[0], g_q1 = lambda[1], n_cut = the steps whose gradient status is 0 (their D_t is all zeros)
//
// The chain of a CLOSED-LOOP rollout (item 3c, plant_feedback.h: u_t = ubar_t + K (x_ref - x), the blocks taken with u_t as a column
// of theta) adds, after v = D_t' a of step t, with gu = v[2nq : 2nq+nu] and k the feedback row of step t:
//                       gx[j] = sum_{i = 0 .. nu-1} K[k][i, j] gu[i]               ascending i from 0.0;   g_xref_step[t] = gx
//                       lambda[t][i]   = lambda[t][i] - n_sample gx[i]             i < nq, after lambda[t] received gq[t] + v[0:nq]
//                       lambda[t+1][i] = (lambda[t+1][i] - (1 - n_sample) gx[i]) - gx[nq + i]      after lambda[t+1] received v[nq:2nq]
// g_u_step stays gu, which is also the gradient of ubar_t.  Without a feedback schedule (fb.K null) none of these statements runs.
//
// The chain of a LIMITED closed-loop rollout (item 3i; `clamped` non-null, T x B mask words, bit i set where control i of the step is
// clamped - plant_feedback_free of plant_feedback.h on the applied control) changes one statement: for column c_u + i, after v is formed,
//                       gm = free ? v : 0.0;   g_u_step[t][i] = gm;   gu[i] = gm
// and everything behind it is unchanged: a clamped control passes nothing to ubar, K or x.  The mask word of step t - 1 is read when block
// t - 1 is sent for, a step ahead of its use.
//
// D_t is the step's dz block of plant_sensitivity.hip, nr x n_cols column-major, contiguous per (t, robot).  The chain of one robot
// is stated here ONCE for a team of workers, the way lin_table_build.h states a table: plant_adjoint_kernel (plant_adjoint.hip) runs it
// with a wavefront per robot, a host program (tests/native/plant_adjoint_check.cpp) with a team of one, statement for statement.
// Every output element has one operation chain whatever the team, so the result does not depend by a bit on who computed it.
//
// Team: rank() in [0, size()), sync() a barrier that also orders the team's memory operations, and a two-phase copy of n doubles into
// the team's shared memory: fetch_issue(src, n) starts it (a wavefront: loads into registers), fetch_commit(dst, src, n) lands it and
// is followed by a sync() before dst is read.  Between the two the team works on the other block: the blocks do not depend on the chain.
#pragma once
#include <cstddef>

#include "plant_feedback.h"

// no contraction in this header's arithmetic: a * b + c rounds twice
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define PADJ_HD __host__ __device__
#else
#define PADJ_HD
#endif

namespace cimpc {

// One robot's chain, every pointer in the memory the team reads (device memory for the kernel).  Cotangents: gq (T + 2) x B x nq,
// ggamma T x B x nc, gb T x B x nb; null = zeros.  dz: T x B x (nr x n_cols), status: T x B.  Outputs: g_q0, g_q1 B x nq, g_u_step
// T x B x nu; g_w_step T x B x nw, g_mu B, g_h B: null = not asked for (the caller has checked that n_cols reaches their columns);
// n_cut B.
struct PlantAdjoint {
    const double* dz;
    const int* status;
    const double *gq, *ggamma, *gb;
    double *g_q0, *g_q1, *g_u_step, *g_w_step, *g_mu, *g_h;
    int* n_cut;
    int B, T, nq, nu, nw, nc, nb, n_cols;
    PlantFeedback fb{};               // fb.K null: an open-loop rollout
    double* g_xref_step = nullptr;    // T x B x 2nq, with fb.K alone; null = not asked for
    const int* clamped = nullptr;     // T x B mask words, with fb.K alone; null = a closed loop without limits (item 3i)
};

// the three compile-time states of the chain, as LOOP is of the step kernel: open loop, closed loop, closed loop with the clamp's mask
constexpr int PLANT_CHAIN_OPEN = 0, PLANT_CHAIN_LOOP = 1, PLANT_CHAIN_CLAMP = 2;

// doubles of the team's shared workspace: two blocks (the one in use and the one in flight), a, the three-row ring of lambda
PADJ_HD constexpr size_t plant_adjoint_work_doubles(int nr, int n_cols, int nq) {
    return (size_t)2 * nr * n_cols + (size_t)nr + (size_t)3 * nq;
}
// what a closed-loop chain adds behind them: gu (nu) and gx (2nq)
PADJ_HD constexpr size_t plant_adjoint_feedback_doubles(int nu, int nq) { return (size_t)nu + (size_t)2 * nq; }
// what a launch of plant_adjoint_kernel needs of a CU's LDS (all of it dynamic), and whether a CU has it
constexpr size_t PLANT_ADJ_MAX_LDS = 160 * 1024;      // of a gfx950 CU
constexpr size_t plant_adjoint_lds(int nr, int n_cols, int nq) { return plant_adjoint_work_doubles(nr, n_cols, nq) * sizeof(double); }
constexpr bool plant_adjoint_fits(int nr, int n_cols, int nq) {
    return nr >= 1 && n_cols >= 1 && nq >= 1 && plant_adjoint_lds(nr, n_cols, nq) <= PLANT_ADJ_MAX_LDS;
}
static_assert(plant_adjoint_lds(58, 53, 18) == 50080, "centroidal_quadruped_wall, every column of theta: 49 KB, the largest model");
static_assert(plant_adjoint_lds(23, 30, 11) == 11488, "quadruped, the nine blocks: 11 KB");

// the team of one: a host caller.  Its copy happens at commit time.
struct PlantAdjointSolo {
    PADJ_HD int rank() const { return 0; }
    PADJ_HD int size() const { return 1; }
    PADJ_HD void sync() const {}
    PADJ_HD void fetch_issue(const double*, int) {}
    PADJ_HD void fetch_commit(double* dst, const double* src, int n) { for (int i = 0; i < n; ++i) dst[i] = src[i]; }
};

// The chain of robot rb.  work: shared by the team, plant_adjoint_work_doubles(nr, n_cols, nq), with a feedback schedule
// plant_adjoint_feedback_doubles(nu, nq) more.  FB != 0: the feedback statements are compiled in (the caller has P.fb.K non-null); without
// it the chain is, statement for statement, the open-loop one - plant_adjoint_kernel is instantiated each way and the open-loop launch
// carries nothing of the feedback path.  FB == PLANT_CHAIN_CLAMP: the mask is read too (the caller has P.clamped non-null); the other two
// carry nothing of it.  (`true` still names the closed loop: it converts to 1.)
template <int FB, class Team>
PADJ_HD inline void plant_adjoint_chain_as(const PlantAdjoint& P, int rb, double* work, Team& team) {
    static_assert(FB == PLANT_CHAIN_OPEN || FB == PLANT_CHAIN_LOOP || FB == PLANT_CHAIN_CLAMP, "open loop, closed loop, or closed loop with the mask");
    const int me = team.rank(), np = team.size();
    const int nq = P.nq, nu = P.nu, nw = P.nw, nc = P.nc, nb = P.nb, n_cols = P.n_cols, B = P.B, T = P.T;
    const int nr = nq + nc + nb, blk = nr * n_cols;
    const int c_u = 2 * nq, c_w = c_u + nu, c_mu = c_w + nw, c_h = c_mu + 1;
    double* D[2] = {work, work + blk};
    double* a = work + (size_t)2 * blk;
    double* ring = a + nr;                                            // lambda[t] lives in row t % 3
    double* gu = ring + (size_t)3 * nq;                               // with feedback alone: the step's control cotangents and gx
    double* gx = gu + nu;
    auto block = [&](int t) { return P.dz + ((size_t)t * B + rb) * blk; };
    auto row = [&](int t) { return ring + (t % 3) * nq; };

    for (int i = me; i < nq; i += np) {
        row(T + 1)[i] = P.gq ? P.gq[((size_t)(T + 1) * B + rb) * nq + i] : 0.0;
        row(T)[i] = P.gq ? P.gq[((size_t)T * B + rb) * nq + i] : 0.0;
    }
    team.fetch_issue(block(T - 1), blk);
    int word_next = 0;                                                // the mask word of the block in flight
    if constexpr (FB == PLANT_CHAIN_CLAMP) word_next = P.clamped[(size_t)(T - 1) * B + rb];
    team.fetch_commit(D[(T - 1) & 1], block(T - 1), blk);
    team.sync();

    double s_mu = 0.0, s_h = 0.0;                                     // running sums of the member that owns the column, t descending
    int cut = 0;
    for (int t = T - 1; t >= 0; --t) {
        const size_t e = (size_t)t * B + rb;
        const int word = word_next;
        if (t > 0) {
            team.fetch_issue(block(t - 1), blk);                      // in flight while block t is used
            if constexpr (FB == PLANT_CHAIN_CLAMP) word_next = P.clamped[e - B];
        }
        if (me == 0 && P.status[e] == 0) ++cut;
        const double* l2 = row(t + 2);
        for (int i = me; i < nr; i += np)
            a[i] = i < nq ? l2[i] : i < nq + nc ? (P.ggamma ? P.ggamma[e * nc + (i - nq)] : 0.0) : (P.gb ? P.gb[e * nb + (i - nq - nc)] : 0.0);
        team.sync();
        const double* Dt = D[t & 1];
        double* l1 = row(t + 1);
        double* l0 = row(t);
        for (int c = me; c < n_cols; c += np) {                       // a member owns column c, c + np, ...
            const double* col = Dt + (size_t)c * nr;
            double v = 0.0;
            for (int r = 0; r < nr; ++r) v += col[r] * a[r];
            if (c < nq) l0[c] = (P.gq ? P.gq[e * nq + c] : 0.0) + v;
            else if (c < c_u) l1[c - nq] += v;
            else if (c < c_w) {
                if constexpr (FB == PLANT_CHAIN_CLAMP) v = plant_feedback_word_free(word, c - c_u) ? v : 0.0;      // gm of item 3i
                P.g_u_step[e * nu + (c - c_u)] = v;
                if constexpr (FB != PLANT_CHAIN_OPEN) gu[c - c_u] = v;
            }
            else if (c < c_mu) { if (P.g_w_step) P.g_w_step[e * nw + (c - c_w)] = v; }
            else if (c < c_h) s_mu += v;
            else s_h += v;
        }
        if constexpr (FB != PLANT_CHAIN_OPEN) {                       // the feedback path of step t (plant_feedback.h)
            const double* Kk = plant_feedback_gain(P.fb, t, rb, nu, nq);
            team.sync();                                              // gu, lambda[t] and lambda[t+1] are whole
            for (int j = me; j < 2 * nq; j += np) {                   // the member that owns column j
                const double g = plant_feedback_pull(Kk, gu, nu, j);
                gx[j] = g;
                if (P.g_xref_step) P.g_xref_step[e * 2 * nq + j] = g;
            }
            team.sync();
            for (int i = me; i < nq; i += np) {
                l0[i] = plant_feedback_lambda0(l0[i], gx, P.fb.n_sample, i);
                l1[i] = plant_feedback_lambda1(l1[i], gx, P.fb.n_sample, nq, i);
            }
        }
        if (t > 0) team.fetch_commit(D[(t - 1) & 1], block(t - 1), blk);      // its last reader left it at the end of step t + 1
        team.sync();
    }
    for (int i = me; i < nq; i += np) {
        P.g_q0[(size_t)rb * nq + i] = row(0)[i];
        P.g_q1[(size_t)rb * nq + i] = row(1)[i];
    }
    // columns c_mu and c_h belong to members c_mu % np and c_h % np: theirs are the sums
    if (P.g_mu && c_mu < n_cols && me == c_mu % np) P.g_mu[rb] = s_mu;
    if (P.g_h && c_h < n_cols && me == c_h % np) P.g_h[rb] = s_h;
    if (me == 0) P.n_cut[rb] = cut;
}

// The chain of robot rb, open or closed loop by what P carries.
template <class Team>
PADJ_HD inline void plant_adjoint_chain(const PlantAdjoint& P, int rb, double* work, Team& team) {
    if (P.fb.K && P.clamped) plant_adjoint_chain_as<PLANT_CHAIN_CLAMP>(P, rb, work, team);
    else if (P.fb.K) plant_adjoint_chain_as<PLANT_CHAIN_LOOP>(P, rb, work, team);
    else plant_adjoint_chain_as<PLANT_CHAIN_OPEN>(P, rb, work, team);
}

}  // namespace cimpc
