// The forward chain of a rollout over its step gradients (DESIGN.md sections 3, item 3d, and 5.5): from tangents of the initial states,
// the controls, the disturbances, friction, the time step and - on a closed-loop tape - the reference states to the tangents of the
// whole trajectory, for MANY directions at once.  Per robot and per direction d:
//
//   dq[0] = dq0, dq[1] = dq1
//   for t = 0 .. T-1:   closed-loop tape only (k the step's feedback row; the functions of plant_feedback.h on tangents - the law is linear):
//                           de[j]   = plant_feedback_error(dxref_t, dq[t], dq[t+1], nq, n_sample, j)      j = 0 .. 2nq-1   (dxref_t absent = zeros)
//                           du_t[i] = plant_feedback_control(K[k], de, nu, nq, i, dubar_t[i])              i = 0 .. nu-1
//                       limited closed-loop tape (item 3i; `clamped` non-null, the mask words of plant_feedback.h):
//                           du_t[i] = free ? plant_feedback_control(K[k], de, nu, nq, i, dubar_t[i]) : 0.0                 and du_applied stores it
//                       open-loop tape: du_t = dubar_t
//                       x = [dq[t]; dq[t+1]; du_t; dw_t; dmu; dh] cut to n_cols      (an input that was not passed is 0.0; nothing is skipped)
//                       y[r] = sum_{c = 0 .. n_cols-1} D_t[r, c] x[c]                ascending c from 0.0, one product and one sum per term
//                       dq[t+2] = y[0 : nq];  dgamma[t] = y[nq : nq+nc];  db[t] = y[nq+nc : nr]
//   outputs: dq (T+2) x B x nq, dgamma T x B x nc, db T x B x nb, on a closed-loop tape du_applied T x B x nu = du_t; n_cut B = the steps
//   whose gradient status is 0 (their D_t is all zeros, so dq[t+2] = 0 there: the flow is cut and counted, as in plant_adjoint.h)
//
// Every array of tangents carries a leading axis of n_dir directions.  A workgroup takes one robot and a GROUP of directions
// [d0, d0 + nd): D_t sits in the team's shared memory once per group, and a work item is one (row r, direction d) pair, r fastest
// across the team, so that consecutive members read consecutive doubles of a column of D_t and x[c] of their direction is a
// broadcast.  Every output element has one operation chain whatever the team, the group or the number of directions, so a direction's
// result does not depend by a bit on what rides with it.
//
// The chain of one (robot, group) is stated here ONCE for a team of workers, like plant_adjoint.h: plant_tangent_kernel
// (plant_tangent.hip) runs it with a workgroup of four wavefronts, a host program (tests/native/plant_tangent_check.cpp) with a team of
// one, statement for statement.  Team: rank(), size(), sync() and the two-phase fetch_issue / fetch_commit of plant_adjoint.h.
#pragma once
#include <cstddef>

#include "plant_feedback.h"

// no contraction in this header's arithmetic: a * b + c rounds twice
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define PTAN_HD __host__ __device__
#else
#define PTAN_HD
#endif

namespace cimpc {

// Every pointer in the memory the team reads (device memory for the kernel).  Tangents in: dq0, dq1 n_dir x B x nq; du_step n_dir x T x
// B x nu (dubar_t); dw_step n_dir x T x B x nw; dmu, dh n_dir x B; dxref_step n_dir x T x B x 2nq (with fb.K alone); null = zeros (the
// caller has checked that n_cols reaches the columns of those given).  dz: T x B x (nr x n_cols) column-major blocks, status: T x B.
// Out: dq n_dir x (T+2) x B x nq; dgamma n_dir x T x B x nc, db n_dir x T x B x nb, du_applied n_dir x T x B x nu (with fb.K alone):
// null = not asked for; n_cut B.
struct PlantTangent {
    const double* dz;
    const int* status;
    const double *dq0, *dq1, *du_step, *dw_step, *dmu, *dh;
    double *dq, *dgamma, *db;
    int* n_cut;
    int B, T, nq, nu, nw, nc, nb, n_cols, n_dir;
    PlantFeedback fb{};                   // fb.K null: an open-loop tape
    const double* dxref_step = nullptr;
    double* du_applied = nullptr;
    const int* clamped = nullptr;         // T x B mask words, with fb.K alone; null = a closed loop without limits (item 3i)
};

// the three compile-time states of the chain, as in plant_adjoint.h: open loop, closed loop, closed loop with the clamp's mask
constexpr int PLANT_TANGENT_OPEN = 0, PLANT_TANGENT_LOOP = 1, PLANT_TANGENT_CLAMP = 2;

// ---- the plan: what a group of nd directions needs of the team's shared memory, and how many directions a workgroup takes --------------
// per direction: x (n_cols), the three-row ring of dq (3 nq), and with feedback de (2nq); du_t has no buffer of its own: it is x[2nq : 2nq+nu]
PTAN_HD constexpr size_t plant_tangent_direction_doubles(int n_cols, int nq, int nu, bool feedback) {
    return (size_t)n_cols + (size_t)3 * nq + (feedback ? (size_t)2 * nq : 0);
}
// two blocks (the one in use and the one in flight), then the directions
PTAN_HD constexpr size_t plant_tangent_work_doubles(int nr, int n_cols, int nq, int nu, bool feedback, int nd) {
    return (size_t)2 * nr * n_cols + (size_t)nd * plant_tangent_direction_doubles(n_cols, nq, nu, feedback);
}
constexpr size_t PLANT_TAN_MAX_LDS = 160 * 1024;      // of a gfx950 CU
constexpr int PLANT_TAN_MAX_GROUP = 64;                // directions per workgroup at the most: further directions are further workgroups
constexpr size_t plant_tangent_lds(int nr, int n_cols, int nq, int nu, bool feedback, int nd) {
    return plant_tangent_work_doubles(nr, n_cols, nq, nu, feedback, nd) * sizeof(double);
}
constexpr bool plant_tangent_fits(int nr, int n_cols, int nq, int nu, bool feedback, int nd) {
    return nr >= 1 && n_cols >= 1 && nq >= 1 && nu >= 0 && nd >= 1 && plant_tangent_lds(nr, n_cols, nq, nu, feedback, nd) <= PLANT_TAN_MAX_LDS;
}
// directions per workgroup: as many as a CU's LDS holds beside the two blocks, PLANT_TAN_MAX_GROUP at the most; 0: not even one fits
constexpr int plant_tangent_group(int nr, int n_cols, int nq, int nu, bool feedback) {
    if (!plant_tangent_fits(nr, n_cols, nq, nu, feedback, 1)) return 0;
    const size_t room = PLANT_TAN_MAX_LDS / sizeof(double) - (size_t)2 * nr * n_cols;
    const size_t nd = room / plant_tangent_direction_doubles(n_cols, nq, nu, feedback);
    return nd < (size_t)PLANT_TAN_MAX_GROUP ? (int)nd : PLANT_TAN_MAX_GROUP;
}
static_assert(plant_tangent_direction_doubles(53, 18, 12, true) * sizeof(double) == 1144, "centroidal_quadruped_wall with feedback: 1.1 KB a direction");
static_assert(plant_tangent_lds(58, 53, 18, 12, true, 36) == 90368, "centroidal_quadruped_wall, every column, feedback, 2nq = 36 directions: 88 KB");
static_assert(plant_tangent_lds(58, 53, 18, 12, true, 0) == 49184, "its two blocks");
static_assert(plant_tangent_group(58, 53, 18, 12, true) == 64 && plant_tangent_lds(58, 53, 18, 12, true, 64) == 122400, "the largest model: a full group, 120 KB");
static_assert(plant_tangent_group(23, 30, 11, 8, false) == 64 && plant_tangent_lds(23, 30, 11, 8, false, 22) == 22128, "quadruped, the nine blocks, 2nq directions: 22 KB");

// the team of one: a host caller.  Its copy happens at commit time.
struct PlantTangentSolo {
    PTAN_HD int rank() const { return 0; }
    PTAN_HD int size() const { return 1; }
    PTAN_HD void sync() const {}
    PTAN_HD void fetch_issue(const double*, int) {}
    PTAN_HD void fetch_commit(double* dst, const double* src, int n) { for (int i = 0; i < n; ++i) dst[i] = src[i]; }
};

// The chain of robot rb for the directions [d0, d0 + nd), d0 + nd <= P.n_dir.  work: shared by the team,
// plant_tangent_work_doubles(nr, n_cols, nq, nu, FB != 0, nd).  FB != 0: the feedback statements are compiled in (the caller has P.fb.K
// non-null); without it the chain carries nothing of the feedback path.  FB == PLANT_TANGENT_CLAMP: the mask is read too (the caller has
// P.clamped non-null), its word of step t + 1 when block t + 1 is sent for; the other two carry nothing of it, and it needs no shared
// memory.  (`true` still names the closed loop: it converts to 1.)  The group with d0 = 0 reports n_cut.
template <int FB, class Team>
PTAN_HD inline void plant_tangent_chain_as(const PlantTangent& P, int rb, int d0, int nd, double* work, Team& team) {
    static_assert(FB == PLANT_TANGENT_OPEN || FB == PLANT_TANGENT_LOOP || FB == PLANT_TANGENT_CLAMP, "open loop, closed loop, or closed loop with the mask");
    const int me = team.rank(), np = team.size();
    const int nq = P.nq, nu = P.nu, nw = P.nw, nc = P.nc, nb = P.nb, n_cols = P.n_cols, B = P.B, T = P.T;
    const int nr = nq + nc + nb, blk = nr * n_cols;
    const int c_u = 2 * nq, c_w = c_u + nu, c_mu = c_w + nw, c_h = c_mu + 1;
    const size_t TB = (size_t)T * B;
    double* D[2] = {work, work + blk};
    double* xs = work + (size_t)2 * blk;                              // x of direction d: xs + d n_cols
    double* ring = xs + (size_t)nd * n_cols;                          // dq[t] of direction d lives in row 3 d + t % 3
    double* es = ring + (size_t)nd * 3 * nq;                          // with feedback alone: de, 2nq a direction
    auto block = [&](int t) { return P.dz + ((size_t)t * B + rb) * blk; };
    auto row = [&](int d, int t) { return ring + ((size_t)3 * d + t % 3) * nq; };

    for (int k = me; k < nd * nq; k += np) {                          // (i, d), i fastest
        const int i = k % nq, d = k / nq;
        const size_t in = ((size_t)(d0 + d) * B + rb) * nq + i;
        const double a0 = P.dq0 ? P.dq0[in] : 0.0, a1 = P.dq1 ? P.dq1[in] : 0.0;
        row(d, 0)[i] = a0;
        row(d, 1)[i] = a1;
        P.dq[((size_t)(d0 + d) * (T + 2) * B + rb) * nq + i] = a0;
        P.dq[(((size_t)(d0 + d) * (T + 2) + 1) * B + rb) * nq + i] = a1;
    }
    team.fetch_issue(block(0), blk);
    int word_next = 0;                                                // the mask word of the block in flight
    if constexpr (FB == PLANT_TANGENT_CLAMP) word_next = P.clamped[rb];
    team.fetch_commit(D[0], block(0), blk);
    team.sync();

    int cut = 0;
    for (int t = 0; t < T; ++t) {
        const size_t e = (size_t)t * B + rb;
        const int word = word_next;
        if (t + 1 < T) {
            team.fetch_issue(block(t + 1), blk);                      // in flight while block t is used
            if constexpr (FB == PLANT_TANGENT_CLAMP) word_next = P.clamped[e + B];
        }
        if (me == 0 && P.status[e] == 0) ++cut;
        // x but for its controls on a closed-loop tape, and de
        for (int k = me; k < nd * n_cols; k += np) {                  // (c, d), c fastest
            const int c = k % n_cols, d = k / n_cols;
            const size_t s = (size_t)(d0 + d) * TB + e;               // (direction, t, robot)
            double v;
            if (c < nq) v = row(d, t)[c];
            else if (c < c_u) v = row(d, t + 1)[c - nq];
            else if (c < c_w) { if constexpr (FB != PLANT_TANGENT_OPEN) continue; else v = P.du_step ? P.du_step[s * nu + (c - c_u)] : 0.0; }
            else if (c < c_mu) v = P.dw_step ? P.dw_step[s * nw + (c - c_w)] : 0.0;
            else if (c < c_h) v = P.dmu ? P.dmu[(size_t)(d0 + d) * B + rb] : 0.0;
            else v = P.dh ? P.dh[(size_t)(d0 + d) * B + rb] : 0.0;
            xs[(size_t)d * n_cols + c] = v;
        }
        if constexpr (FB != PLANT_TANGENT_OPEN) {                     // the feedback path of step t (plant_feedback.h), on tangents
            for (int k = me; k < nd * 2 * nq; k += np) {              // (j, d), j fastest
                const int j = k % (2 * nq), d = k / (2 * nq);
                double* de = es + (size_t)d * 2 * nq;
                de[j] = P.dxref_step ? P.dxref_step[((size_t)(d0 + d) * TB + e) * 2 * nq + j] : 0.0;      // the target of this member's own j
                de[j] = plant_feedback_error(de, row(d, t), row(d, t + 1), nq, P.fb.n_sample, j);
            }
            team.sync();                                              // de is whole
            const double* Kk = plant_feedback_gain(P.fb, t, rb, nu, nq);
            for (int k = me; k < nd * nu; k += np) {                  // (i, d), i fastest
                const int i = k % nu, d = k / nu;
                const size_t s = ((size_t)(d0 + d) * TB + e) * nu + i;
                double u;
                if constexpr (FB == PLANT_TANGENT_CLAMP) {            // item 3i: nothing passes a clamped control
                    u = plant_feedback_word_free(word, i) ? plant_feedback_control(Kk, es + (size_t)d * 2 * nq, nu, nq, i, P.du_step ? P.du_step[s] : 0.0) : 0.0;
                } else u = plant_feedback_control(Kk, es + (size_t)d * 2 * nq, nu, nq, i, P.du_step ? P.du_step[s] : 0.0);
                xs[(size_t)d * n_cols + c_u + i] = u;
                if (P.du_applied) P.du_applied[s] = u;
            }
        }
        team.sync();                                                  // x is whole
        const double* Dt = D[t & 1];
        for (int k = me; k < nd * nr; k += np) {                      // (r, d), r fastest: consecutive doubles of a column, x[c] a broadcast
            const int r = k % nr, d = k / nr;
            const double* x = xs + (size_t)d * n_cols;
            double y = 0.0;
            for (int c = 0; c < n_cols; ++c) y += Dt[(size_t)c * nr + r] * x[c];
            const size_t s = (size_t)(d0 + d) * TB + e;
            if (r < nq) {
                row(d, t + 2)[r] = y;
                P.dq[(((size_t)(d0 + d) * (T + 2) + t + 2) * B + rb) * nq + r] = y;
            } else if (r < nq + nc) { if (P.dgamma) P.dgamma[s * nc + (r - nq)] = y; }
            else if (P.db) P.db[s * nb + (r - nq - nc)] = y;
        }
        if (t + 1 < T) team.fetch_commit(D[(t + 1) & 1], block(t + 1), blk);      // its last reader left it at the end of step t - 1
        team.sync();
    }
    if (me == 0 && d0 == 0) P.n_cut[rb] = cut;
}

// The chain of (robot rb, group [d0, d0 + nd)), open or closed loop by what P carries.
template <class Team>
PTAN_HD inline void plant_tangent_chain(const PlantTangent& P, int rb, int d0, int nd, double* work, Team& team) {
    if (P.fb.K && P.clamped) plant_tangent_chain_as<PLANT_TANGENT_CLAMP>(P, rb, d0, nd, work, team);
    else if (P.fb.K) plant_tangent_chain_as<PLANT_TANGENT_LOOP>(P, rb, d0, nd, work, team);
    else plant_tangent_chain_as<PLANT_TANGENT_OPEN>(P, rb, d0, nd, work, team);
}

}  // namespace cimpc
