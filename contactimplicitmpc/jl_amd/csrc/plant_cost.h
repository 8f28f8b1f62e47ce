// The tracking cost of a rollout and the line search's rules (DESIGN.md sections 3, item 3f, and 5.5), stated ONCE for the kernels of
// plant_linesearch.hip, the host entry cimpc_plant_tracking_cost and a host program (tests/native/plant_cost_check.cpp).
//
// THE COST of one robot's trajectory q[0 .. T+1], with the controls u_t its steps applied: x_t = [q[t]; q[t+1]] (n = 2nq) for t = 0 .. T,
// u_t (m = nu) for t < T; weights as cimpc_plant_tape_lqr takes them, Q n_Q x (n x n) and R n_R x (m x m) column-major with n_Q, n_R 1 or
// T, Qf n x n, shared by the robots; targets x_goal (T+1) x n_x x n and u_goal T x n_x x m with n_x = 1 (shared) or B:
//
//   ex[j] = x_t[j] - x_goal_t[j]          qx_t[i] = sum_j Q_t[i, j] ex[j]      ascending j from 0.0, one rounded product and one rounded sum per term
//   eu[j] = u_t[j] - u_goal_t[j]          ru_t[i] = sum_j R_t[i, j] eu[j]
//   l_t   = 0.5 (sum_i ex[i] qx_t[i]) + 0.5 (sum_i eu[i] ru_t[i])      t < T;      l_T = 0.5 sum_i ex[i] (Qf ex)[i]      (ascending i from 0.0)
//   J     = (((l_0 + l_1) + ...) + l_T)                                  ascending t
//
// lin_q[t] = qx_t (lin_q[T] = Qf ex_T) and lin_r[t] = ru_t are the q, r of cimpc_plant_tape_lqr for the expansion about this trajectory.
// Every output element is one ordered chain, so the result does not depend on the team, the batch or what rides along.
//
// THE CANDIDATE LAW.  Candidate c of robot b is rollout robot c B + b: it starts from the parent's q[0], q[1], its open-loop row is
// ubar_t = u_nom[t, b] + alpha[c] k[t, b] (plant_candidate_control), it runs under the feedback law of plant_feedback.h with K_t[b], hold 1,
// n_sample 1.0 and x_ref[t] = [q[t+1] - 1.0 (q[t+1] - q[t]); q[t+1]] of the parent (plant_candidate_target), on robot b's w, mu and terrain.
//
// ACCEPTANCE.  Candidate c of robot b is acceptable iff every one of its T steps converged, J_c is finite and
// J_c <= J_nom[b] + armijo (alpha[c] dV1[b] + alpha[c]^2 dV2[b]) (plant_candidate_acceptable); choice[b] is the acceptable candidate of
// least J, the lower index on a tie, -1 if there is none (plant_linesearch_choice).
//
// No contraction in these functions (a * b + c rounds twice); the pragma stands inside each body, as in plant_feedback.h.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../../include/cimpc.h"

#ifdef __HIPCC__
#define PCOST_HD __host__ __device__
#else
#define PCOST_HD
#endif

namespace cimpc {

// Every pointer in the memory the team reads (device memory for the kernels).
struct PlantCost {
    const double *Q, *Qf, *R;          // n_Q x (n x n), n x n, n_R x (m x m), column-major
    const double *x_goal, *u_goal;     // (T+1) x n_x x n, T x n_x x m
    int n_Q, n_R, n_x;
    int T, nq, nu;
};

// The C ABI's cost on the caller's pointers, for a rollout of T steps of a model with nq, nu
inline PlantCost plant_cost_of(const cimpc_tracking_cost& c, int T, int nq, int nu) {
    return PlantCost{c.Q, c.Qf, c.R, c.x_goal, c.u_goal, c.n_Q, c.n_R, c.n_x, T, nq, nu};
}

// ex (n) | eu (m) | qx (n) | ru (m) | l_t and one of padding
PCOST_HD constexpr size_t plant_cost_work_doubles(int nq, int nu) { return (size_t)4 * nq + 2 * (size_t)nu + 2; }

// the team of one: a host caller
struct PlantCostSolo {
    PCOST_HD int rank() const { return 0; }
    PCOST_HD int size() const { return 1; }
    PCOST_HD void sync() const {}
};

// l_t of stage t (0 .. T) of a robot whose goals are column g (0 with n_x = 1): q0 = q[t], q1 = q[t+1], u = u_t (not read at t = T).
// lin_q (n) and lin_r (m, not written at t = T) receive qx_t and ru_t where given.  Every member gets l_t; the team is synchronized on
// return, so `work` may be reused at once.
template <class Team>
PCOST_HD inline double plant_cost_stage(const PlantCost& C, int t, int g, const double* q0, const double* q1, const double* u, double* work,
                                        double* lin_q, double* lin_r, Team& team) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const int nq = C.nq, n = 2 * C.nq, m = C.nu;
    const bool last = t == C.T;
    double *ex = work, *eu = ex + n, *qx = eu + m, *ru = qx + n, *lt = ru + m;
    const double* xg = C.x_goal + ((size_t)t * C.n_x + g) * n;
    for (int j = team.rank(); j < n; j += team.size()) ex[j] = (j < nq ? q0[j] : q1[j - nq]) - xg[j];
    if (!last) {
        const double* ug = C.u_goal + ((size_t)t * C.n_x + g) * m;
        for (int j = team.rank(); j < m; j += team.size()) eu[j] = u[j] - ug[j];
    }
    team.sync();
    const double* Qt = last ? C.Qf : C.Q + (C.n_Q == 1 ? 0 : (size_t)t * n * n);
    for (int i = team.rank(); i < n; i += team.size()) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = s + Qt[(size_t)j * n + i] * ex[j];
        qx[i] = s;
        if (lin_q) lin_q[i] = s;
    }
    if (!last) {
        const double* Rt = C.R + (C.n_R == 1 ? 0 : (size_t)t * m * m);
        for (int i = team.rank(); i < m; i += team.size()) {
            double s = 0.0;
            for (int j = 0; j < m; ++j) s = s + Rt[(size_t)j * m + i] * eu[j];
            ru[i] = s;
            if (lin_r) lin_r[i] = s;
        }
    }
    team.sync();
    if (team.rank() == 0) {
        double a = 0.0;
        for (int i = 0; i < n; ++i) a = a + ex[i] * qx[i];
        double l = 0.5 * a;
        if (!last) {
            double c = 0.0;
            for (int i = 0; i < m; ++i) c = c + eu[i] * ru[i];
            l = l + 0.5 * c;
        }
        lt[0] = l;
    }
    team.sync();
    const double l = lt[0];
    team.sync();
    return l;
}

// J of one robot: q its trajectory row 0 with q_stride doubles between rows, u its control row 0 with u_stride between rows; lin_q, lin_r
// (null: not asked for) its rows alike.  Every member gets J.
template <class Team>
PCOST_HD inline double plant_cost_trajectory(const PlantCost& C, int g, const double* q, size_t q_stride, const double* u, size_t u_stride,
                                             double* work, double* lin_q, size_t lq_stride, double* lin_r, size_t lr_stride, Team& team) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double J = 0.0;
    for (int t = 0; t <= C.T; ++t) {
        const double l = plant_cost_stage(C, t, g, q + (size_t)t * q_stride, q + (size_t)(t + 1) * q_stride, t < C.T ? u + (size_t)t * u_stride : nullptr,
                                          work, lin_q ? lin_q + (size_t)t * lq_stride : nullptr, (lin_r && t < C.T) ? lin_r + (size_t)t * lr_stride : nullptr,
                                          team);
        J = t == 0 ? l : J + l;
    }
    return J;
}

// ubar_t[i] of a candidate: one rounded product, one rounded sum
PCOST_HD inline double plant_candidate_control(double u_nom, double alpha, double k) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return u_nom + alpha * k;
}

// x_ref[t][j] of a candidate, from the parent's q0 = q[t], q1 = q[t+1]: what TapeGains.feedback writes, so that on the parent's own
// trajectory the law's error is exactly zero
PCOST_HD inline double plant_candidate_target(const double* q0, const double* q1, int nq, int j) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return j < nq ? q1[j] - 1.0 * (q1[j] - q0[j]) : q1[j - nq];
}

PCOST_HD inline bool plant_candidate_acceptable(bool converged, double J, double J_nom, double armijo, double alpha, double dV1, double dV2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return converged && std::isfinite(J) && J <= J_nom + armijo * (alpha * dV1 + (alpha * alpha) * dV2);
}

// choice of one robot among its n_alpha candidates: candidate c's J at J[c * J_stride], its acceptability at ok[c * ok_stride]
PCOST_HD inline int plant_linesearch_choice(const double* J, size_t J_stride, const int* ok, size_t ok_stride, int n_alpha) {
    int best = -1;
    for (int c = 0; c < n_alpha; ++c)
        if (ok[c * ok_stride] && (best < 0 || J[c * J_stride] < J[best * J_stride])) best = c;
    return best;
}

// What cimpc_plant_tape_linesearch refuses before any device is touched, beside its null pointers, the tape and the rollout's own check
// (plant_rollout_check).  Each returns the reason of the refusal, or null.  The tests that need no tape come first in the entry
// (plant_cost_pointers, plant_linesearch_refusal), those against the tape's B and T after it (plant_cost_sizes, plant_linesearch_fits).
inline const char* plant_cost_pointers(const PlantCost& C) {
    if (!C.Q || !C.Qf || !C.R || !C.x_goal || !C.u_goal) return "a null pointer in the cost";
    if (C.n_Q < 1 || C.n_R < 1 || C.n_x < 1) return "n_Q, n_R or n_x of the cost below 1";
    return nullptr;
}
inline const char* plant_cost_sizes(const PlantCost& C, int B) {
    if (C.T < 1 || C.nq < 1 || C.nu < 1 || B < 1) return "nq, nu, B or T below 1";
    if (C.n_Q != 1 && C.n_Q != C.T) return "n_Q of the cost neither 1 nor T";
    if (C.n_R != 1 && C.n_R != C.T) return "n_R of the cost neither 1 nor T";
    if (C.n_x != 1 && C.n_x != B) return "n_x of the cost neither 1 nor B";
    return nullptr;
}
inline bool plant_cost_valid(const PlantCost& C, int B) { return !plant_cost_pointers(C) && !plant_cost_sizes(C, B); }

constexpr int PLANT_LS_MAX_ALPHA = 64;      // the gather kernel keeps a flag per candidate of a robot in LDS
inline const char* plant_linesearch_refusal(int n_alpha, const double* alpha, double armijo) {
    if (!alpha) return "null alpha";
    if (n_alpha < 1 || n_alpha > PLANT_LS_MAX_ALPHA) return "n_alpha outside 1 .. 64";
    for (int c = 0; c < n_alpha; ++c) if (!std::isfinite(alpha[c])) return "a non-finite alpha";
    if (!(armijo >= 0.0)) return "armijo negative or not a number";
    return nullptr;
}
// n_alpha B T entries are indexed by an int
inline bool plant_linesearch_fits(int n_alpha, int B, int T) { return B >= 1 && T >= 1 && (long long)n_alpha * B * T <= 2147483647LL; }

}  // namespace cimpc
