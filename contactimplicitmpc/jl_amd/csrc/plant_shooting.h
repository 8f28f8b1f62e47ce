// Multiple shooting on the device plant (DESIGN.md sections 3, item 3l, and 5.5): the horizon of T steps cut into M segments of L = T / M
// steps that roll out abreast, stated ONCE for the kernels of plant_shooting.hip, the host entry cimpc_plant_shooting_cost and a host
// program (tests/native/plant_shooting_check.cpp).  Plain C++, contraction off inside each body, as plant_cost.h.
//
// SEGMENTS AND LAYOUT.  T = M L (a T that M does not divide and M < 1 are refused).  Segment j (0 .. M-1) of robot b is virtual robot
// r = j B + b (plant_shoot_robot) of a rollout of M B robots for L steps; its trajectory rows are qs[l, r], l = 0 .. L+1, and its step l is
// global step t = j L + l (plant_shoot_step).  Node j is x^_j = [qs[0, j B + b]; qs[1, j B + b]] (2nq numbers): what segment j starts
// from.  Node 0 is the measured state.  Step l of segment j reads the inputs of global step t: the control row u[t, b], the w row
// rollout_row(t, hold_w, K_w) of robot b, and mu, terrain and limits of robot b.
//
// DEFECT of node j = 1 .. M-1 (plant_shoot_defect): d_j[i] = [qs[L, (j-1) B + b]; qs[L+1, (j-1) B + b]][i] - x^_j[i], one rounded
// difference: where segment j-1 ends less where segment j starts.  D[b] = sum_j sum_i |d_j[i]| in ascending j, then i, as one running sum
// from 0.0 (plant_shoot_defect_sum).
//
// COST.  Stage t < T is plant_cost_stage (plant_cost.h) on rows l, l+1 of the segment that owns step t (plant_shoot_stage_rows), with the
// goals, Q_t and R_t of global step t; the terminal stage is taken on rows L, L+1 of the last segment.  J = (((l_0 + l_1) + ...) + l_T) in
// ascending global t (plant_shoot_total on the l_t), so M = 1 gives plant_cost_trajectory's bits.  lin_q (T+1) x B x 2nq and lin_r T x B x nu
// are the stages' qx_t and ru_t in global layout.  Merit phi = J + nu D with nu the defect weight: one rounded product, one rounded sum
// (plant_shoot_merit).
//
// THE LINEAR FORWARD PASS of one robot at alpha = 1 (plant_shoot_forward_chain), about the segments' trajectories, with the gains K_t, k_t of
// the backward pass with defects (plant_riccati.h), A_t = [0 I; D1 D2], B_t = [0; Du] from the tape's blocks (a cut step's block is zero) and
// d_{t+1} the defect where t + 1 is a node, zero elsewhere:
//   dx_0 = 0;   du_t[i] = k_t[i] - (sum_j K_t[i, j] dx_t[j]);
//   dx_{t+1}[i] = dx_t[nq + i] (+ d[i])                                                       i < nq
//   dx_{t+1}[nq + r] = (sum_j D[r, j] dx_t[j], continued by sum_j Du[r, j] du_t[j]) (+ d[nq + r])      one running sum over both parts
//   dJ1 = sum_t ((lin_q[t].dx_t) + (lin_r[t].du_t)) + lin_q[T].dx_T;   dJ2 = sum_t (0.5 (dx_t'(Q_t dx_t)) + 0.5 (du_t'(R_t du_t))) + 0.5 (dx_T'(Qf dx_T))
// every sum ascending from 0.0, one rounded product and one rounded sum per term, the stages added in ascending t as bracketed.  It returns
// dx at the nodes, dJ1 and dJ2, and du where asked for.  The chain is stated for a team (rank, size, sync and the two-phase fetch of a block's
// corner of plant_riccati.h, the next step's corner in flight while a step is worked): plant_shoot_forward_kernel runs it with a workgroup
// per robot, a host program with a team of one, statement for statement.
//
// THE CANDIDATE LAW.  Candidate c of segment j of robot b is rollout robot (c M + j) B + b (plant_shoot_candidate_robot) of ONE closed-loop
// rollout of n_alpha M B robots for L steps.  It starts from node j moved along the forward pass, x^_j + alpha_c dx_{jL}, each entry one rounded
// product and one rounded sum (plant_shoot_candidate_node); node 0 is left as it stands.  On its segment's own rows it runs plant_cost.h's
// candidate law: open-loop row limit(u_nom[jL + l, b] + alpha_c k[jL + l, b]), gains K_{jL + l}[b], x_ref from plant_candidate_target on the
// segment's parent rows l, l+1, hold 1, n_sample 1.0, on the w row of global step jL + l and robot b's mu, terrain and limits.
// A candidate's J is the cost above on its own M segments with the controls its steps applied (plant_shoot_candidate_cost), its defects and
// D those of its own segments (plant_shoot_candidate_defect, _defect_sum), its merit phi_c = J_c + nu D_c.
//
// ACCEPTANCE.  A candidate of robot b is acceptable iff all M L of its steps converged, phi_c is finite and
// phi_c <= phi_nom + armijo (alpha (dJ1 - nu D_nom) + alpha^2 dJ2) (plant_shoot_acceptable): the model's decrease of J and, along the full
// step, the closing of every gap.  The choice is the acceptable candidate of least phi, the lower index on a tie, else -1
// (plant_linesearch_choice on phi).  With M = 1 there is no defect, D = 0.0 and nu is passed as 0.0: these are plant_candidate_acceptable and
// plant_linesearch_choice to the bit.
//
// LOOP BOOKKEEPING (plant.ilqr_shooting, a host loop): plant_ilqr.h's NumPy lines with phi in the place of J;
// small = accepted and (phi - phi_new < tol |phi|) and (D_new <= defect_tol); the rho ladder, rho_max and `active` are unchanged.
//
// STITCHING.  Entry l (M B) + j B + b of the segments' rollout is entry (j L + l) B + b of a rollout in (T, B) layout
// (plant_shoot_entry, plant_shoot_stitched): the tape of a segmented rollout holds each step's block where an ordinary tape holds it.
#pragma once
#include <cmath>
#include <cstddef>

#include "plant_cost.h"
#include "plant_riccati.h"

namespace cimpc {

// Why a segmentation is refused, or null: before any device is touched
inline const char* plant_shooting_refusal(int T, int M, int B) {
    if (B < 1 || T < 1) return "B or T below 1";
    if (M < 1) return "segments below 1";
    if (T % M != 0) return "T not divisible by segments";
    if ((long long)T * B > 2147483647LL) return "T B beyond an int";
    return nullptr;
}
// Why the nodes (M x B x 2nq) are refused, or null
inline const char* plant_shooting_nodes_refusal(const double* nodes, int M, int B, int nq) {
    if (!nodes) return "null nodes";
    for (size_t e = 0; e < (size_t)M * B * 2 * nq; ++e) if (!std::isfinite(nodes[e])) return "a non-finite entry of nodes";
    return nullptr;
}

PCOST_HD constexpr int plant_shoot_robot(int j, int B, int b) { return j * B + b; }
PCOST_HD constexpr int plant_shoot_step(int j, int L, int l) { return j * L + l; }
// entry (l, j, b) of the segments' rollout, and where it lies in (T, B) layout
PCOST_HD constexpr size_t plant_shoot_entry(int l, int j, int b, int M, int B) { return ((size_t)l * M + j) * B + b; }
PCOST_HD constexpr size_t plant_shoot_stitched(int l, int j, int b, int L, int B) { return (size_t)plant_shoot_step(j, L, l) * B + b; }

// The segment and the row of it that stage t (0 .. T) is taken on: rows l, l+1 of segment j; the terminal stage on rows L, L+1 of the last
struct PlantShootRows { int j, l; };
PCOST_HD constexpr PlantShootRows plant_shoot_stage_rows(int t, int T, int L) { return t < T ? PlantShootRows{t / L, t % L} : PlantShootRows{T / L - 1, L}; }
static_assert(plant_shoot_stage_rows(0, 12, 3).j == 0 && plant_shoot_stage_rows(3, 12, 3).j == 1 && plant_shoot_stage_rows(3, 12, 3).l == 0 &&
                  plant_shoot_stage_rows(11, 12, 3).l == 2 && plant_shoot_stage_rows(12, 12, 3).j == 3 && plant_shoot_stage_rows(12, 12, 3).l == 3,
              "a step belongs to the segment that takes it; the terminal stage to the last one");
static_assert(plant_shoot_stage_rows(5, 12, 1).j == 5 && plant_shoot_stage_rows(5, 12, 1).l == 0 && plant_shoot_stage_rows(12, 12, 1).j == 11 &&
                  plant_shoot_stage_rows(12, 12, 1).l == 1, "L = 1: every step its own segment");
static_assert(plant_shoot_entry(2, 1, 0, 4, 3) == 27 && plant_shoot_stitched(2, 1, 0, 3, 3) == 15, "entry (l, j, b) and its place in (T, B) layout");

// d_j[i] of robot b, j = 1 .. M-1, i = 0 .. 2nq-1; qs (L+2) x (M B) x nq
PCOST_HD inline double plant_shoot_defect(const double* qs, int M, int B, int L, int nq, int j, int b, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const size_t row = (size_t)M * B * nq, prev = (size_t)plant_shoot_robot(j - 1, B, b) * nq, own = (size_t)plant_shoot_robot(j, B, b) * nq;
    return i < nq ? qs[(size_t)L * row + prev + i] - qs[own + i] : qs[(size_t)(L + 1) * row + prev + (i - nq)] - qs[row + own + (i - nq)];
}

// D[b] of defects (M-1) x B x 2nq
PCOST_HD inline double plant_shoot_defect_sum(const double* defects, int M, int B, int nq, int b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double D = 0.0;
    for (int j = 1; j < M; ++j)
        for (int i = 0; i < 2 * nq; ++i) D = D + std::fabs(defects[((size_t)(j - 1) * B + b) * 2 * nq + i]);
    return D;
}

// J of robot b from its stage costs l (T+1) x B
PCOST_HD inline double plant_shoot_total(const double* l, int T, int B, int b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double J = l[b];
    for (int t = 1; t <= T; ++t) J = J + l[(size_t)t * B + b];
    return J;
}

PCOST_HD inline double plant_shoot_merit(double J, double weight, double D) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return J + weight * D;
}

// l_t of stage t (0 .. T) of robot b on its segments' rows: qs (L+2) x (M B) x nq, u T x B x nu in global layout; lin_q (2nq) and lin_r (nu,
// not written at t = T) receive the stage's qx_t and ru_t where given.  C carries the global T; the team is synchronized on return.
template <class Team>
PCOST_HD inline double plant_shoot_stage(const PlantCost& C, int M, int B, int t, int b, const double* qs, const double* u, double* work, double* lin_q,
                                         double* lin_r, Team& team) {
    const int L = C.T / M, nq = C.nq;
    const PlantShootRows at = plant_shoot_stage_rows(t, C.T, L);
    const size_t row = (size_t)M * B * nq, r = (size_t)plant_shoot_robot(at.j, B, b) * nq;
    return plant_cost_stage(C, t, C.n_x == 1 ? 0 : b, qs + (size_t)at.l * row + r, qs + (size_t)(at.l + 1) * row + r,
                            t < C.T ? u + ((size_t)t * B + b) * C.nu : nullptr, work, lin_q, t < C.T ? lin_r : nullptr, team);
}

// J of robot b, every stage in ascending global t; lin_q (T+1) x B x 2nq and lin_r T x B x nu in global layout (null: not asked for)
template <class Team>
PCOST_HD inline double plant_shoot_cost(const PlantCost& C, int M, int B, int b, const double* qs, const double* u, double* work, double* lin_q,
                                        double* lin_r, Team& team) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const size_t n = (size_t)2 * C.nq;
    double J = 0.0;
    for (int t = 0; t <= C.T; ++t) {
        const double l = plant_shoot_stage(C, M, B, t, b, qs, u, work, lin_q ? lin_q + ((size_t)t * B + b) * n : nullptr,
                                           (lin_r && t < C.T) ? lin_r + ((size_t)t * B + b) * C.nu : nullptr, team);
        J = t == 0 ? l : J + l;
    }
    return J;
}

// ---- the candidates of the line search ---------------------------------------------------------------------------------------------------
PCOST_HD constexpr int plant_shoot_candidate_robot(int c, int j, int b, int M, int B) { return (c * M + j) * B + b; }
static_assert(plant_shoot_candidate_robot(2, 1, 0, 4, 3) == 27 && plant_shoot_candidate_robot(1, 0, 2, 1, 3) == 5, "(c, j, b); with M = 1 it is c B + b");

PCOST_HD inline double plant_shoot_candidate_node(double x, double alpha, double dx) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return x + alpha * dx;
}

PCOST_HD inline bool plant_shoot_acceptable(bool converged, double phi, double phi_nom, double armijo, double alpha, double dJ1, double dJ2, double weight,
                                            double D_nom) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return converged && std::isfinite(phi) && phi <= phi_nom + armijo * (alpha * (dJ1 - weight * D_nom) + (alpha * alpha) * dJ2);
}

// d_j[i] of candidate c of robot b from the candidates' trajectories q (L+2) x NB x nq
PCOST_HD inline double plant_shoot_candidate_defect(const double* q, int M, int B, int NB, int L, int nq, int c, int j, int b, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const size_t row = (size_t)NB * nq, prev = (size_t)plant_shoot_candidate_robot(c, j - 1, b, M, B) * nq, own = (size_t)plant_shoot_candidate_robot(c, j, b, M, B) * nq;
    return i < nq ? q[(size_t)L * row + prev + i] - q[own + i] : q[(size_t)(L + 1) * row + prev + (i - nq)] - q[row + own + (i - nq)];
}

PCOST_HD inline double plant_shoot_candidate_defect_sum(const double* q, int M, int B, int NB, int L, int nq, int c, int b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double D = 0.0;
    for (int j = 1; j < M; ++j)
        for (int i = 0; i < 2 * nq; ++i) D = D + std::fabs(plant_shoot_candidate_defect(q, M, B, NB, L, nq, c, j, b, i));
    return D;
}

// J of candidate c of robot b: every stage in ascending global t on the rows of the candidate's own segments, with the controls its steps
// applied, u_applied L x NB x nu.  Every member gets J.
template <class Team>
PCOST_HD inline double plant_shoot_candidate_cost(const PlantCost& C, int M, int B, int NB, int c, int b, const double* q, const double* u_applied, double* work,
                                                  Team& team) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const int L = C.T / M, nq = C.nq;
    const size_t row = (size_t)NB * nq;
    double J = 0.0;
    for (int t = 0; t <= C.T; ++t) {
        const PlantShootRows at = plant_shoot_stage_rows(t, C.T, L);
        const size_t R = (size_t)plant_shoot_candidate_robot(c, at.j, b, M, B);
        const double l = plant_cost_stage(C, t, C.n_x == 1 ? 0 : b, q + (size_t)at.l * row + R * nq, q + (size_t)(at.l + 1) * row + R * nq,
                                          t < C.T ? u_applied + ((size_t)at.l * NB + R) * C.nu : nullptr, work, nullptr, nullptr, team);
        J = t == 0 ? l : J + l;
    }
    return J;
}

// Why a line search over segments is refused, or null, beside plant_linesearch_refusal's tests of alpha and armijo: before any device is touched
inline const char* plant_shoot_linesearch_refusal(int n_alpha, int M, int B, int T, int n_weight, const double* weight) {
    if (const char* why = plant_shooting_refusal(T, M, B)) return why;
    if ((long long)n_alpha * M * B * (T / M + 2) > 2147483647LL) return "n_alpha M B L beyond an int";
    if (!weight) return "null defect_weight";
    if (n_weight != 1 && n_weight != B) return "n_weight neither 1 nor B";
    for (int e = 0; e < n_weight; ++e) if (!(weight[e] >= 0.0) || !std::isfinite(weight[e])) return "a defect_weight that is negative or not finite";
    return nullptr;
}

// Every pointer in the memory the team reads (device memory for the kernel).  dz T x B x (nr x n_cols) column-major; K T x B x (m x n
// column-major), k T x B x m; Q n_Q x (n x n), R n_R x (m x m), Qf, column-major; lin_q (T+1) x B x n, lin_r T x B x m; defects
// (T / seg_len - 1) x B x n.  Out: dx_nodes (T / seg_len - 1) x B x n, du T x B x m (null: not asked for), dJ B x 2.
struct PlantShootForward {
    const double* dz;
    const double *K, *k, *Q, *Qf, *R, *lin_q, *lin_r, *defects;
    double *dx_nodes, *du, *dJ;
    int B, T, nq, nu, nr, n_cols, n_Q, n_R, seg_len;
};

// dx, its successor (n each), du (m), Q dx (n), R du (m), the corner in use and the one in flight (nq x (n + m) each), dJ1, dJ2 and two of padding
PCOST_HD constexpr size_t plant_shoot_forward_work_doubles(int nq, int nu) {
    return (size_t)6 * nq + 2 * (size_t)nu + 2 * (size_t)nq * (2 * nq + nu) + 4;
}
static_assert(plant_shoot_forward_work_doubles(18, 12) * sizeof(double) == 14912, "the largest model: 14.6 KB of LDS");

template <class Team>
PCOST_HD inline void plant_shoot_forward_chain(const PlantShootForward& F, int rb, double* work, Team& team) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const int me = team.rank(), np = team.size(), nq = F.nq, n = 2 * nq, m = F.nu, B = F.B, T = F.T, nr = F.nr, nc = n + m, L = F.seg_len;
    const size_t blk = (size_t)nr * F.n_cols;
    double *x = work, *xn = x + n, *u = xn + n, *qx = u + m, *ru = qx + n;
    double* Dc[2] = {ru + m, ru + m + nq * nc};
    double* acc = Dc[1] + nq * nc;      // dJ1, dJ2
    auto block = [&](int t) { return F.dz + ((size_t)t * B + rb) * blk; };
    for (int e = me; e < n; e += np) x[e] = 0.0;
    if (me == 0) { acc[0] = 0.0; acc[1] = 0.0; }
    team.fetch_issue(block(0), nq, nc, nr);
    team.fetch_commit(Dc[0], block(0), nq, nc, nr);
    team.sync();
    for (int t = 0; t < T; ++t) {
        const double* D = Dc[t & 1];          // [D1 D2] nq x n, then Du nq x m
        const double* Du = D + nq * n;
        if (t + 1 < T) team.fetch_issue(block(t + 1), nq, nc, nr);      // in flight while step t is worked
        const size_t e0 = (size_t)t * B + rb;
        const double *Kt = F.K + e0 * m * n, *kt = F.k + e0 * m;
        const double* Qt = F.Q + (F.n_Q == 1 ? 0 : (size_t)t * n * n);
        const double* Rt = F.R + (F.n_R == 1 ? 0 : (size_t)t * m * m);
        for (int i = me; i < m; i += np) {    // du = k - K dx
            double s = 0.0;
            for (int j = 0; j < n; ++j) s = s + Kt[j * m + i] * x[j];
            const double v = kt[i] - s;
            u[i] = v;
            if (F.du) F.du[e0 * m + i] = v;
        }
        for (int i = me; i < n; i += np) {    // Q dx
            double s = 0.0;
            for (int j = 0; j < n; ++j) s = s + Qt[j * n + i] * x[j];
            qx[i] = s;
        }
        team.sync();
        for (int i = np - 1 - me; i < m; i += np) {      // R du, from the far end of the team
            double s = 0.0;
            for (int j = 0; j < m; ++j) s = s + Rt[j * m + i] * u[j];
            ru[i] = s;
        }
        const bool node = t + 1 < T && (t + 1) % L == 0;
        const double* d = node ? F.defects + ((size_t)((t + 1) / L - 1) * B + rb) * n : nullptr;
        for (int i = me; i < n; i += np) {    // dx_{t+1} = A dx + B du (+ d)
            double v;
            if (i < nq) v = x[nq + i];
            else {
                const int r = i - nq;
                double s = 0.0;
                for (int j = 0; j < n; ++j) s = s + D[j * nq + r] * x[j];
                for (int j = 0; j < m; ++j) s = s + Du[j * nq + r] * u[j];
                v = s;
            }
            if (d) v = v + d[i];
            xn[i] = v;
            if (node) F.dx_nodes[((size_t)((t + 1) / L - 1) * B + rb) * n + i] = v;
        }
        team.sync();
        if (me == 0) {                        // the stage's two terms of the quadratic model
            const double *lq = F.lin_q + e0 * n, *lr = F.lin_r + e0 * m;
            double a = 0.0, b = 0.0, c = 0.0, e = 0.0;
            for (int j = 0; j < n; ++j) a = a + lq[j] * x[j];
            for (int i = 0; i < m; ++i) b = b + lr[i] * u[i];
            acc[0] = acc[0] + (a + b);
            for (int i = 0; i < n; ++i) c = c + x[i] * qx[i];
            for (int i = 0; i < m; ++i) e = e + u[i] * ru[i];
            acc[1] = acc[1] + (0.5 * c + 0.5 * e);
        }
        team.sync();                          // the stage's terms have read dx
        for (int i = me; i < n; i += np) x[i] = xn[i];
        if (t + 1 < T) team.fetch_commit(Dc[(t + 1) & 1], block(t + 1), nq, nc, nr);
        team.sync();
    }
    for (int i = me; i < n; i += np) {        // the terminal stage
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = s + F.Qf[j * n + i] * x[j];
        qx[i] = s;
    }
    team.sync();
    if (me == 0) {
        const double* lq = F.lin_q + ((size_t)T * B + rb) * n;
        double a = 0.0, c = 0.0;
        for (int j = 0; j < n; ++j) a = a + lq[j] * x[j];
        for (int i = 0; i < n; ++i) c = c + x[i] * qx[i];
        F.dJ[2 * rb] = acc[0] + a;
        F.dJ[2 * rb + 1] = acc[1] + 0.5 * c;
    }
    team.sync();
}

// Why a forward pass is refused, or null, beside its null pointers and the tape: before any device is touched
inline const char* plant_shoot_forward_refusal(int T, int seg_len, int n_Q, int n_R) {
    if (seg_len < 1 || T % seg_len != 0) return "T not divisible by segment_len";
    if ((n_Q != 1 && n_Q != T) || (n_R != 1 && n_R != T)) return "n_Q or n_R neither 1 nor T";
    return nullptr;
}

}  // namespace cimpc
