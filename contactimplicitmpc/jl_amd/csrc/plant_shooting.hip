// Multiple shooting on the device plant (DESIGN.md sections 3, item 3l, and 5.5; plant_shooting.h): the M segments of every robot's horizon
// rolled out abreast, as M B robots for L = T / M steps where an ordinary rollout walks B robots for T.
//
//   cimpc_plant_rollout_segments   nodes (M x B x 2nq) and u (T x B x nu) up; plant_shoot_spread_kernel writes what the step kernel reads for
//                                  the M B virtual robots (their two start rows, and per step the control and disturbance rows of GLOBAL step
//                                  j L + l); the open-loop step kernel's chunks (plant_step_launch.h) for L steps; ONE sensitivity launch over
//                                  the L x M B entries, each on its own robot's rows l, l+1; plant_shoot_stitch_kernel moves blocks, status
//                                  words and the steps' outputs into (T, B) layout - the blocks into memory an ordinary cimpc_plant_tape owns -
//                                  and writes the defects and, with a cost, every stage's l_t, lin_q and lin_r; plant_shoot_total_kernel sums D
//                                  and J per robot; one read-back, one synchronize
//   cimpc_plant_shooting_cost      plant_shooting.h on the host with a team of one
//   cimpc_plant_shooting_forward   the linear forward pass at alpha = 1 over a tape's blocks with the backward pass's gains and the defects:
//                                  the weights, gains, linear terms and defects up, ONE launch of plant_shoot_forward_kernel (a workgroup of one
//                                  wavefront per robot walks t = 0 .. T-1 through plant_shoot_forward_chain, the step's nq x (2nq + nu) corner
//                                  fetched a step ahead), dx at the nodes, du and (dJ1, dJ2) down
//   cimpc_plant_shooting_linesearch  n_alpha step lengths of every segment of every robot in ONE closed-loop rollout of n_alpha M B robots for L
//                                  steps: plant_shoot_expand_kernel (the candidates' inputs: time-offset rows, gains, x_ref from the segment's
//                                  parent rows, and the shifted nodes), the closed-loop step kernel's chunks, plant_shoot_cand_cost_kernel (J on the
//                                  candidate's own segments in global order, its D, convergence), plant_shoot_gather_kernel (phi, acceptance and
//                                  choice per REAL robot, the chosen candidate's M segments compacted to M B virtual robots), ONE sensitivity
//                                  launch over the chosen L x M B entries, plant_shoot_stitch_kernel and plant_shoot_total_kernel as in the
//                                  rollout, the line search's restore kernel (plant_restore_launch: the parent's blocks for a robot without an
//                                  acceptable candidate)
//
// The kernels here move rows and run the short ordered chains of plant_shooting.h and plant_cost.h; a wavefront per workgroup.  The time of
// the call is the step kernel's, for L steps.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

// No fused multiply-adds in this translation unit: the cost and the defects round as the float64 restatement of the definition does.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_cost.h"
#include "plant_model.h"
#include "plant_rollout_call.h"
#include "plant_rollout_plan.h"
#include "plant_sensitivity.h"
#include "plant_shooting.h"
#include "plant_stage_launch.h"
#include "plant_step_launch.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

// Entry e = l (M B) + r of the virtual robots' inputs, r = j B + b: the control row of global step t = j L + l of robot b, the w row that step
// reads; at l = 0 also trajectory rows 0 and 1 from node j and mu (given per robot).
struct PlantShootSpread {
    const double *nodes, *u, *w, *mu;      // M x B x 2nq, T x B x nu, K_w x n_w x nw (null: none), B (null: shared)
    double *q, *u_out, *w_out, *mu_out;    // (L + 2) x MB x nq, L x MB x nu, L x MB x nw, MB
    int B, M, L, nq, nu, nw, K_w, n_w, hold_w;
};

__global__ __launch_bounds__(LS_THREADS) void plant_shoot_spread_kernel(PlantShootSpread S) {
    const int e = blockIdx.x, lane = threadIdx.x, MB = S.M * S.B;
    if (e >= S.L * MB) return;
    const int l = e / MB, r = e % MB, j = r / S.B, b = r % S.B, t = plant_shoot_step(j, S.L, l), nq = S.nq, nu = S.nu;
    for (int i = lane; i < nu; i += LS_THREADS) S.u_out[(size_t)e * nu + i] = S.u[((size_t)t * S.B + b) * nu + i];
    if (S.w) {
        const double* wt = rollout_schedule(S.w, t, S.hold_w, S.K_w, S.n_w, b, S.nw);
        for (int i = lane; i < S.nw; i += LS_THREADS) S.w_out[(size_t)e * S.nw + i] = wt[i];
    }
    if (l != 0) return;
    const double* node = S.nodes + (size_t)r * 2 * nq;
    for (int i = lane; i < nq; i += LS_THREADS) {
        S.q[(size_t)r * nq + i] = node[i];
        S.q[((size_t)MB + r) * nq + i] = node[nq + i];
    }
    if (S.mu && lane == 0) S.mu_out[r] = S.mu[b];
}

// Entry e = t B + b, t = 0 .. T, of the stitched rollout.  t < T: step l of segment j, virtual entry l (M B) + j B + b - its block and
// gradient status into the tape, its gamma, b, step status and iteration count into (T, B) layout.  Every t with a cost: l_t, lin_q[t] and
// lin_r[t] on the segment's own rows.  The workgroups t = 1 .. M-1 also write defect t of robot b.
struct PlantShootStitch {
    PlantCost C;                                   // C.Q null: no cost
    const double *qs, *u, *gamma, *b, *dz;         // the segments': (L + 2) x MB x nq; u T x B x nu as given; L x MB x nc, nb; L x MB blocks
    const int *status, *iters, *grad_status;
    double *Tg, *Tb, *Tdz;                         // (T, B) layout
    int *Tst, *Tit, *Tgst;
    double *defects, *lt, *lin_q, *lin_r;          // (M-1) x B x 2nq; (T+1) x B; (T+1) x B x 2nq; T x B x nu
    int B, M, T, nq, nu, nc, nb, block;
};

__global__ __launch_bounds__(LS_THREADS) void plant_shoot_stitch_kernel(PlantShootStitch S) {
    __shared__ double work[LS_MAX_WORK];
    const int e = blockIdx.x, lane = threadIdx.x, B = S.B, M = S.M, T = S.T, L = T / M, nq = S.nq, nu = S.nu;
    if (e >= (T + 1) * B) return;
    const int t = e / B, b = e % B;
    if (t < T) {
        const PlantShootRows at = plant_shoot_stage_rows(t, T, L);
        const size_t from = plant_shoot_entry(at.l, at.j, b, M, B), to = (size_t)e;
        for (int i = lane; i < S.block; i += LS_THREADS) S.Tdz[to * S.block + i] = S.dz[from * S.block + i];
        for (int i = lane; i < S.nc; i += LS_THREADS) S.Tg[to * S.nc + i] = S.gamma[from * S.nc + i];
        for (int i = lane; i < S.nb; i += LS_THREADS) S.Tb[to * S.nb + i] = S.b[from * S.nb + i];
        if (lane == 0) { S.Tst[to] = S.status[from]; S.Tit[to] = S.iters[from]; S.Tgst[to] = S.grad_status[from]; }
    }
    if (t >= 1 && t < M)
        for (int i = lane; i < 2 * nq; i += LS_THREADS) S.defects[((size_t)(t - 1) * B + b) * 2 * nq + i] = plant_shoot_defect(S.qs, M, B, L, nq, t, b, i);
    if (!S.C.Q) return;
    PlantCostWave team;
    const double l = plant_shoot_stage(S.C, M, B, t, b, S.qs, S.u, work, S.lin_q + (size_t)e * 2 * nq, t < T ? S.lin_r + (size_t)e * nu : nullptr, team);
    if (lane == 0) S.lt[e] = l;
}

// D and, with a cost, J of robot b: the two running sums of plant_shooting.h, a work item each
constexpr int SHOOT_TOTAL_THREADS = 64;
__global__ __launch_bounds__(SHOOT_TOTAL_THREADS) void plant_shoot_total_kernel(const double* defects, const double* lt, double* D, double* J, int B, int M,
                                                                                int T, int nq) {
    const int b = (int)blockIdx.x * SHOOT_TOTAL_THREADS + (int)threadIdx.x;
    if (b >= B) return;
    D[b] = plant_shoot_defect_sum(defects, M, B, nq, b);
    if (lt) J[b] = plant_shoot_total(lt, T, B, b);
}

// Entry e = l NB + R of the candidates' inputs, R = (c M + j) B + b, from the nominal's rows of robot b at global step t = j L + l (all device
// memory): the open-loop row, the gain block, the x_ref row from the segment's parent rows l, l+1, the w row; at l = 0 also the shifted node,
// mu and the limit rows.
struct PlantShootExpand {
    const double *qs_nom, *u_nom, *k, *K, *dx_nodes, *w, *mu, *alpha;      // (L+2) x MB x nq; T x B x nu; T x B x nu; T x B x (nu x 2nq); (M-1) x B x 2nq
    double *q, *u, *fb_K, *x_ref, *w_out, *mu_out;
    int B, M, L, NB, nq, nu, nw, K_w, n_w, hold_w;
    const double *u_lo, *u_hi;      // n_lim x nu, or both null
    double *lo_out, *hi_out;        // NB rows, or null (n_lim = 1)
    int n_lim;
};

__global__ __launch_bounds__(LS_THREADS) void plant_shoot_expand_kernel(PlantShootExpand E) {
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= E.L * E.NB) return;
    const int l = e / E.NB, R = e % E.NB, MB = E.M * E.B, c = R / MB, r = R % MB, j = r / E.B, b = r % E.B, nq = E.nq, nu = E.nu, kk = nu * 2 * nq;
    const size_t from = (size_t)plant_shoot_step(j, E.L, l) * E.B + b;
    const double *lo = E.u_lo ? plant_feedback_limits(E.u_lo, E.n_lim, b, nu) : nullptr, *hi = E.u_lo ? plant_feedback_limits(E.u_hi, E.n_lim, b, nu) : nullptr;
    for (int i = lane; i < nu; i += LS_THREADS) {
        const double ubar = plant_candidate_control(E.u_nom[from * nu + i], E.alpha[c], E.k[from * nu + i]);
        E.u[(size_t)e * nu + i] = lo ? plant_feedback_limit(ubar, lo[i], hi[i]) : ubar;
    }
    for (int i = lane; i < kk; i += LS_THREADS) E.fb_K[(size_t)e * kk + i] = E.K[from * kk + i];
    const double *q0 = E.qs_nom + ((size_t)l * MB + r) * nq, *q1 = E.qs_nom + ((size_t)(l + 1) * MB + r) * nq;
    for (int i = lane; i < 2 * nq; i += LS_THREADS) E.x_ref[(size_t)e * 2 * nq + i] = plant_candidate_target(q0, q1, nq, i);
    if (E.w) {
        const double* wt = rollout_schedule(E.w, plant_shoot_step(j, E.L, l), E.hold_w, E.K_w, E.n_w, b, E.nw);
        for (int i = lane; i < E.nw; i += LS_THREADS) E.w_out[(size_t)e * E.nw + i] = wt[i];
    }
    if (l != 0) return;
    const double* dx = j > 0 ? E.dx_nodes + ((size_t)(j - 1) * E.B + b) * 2 * nq : nullptr;      // node 0 is left as it stands
    for (int i = lane; i < nq; i += LS_THREADS) {
        E.q[(size_t)R * nq + i] = dx ? plant_shoot_candidate_node(q0[i], E.alpha[c], dx[i]) : q0[i];
        E.q[((size_t)E.NB + R) * nq + i] = dx ? plant_shoot_candidate_node(q1[i], E.alpha[c], dx[nq + i]) : q1[i];
    }
    if (E.mu && lane == 0) E.mu_out[R] = E.mu[b];
    if (E.lo_out)
        for (int i = lane; i < nu; i += LS_THREADS) { E.lo_out[(size_t)R * nu + i] = lo[i]; E.hi_out[(size_t)R * nu + i] = hi[i]; }
}

// J, D and convergence of candidate c of robot b, a workgroup each: the chains of plant_shooting.h on the candidates' rollout
struct PlantShootCandCost {
    PlantCost C;
    const double *q, *u_applied;      // (L+2) x NB x nq, L x NB x nu
    const int* status;                // L x NB
    double *J, *D;                    // n_alpha x B each
    int* conv;
    int B, M, NB, n_alpha;
};

__global__ __launch_bounds__(LS_THREADS) void plant_shoot_cand_cost_kernel(PlantShootCandCost P) {
    __shared__ double work[LS_MAX_WORK];
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= P.n_alpha * P.B) return;
    const int c = e / P.B, b = e % P.B, M = P.M, L = P.C.T / M;
    PlantCostWave team;
    const double J = plant_shoot_candidate_cost(P.C, M, P.B, P.NB, c, b, P.q, P.u_applied, work, team);
    int all = 1;
    for (int s = lane; s < P.C.T; s += LS_THREADS) all &= P.status[(size_t)(s % L) * P.NB + plant_shoot_candidate_robot(c, s / L, b, M, P.B)] != 0;
    all = __syncthreads_and(all);
    if (lane == 0) { P.J[e] = J; P.D[e] = plant_shoot_candidate_defect_sum(P.q, M, P.B, P.NB, L, P.C.nq, c, b); P.conv[e] = all; }
}

// Row l (0 .. L+1) of virtual robot r = j B + b of robot b's chosen candidate, compacted to M B robots; every workgroup of a robot finds the
// choice again (n_alpha <= 64 tests), the one of row 0 and segment 0 stores it with phi and the acceptability flags.
struct PlantShootGather {
    const double *q, *z, *u_applied, *gamma, *b, *w;      // the candidates': NB robots
    const int *status, *iters, *conv;
    const double *J, *D, *phi_nom, *D_nom, *dJ, *alpha, *weight;
    double armijo;
    int n_alpha, n_weight;
    double* phi;
    int *ok, *choice;
    double *Cq, *Cz, *Cu, *Cu_steps, *Cg, *Cb, *Cw, *Cmu;      // the chosen: M B virtual robots; Cu_steps T x B x nu in global layout
    const double* mu;
    int *Cst, *Cit;
    int B, M, L, NB, nq, nu, nc, nb, nz, nw;
};

__global__ __launch_bounds__(LS_THREADS) void plant_shoot_gather_kernel(PlantShootGather G) {
    __shared__ int s_ok[PLANT_LS_MAX_ALPHA];
    __shared__ double s_phi[PLANT_LS_MAX_ALPHA];
    const int e = blockIdx.x, lane = threadIdx.x, B = G.B, M = G.M, L = G.L, MB = M * B;
    if (e >= (L + 2) * MB) return;
    const int l = e / MB, r = e % MB, j = r / B, b = r % B, nq = G.nq, nu = G.nu;
    const double weight = G.weight[G.n_weight == 1 ? 0 : b];
    for (int c = lane; c < G.n_alpha; c += LS_THREADS) {
        const double phi = plant_shoot_merit(G.J[c * B + b], weight, G.D[c * B + b]);
        s_phi[c] = phi;
        s_ok[c] = plant_shoot_acceptable(G.conv[c * B + b] != 0, phi, G.phi_nom[b], G.armijo, G.alpha[c], G.dJ[2 * b], G.dJ[2 * b + 1], weight, G.D_nom[b]) ? 1 : 0;
    }
    __syncthreads();
    const int choice = plant_linesearch_choice(s_phi, 1, s_ok, 1, G.n_alpha);
    if (l == 0 && j == 0) {
        for (int c = lane; c < G.n_alpha; c += LS_THREADS) { G.ok[c * B + b] = s_ok[c]; G.phi[c * B + b] = s_phi[c]; }
        if (lane == 0) G.choice[b] = choice;
    }
    const int R = plant_shoot_candidate_robot(choice < 0 ? 0 : choice, j, b, M, B);
    const size_t from = (size_t)l * G.NB + R, to = (size_t)l * MB + r;
    for (int i = lane; i < nq; i += LS_THREADS) G.Cq[to * nq + i] = G.q[from * nq + i];
    if (l == 0 && G.Cmu && lane == 0) G.Cmu[r] = G.mu[b];
    if (l >= L) return;
    const size_t step = (size_t)plant_shoot_step(j, L, l) * B + b;
    for (int i = lane; i < G.nz; i += LS_THREADS) G.Cz[to * G.nz + i] = G.z[from * G.nz + i];
    for (int i = lane; i < nu; i += LS_THREADS) { const double v = G.u_applied[from * nu + i]; G.Cu[to * nu + i] = v; G.Cu_steps[step * nu + i] = v; }
    for (int i = lane; i < G.nc; i += LS_THREADS) G.Cg[to * G.nc + i] = G.gamma[from * G.nc + i];
    for (int i = lane; i < G.nb; i += LS_THREADS) G.Cb[to * G.nb + i] = G.b[from * G.nb + i];
    if (G.w) for (int i = lane; i < G.nw; i += LS_THREADS) G.Cw[to * G.nw + i] = G.w[from * G.nw + i];
    if (lane == 0) { G.Cst[to] = G.status[from]; G.Cit[to] = G.iters[from]; }
}

// the wavefront as the team of plant_shoot_forward_chain: the corner of the step ahead rides in registers while a step is worked
constexpr int SHOOT_FWD_STAGE = 16;      // per lane: a corner of up to 1024 doubles (18 x 48 = 864 at the largest model) is wholly in flight
using PlantShootWave = PlantCornerTeam<LS_THREADS, SHOOT_FWD_STAGE>;

constexpr int SHOOT_FWD_MAX_WORK = (int)plant_shoot_forward_work_doubles(PLANT_MAX_Q, PLANT_MAX_U);
__global__ __launch_bounds__(LS_THREADS) void plant_shoot_forward_kernel(PlantShootForward F) {
    __shared__ double work[SHOOT_FWD_MAX_WORK];
    const int rb = blockIdx.x;
    if (rb >= F.B) return;      // uniform over the workgroup
    PlantShootWave team;
    plant_shoot_forward_chain(F, rb, work, team);
}

namespace {
// the entries' own buffers, beside the segments' rollout in the plant workspace: the B-robot inputs, the stitched outputs, the integer outputs
PlantStageWs g_shooting_ws[PLANT_MAX_DEVICES];

// Why the rollout arguments of cimpc_plant_rollout_segments are refused, or null: the tests of plant_rollout_check (plant_rollout_call.h) on
// the arguments the entry shares with cimpc_plant_rollout_tape, each with its reason, in that function's order.
const char* shoot_call_refusal(int model, int B, int n_terrain, const cimpc_terrain* terrain, const double* w, int K_w, int n_w, int hold_w, int n_mu,
                               double h, const cimpc_ip_opts* opts, double reg, int n_cols) {
    if ((n_terrain != 0) != (terrain != nullptr)) return "terrain and n_terrain do not go together";
    if (!(h > 0.0)) return "h not positive";
    if (n_mu != 1 && n_mu != B) return "n_mu neither 1 nor B";
    if (w && (K_w < 1 || hold_w < 1 || (n_w != 1 && n_w != B))) return "K_w or hold_w below 1, or n_w neither 1 nor B";
    PlantModel M{};
    bool rough = false;
    if (!plant_model_and_ground(model, B, n_terrain, terrain, &M, &rough)) return "n_terrain neither 1 nor B, a terrain the model does not take, or a model that needs one";
    const cimpc_ip_opts& o = *opts;
    if (o.max_iter <= 0 || o.max_ls < 0 || !(o.r_tol > 0.0) || !(o.kappa_tol > 0.0) || !(o.ls_scale > 0.0 && o.ls_scale < 1.0)) return "interior-point options out of range";
    if (!std::isfinite(reg) || reg < 0.0) return "reg negative or not finite";
    if (n_cols < 2 * M.nq + M.nu || n_cols > M.nth()) return "n_cols outside 2 nq + nu .. ntheta";
    if (!plant_sensitivity_fits(M.nz(), n_cols)) return "a block too large for the sensitivity kernel";
    return nullptr;
}
}  // namespace

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int cimpc_plant_shooting_cost(int nq, int nu, int B, int T, int segments, const cimpc_tracking_cost* cost, const double* qs, const double* u,
                                         double* J, double* D, double* defects, double* lin_q, double* lin_r) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_shooting_cost", why); };
    if (!cost || !qs || !u || !J || !D) return refuse("a null cost, qs, u, J or D");
    if (nq < 1 || nu < 1) return refuse("nq or nu below 1");
    if (const char* why = plant_shooting_refusal(T, segments, B)) return refuse(why);
    const PlantCost C = plant_cost_of(*cost, T, nq, nu);
    if (const char* why = plant_cost_pointers(C)) return refuse(why);
    if (const char* why = plant_cost_sizes(C, B)) return refuse(why);
    const int M = segments, L = T / M;
    std::vector<double> work(plant_cost_work_doubles(nq, nu)), d((size_t)(M > 1 ? M - 1 : 0) * B * 2 * nq);
    PlantCostSolo team;
    for (int j = 1; j < M; ++j)
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < 2 * nq; ++i) d[((size_t)(j - 1) * B + b) * 2 * nq + i] = plant_shoot_defect(qs, M, B, L, nq, j, b, i);
    for (int b = 0; b < B; ++b) {
        J[b] = plant_shoot_cost(C, M, B, b, qs, u, work.data(), lin_q, lin_r, team);
        D[b] = plant_shoot_defect_sum(d.data(), M, B, nq, b);
    }
    if (defects) for (size_t e = 0; e < d.size(); ++e) defects[e] = d[e];
    return CIMPC_OK;
}

extern "C" int cimpc_plant_shooting_forward(cimpc_plant_tape tape, int n_Q, const double* Q, const double* Qf, int n_R, const double* R, const double* lin_q,
                                            const double* lin_r, const double* K, const double* k, int segment_len, const double* defects,
                                            double* dx_nodes, double* du, double* dJ) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_shooting_forward", why); };
    const PlantRequired required[] = {{"tape", tape}, {"Q", Q}, {"Qf", Qf}, {"R", R}, {"lin_q", lin_q}, {"lin_r", lin_r}, {"K", K}, {"k", k},
                                      {"defects", defects}, {"dx_nodes", dx_nodes}, {"dJ", dJ}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
    const PlantTapeBuffers& buf = tape->buf;
    const int B = tape->B, T = tape->T, n_cols = tape->n_cols;
    if (B < 1 || T < 1 || buf.device < 0 || buf.device >= PLANT_MAX_DEVICES || !buf.d_dz || !buf.d_status) return refuse("a closed tape");
    if (const char* why = plant_shoot_forward_refusal(T, segment_len, n_Q, n_R)) return refuse(why);
    const PlantModel& Mo = buf.M;
    const int nq = Mo.nq, nu = Mo.nu, nr = nq + Mo.nc + Mo.nb(), M = T / segment_len;
    if (nu < 1 || n_cols < 2 * nq + nu || nq > PLANT_MAX_Q || nu > PLANT_MAX_U) return refuse("a model without controls, or a tape without the control columns");
    const size_t n = (size_t)2 * nq, m = (size_t)nu, TB = (size_t)T * B;
    PlantCursor at;
    const PlantSpan i_Q = at.take((size_t)n_Q * n * n), i_Qf = at.take(n * n), i_R = at.take((size_t)n_R * m * m), i_lq = at.take((size_t)(T + 1) * B * n),
                    i_lr = at.take(TB * m), i_K = at.take(TB * m * n), i_k = at.take(TB * m), i_d = at.take((size_t)(M - 1) * B * n);
    const size_t n_in = at.end();
    const PlantSpan o_x = at.take(i_d.n), o_u = at.take(TB * m), o_J = at.take((size_t)2 * B);
    const size_t n_out = at.end();
    if (!plant_all_finite(K, i_K.n) || !plant_all_finite(k, i_k.n)) return refuse("a non-finite entry of K or k");
    if (!plant_all_finite(defects, i_d.n)) return refuse("a non-finite entry of defects");
    PlantDeviceScope scope(buf.device);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok_ = false;
    PlantWs* ws = plant_ws_open(buf.device);
    PlantStageWs& S = g_shooting_ws[buf.device];
    if (ws && S.grow(n_in, n_out, 0)) {
        hipStream_t st = ws->st;
        ok_ = true;
        PlantStreamCopier copy{{st}, ok_};
        double *I = S.d_in, *O = S.d_out;
        copy.up(I, i_Q, Q); copy.up(I, i_Qf, Qf); copy.up(I, i_R, R); copy.up(I, i_lq, lin_q);
        copy.up(I, i_lr, lin_r); copy.up(I, i_K, K); copy.up(I, i_k, k); copy.up(I, i_d, defects);
        if (ok_) {
            const PlantShootForward F{buf.d_dz, i_K.on(I), i_k.on(I), i_Q.on(I), i_Qf.on(I), i_R.on(I), i_lq.on(I), i_lr.on(I), i_d.on(I), o_x.on(O), o_u.on(O),
                                      o_J.on(O), B, T, nq, nu, nr, n_cols, n_Q, n_R, segment_len};
            hipLaunchKernelGGL(plant_shoot_forward_kernel, dim3(B), dim3(LS_THREADS), 0, st, F);
            ok_ = hipGetLastError() == hipSuccess;
        }
        copy.down(dx_nodes, O, o_x); copy.down(dJ, O, o_J);
        copy.down(du, O, o_u);      // where it is asked for
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
    }
    return scope.leave(ok_) ? CIMPC_OK : CIMPC_ERR_HIP;
}

extern "C" int cimpc_plant_rollout_segments(int model, int B, int T, int segments, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                            const double* nodes, const double* u, const double* w, int K_w, int n_w, int hold_w, const double* mu,
                                            int n_mu, double h, const cimpc_ip_opts* opts, const cimpc_tracking_cost* cost, double reg, int n_cols,
                                            double* qs, double* gamma, double* b, int* status, int* iters, double* defects, double* D, double* J,
                                            double* lin_q, double* lin_r, int* grad_status, cimpc_plant_tape* tape) {
    using namespace cimpc;
    // every refusal leaves its reason where cimpc_last_error(NULL) finds it, before any device is touched
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_rollout_segments", why); };
    if (!tape) return refuse("null tape");
    *tape = nullptr;
    const PlantRequired required[] = {{"nodes", nodes}, {"u", u}, {"mu", mu}, {"opts", opts}, {"qs", qs}, {"gamma", gamma}, {"b", b},
                                      {"status", status}, {"iters", iters}, {"defects", defects}, {"D", D}, {"grad_status", grad_status}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
    if (cost && (!J || !lin_q || !lin_r)) return refuse("a cost without J, lin_q or lin_r");
    if (const char* why = plant_shooting_refusal(T, segments, B)) return refuse(why);
    {      // the nodes, by the model's nq from its id alone, before anything else reads the call
        PlantModel named{};
        if (!plant_model_by_id(model, &named)) return refuse("an unknown model");
        if (named.nu < 1) return refuse("a model without controls");
        if (const char* why = plant_shooting_nodes_refusal(nodes, segments, B, named.nq)) return refuse(why);
    }
    if (const char* why = shoot_call_refusal(model, B, n_terrain, terrain, w, K_w, n_w, hold_w, n_mu, h, opts, reg, n_cols)) return refuse(why);
    // everything cimpc_plant_rollout_tape validates for the B robots over T steps, on the arrays that stand in for its arguments: the reasons
    // above restate its tests one by one, and this call stands behind them so that nothing it refuses gets through unnamed
    const PlantRolloutCall real{.model = model, .B = B, .T = T, .steps_per_launch = steps_per_launch, .n_terrain = n_terrain, .terrain = terrain,
                                .q0 = nodes, .q1 = nodes, .u = {u, T, B, 1}, .w = {w, K_w, n_w, hold_w}, .mu = mu, .n_mu = n_mu, .h = h, .opts = opts,
                                .q = qs, .gamma = gamma, .b = b, .status = status, .iters = iters,
                                .grad = PlantRolloutGrad{reg, n_cols, nullptr, nullptr, grad_status, true}};
    PlantModel Mo{};
    bool rough = false;
    if (plant_rollout_check(real, &Mo, &rough) != CIMPC_OK) return refuse("an argument that cimpc_plant_rollout_tape refuses for B robots over T steps");
    const int M = segments, L = T / M, MB = M * B, nq = Mo.nq, nu = Mo.nu, nc = Mo.nc, nb = Mo.nb(), nw = Mo.nw, nr = nq + nc + nb;
    PlantCost C{};
    if (cost) {
        C = plant_cost_of(*cost, T, nq, nu);
        if (const char* why = plant_cost_pointers(C)) return refuse(why);
        if (const char* why = plant_cost_sizes(C, B)) return refuse(why);
    }
    const bool has_w = w != nullptr, mu_each = n_mu != 1, ter_each = rough && n_terrain != 1;
    // the segments' rollout in the plant workspace, laid out as a gradient call of M B robots over L steps lays itself out: controls and
    // disturbances one row per step and virtual robot, hold 1
    const PlantRolloutCall virt{.model = model, .B = MB, .T = L, .steps_per_launch = steps_per_launch, .n_terrain = 0, .terrain = nullptr, .q0 = nodes,
                                .q1 = nodes, .u = {u, L, MB, 1}, .w = {w, L, MB, 1}, .mu = mu, .n_mu = mu_each ? MB : 1, .h = h, .opts = opts, .q = qs,
                                .gamma = gamma, .b = b, .status = status, .iters = iters,
                                .grad = PlantRolloutGrad{reg, n_cols, nullptr, qs, grad_status, false}};
    const PlantRolloutLayout Lo = plant_rollout_layout(Mo, virt);
    const size_t TB = (size_t)T * B, block = (size_t)nr * n_cols;
    const int n_ter = !rough ? 0 : ter_each ? MB : 1;
    std::vector<cimpc_terrain> ter;      // the virtual robots' terrains: robot b's for every segment
    if (ter_each) for (int j = 0; j < M; ++j) ter.insert(ter.end(), terrain, terrain + B);
    // the B-robot inputs in d_in, the stitched outputs in d_out, the integers in d_int
    const PlantSegmentsLayout Y = plant_segments_layout(Mo, C, PlantSegmentsShape{B, T, M, K_w, n_w, has_w, mu_each, cost != nullptr});

    int dev = 0;
    if (!plant_current_device(&dev)) return CIMPC_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lock(g_plant_mu);
    bool ok_ = false;
    PlantTapeBuffers buf;
    PlantWs* ws = plant_ws_open(dev);
    PlantStageWs& S = g_shooting_ws[dev];
    if (ws && plant_grow(&ws->d_in, &ws->cap_in, Lo.need_in) && plant_grow(&ws->d_out, &ws->cap_out, Lo.need_out) && plant_grow(&ws->d_st, &ws->cap_st, Lo.need_st) &&
        plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)n_ter) && plant_grow(&ws->d_z, &ws->cap_z, Lo.need_z) && plant_grow(&ws->d_grad, &ws->cap_grad, Lo.need_grad) &&
        plant_grow(&ws->d_grad_st, &ws->cap_grad_st, Lo.need_grad_st) && S.grow(Y.need_in, Y.need_out, Y.need_int) && hipMalloc((void**)&buf.d_dz, TB * block * sizeof(double)) == hipSuccess) {      // the tape's memory, the last
        if (hipMalloc((void**)&buf.d_status, TB * sizeof(int)) != hipSuccess) buf.d_status = nullptr;
        buf.device = dev; buf.M = Mo;
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        ok_ = buf.d_status != nullptr;
        PlantStreamCopier copy{{st}, ok_};
        double *I = S.d_in, *O = S.d_out;
        int* N = S.d_int;
        copy.up(I, Y.nodes, nodes); copy.up(I, Y.u, u);
        copy.up(I, Y.w, w); copy.up(I, Y.mu, mu);      // w where it is given, mu where it is per robot
        if (rough) copy.up(W.d_ter, PlantSpan{0, (size_t)n_ter}, ter_each ? ter.data() : terrain);
        if (cost) C = plant_cost_up(copy, I, Y.cost, C);
        double *dq = W.d_in + Lo.q.at, *du = W.d_in + Lo.u.at, *dw = W.d_in + Lo.w.at, *dmu = W.d_in + Lo.mu.at;
        double *dg = W.d_out + Lo.gamma.at, *db = W.d_out + Lo.b.at, *d_dz = W.d_grad + Lo.dz.at;
        int *d_st = W.d_st + Lo.status.at, *d_it = W.d_st + Lo.iters.at, *d_gst = W.d_grad_st + Lo.grad_status.at;
        if (ok_) {
            const PlantShootSpread Sp{Y.nodes.on(I), Y.u.on(I), Y.w.or_null(I), Y.mu.or_null(I), dq, du, dw, dmu, B, M, L, nq, nu, nw,
                                      has_w ? K_w : 1, has_w ? n_w : 1, has_w ? hold_w : 1};
            hipLaunchKernelGGL(plant_shoot_spread_kernel, dim3((unsigned)TB), dim3(LS_THREADS), 0, st, Sp);
            ok_ = hipGetLastError() == hipSuccess;
        }
        const PlantStepArrays R{dq, du, has_w ? dw : nullptr, mu_each ? dmu : nullptr, dg, db, d_st, d_it, mu[0], h, L, MB, 1, has_w ? L : 1, has_w ? MB : 1, 1,
                                mu_each ? MB : 1, W.d_z, PlantFeedback{}, nullptr, nullptr};
        ok_ = ok_ && plant_step_chunks(Mo, rough, *opts, MB, L, steps_per_launch, R, rough ? W.d_ter : nullptr, n_ter, st);
        if (ok_) {      // every step's gradients on its own virtual robot's rows l, l+1
            const PlantSensSource src{W.d_z, nullptr, dq, du, R.w, R.mu, d_st, R.mu0, h, MB, L, MB, 1, R.K_w, R.n_w, 1, R.n_mu};
            ok_ = plant_sensitivity_launch(Mo, (int)TB, src, rough ? W.d_ter : nullptr, n_ter, reg, n_cols, d_dz, d_gst, st);
        }
        if (ok_) {
            const PlantShootStitch Ss{C, dq, Y.u.on(I), dg, db, d_dz, d_st, d_it, d_gst, Y.gamma.on(O), Y.b.on(O), buf.d_dz, Y.status.on(N), Y.iters.on(N),
                                      buf.d_status, Y.defects.on(O), Y.lt.on(O), Y.lin_q.on(O), Y.lin_r.on(O), B, M, T, nq, nu, nc, nb, (int)block};
            hipLaunchKernelGGL(plant_shoot_stitch_kernel, dim3((unsigned)((T + 1) * B)), dim3(LS_THREADS), 0, st, Ss);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {
            hipLaunchKernelGGL(plant_shoot_total_kernel, dim3((unsigned)((B + SHOOT_TOTAL_THREADS - 1) / SHOOT_TOTAL_THREADS)), dim3(SHOOT_TOTAL_THREADS), 0, st,
                               (const double*)Y.defects.on(O), cost ? (const double*)Y.lt.on(O) : nullptr, Y.D.on(O), Y.J.on(O), B, M, T, nq);
            ok_ = hipGetLastError() == hipSuccess;
        }
        copy.down(qs, W.d_in, Lo.q); copy.down(gamma, O, Y.gamma); copy.down(b, O, Y.b); copy.down(status, N, Y.status);
        copy.down(iters, N, Y.iters); copy.down(D, O, Y.D); copy.down(grad_status, buf.d_status, PlantSpan{0, TB});
        copy.down(defects, O, Y.defects);      // none with one segment
        if (cost) { copy.down(J, O, Y.J); copy.down(lin_q, O, Y.lin_q); copy.down(lin_r, O, Y.lin_r); }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
    }
    if (!ok_) { (void)buf.release(); return CIMPC_ERR_HIP; }
    *tape = new cimpc_plant_tape_s{buf, model, B, T, n_cols};
    return CIMPC_OK;
}

// The line search of a multiple-shooting iteration (plant_shooting.h: THE CANDIDATE LAW, ACCEPTANCE).  `tape` is the
// parent: the stitched tape of the nominal qs_nom ((L+2) x MB x nq), whose steps applied u_nom (T x B x nu); K, k the gains of
// cimpc_plant_tape_lqr_shooting, dx_nodes and dJ those of cimpc_plant_shooting_forward (with one segment: no node, dJ = dV).
extern "C" int cimpc_plant_shooting_linesearch(cimpc_plant_tape tape, int segments, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                               const double* qs_nom, const double* u_nom, const double* w, int K_w, int n_w, int hold_w, const double* mu,
                                               int n_mu, double h, const cimpc_ip_opts* opts, const double* K, const double* k, const double* dx_nodes,
                                               const double* dJ, const double* phi_nom, const double* D_nom, int n_weight, const double* weight,
                                               int n_alpha, const double* alpha, double armijo, const cimpc_tracking_cost* cost, double reg, double* J,
                                               double* D_cand, double* phi, int* ok, int* choice, double* qs, double* u_applied, double* gamma, double* b,
                                               int* status, int* iters, double* defects, double* D, double* J_chosen, double* lin_q, double* lin_r,
                                               int* grad_status, cimpc_plant_tape* new_tape, int n_lim, const double* u_lo, const double* u_hi) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_shooting_linesearch", why); };
    if (!new_tape) return refuse("null new_tape");
    *new_tape = nullptr;
    const PlantRequired required[] = {
        {"tape", tape}, {"qs_nom", qs_nom}, {"u_nom", u_nom}, {"mu", mu}, {"opts", opts}, {"K", K}, {"k", k}, {"dx_nodes", dx_nodes}, {"dJ", dJ}, {"phi_nom", phi_nom},
        {"D_nom", D_nom}, {"alpha", alpha}, {"cost", cost}, {"J", J}, {"D_cand", D_cand}, {"phi", phi}, {"ok", ok}, {"choice", choice}, {"qs", qs},
        {"u_applied", u_applied}, {"gamma", gamma}, {"b", b}, {"status", status}, {"iters", iters}, {"defects", defects}, {"D", D}, {"J_chosen", J_chosen},
        {"lin_q", lin_q}, {"lin_r", lin_r}, {"grad_status", grad_status}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
    if (const char* why = plant_linesearch_refusal(n_alpha, alpha, armijo)) return refuse(why);
    const PlantTapeBuffers& parent = tape->buf;
    const int B = tape->B, T = tape->T, n_cols = tape->n_cols, model = tape->model;
    if (parent.device < 0 || parent.device >= PLANT_MAX_DEVICES || !parent.d_dz || !parent.d_status) return refuse("a closed tape");
    if (const char* why = plant_shoot_linesearch_refusal(n_alpha, segments, B, T, n_weight, weight)) return refuse(why);
    if (const char* why = shoot_call_refusal(model, B, n_terrain, terrain, w, K_w, n_w, hold_w, n_mu, h, opts, reg, n_cols)) return refuse(why);
    const bool limits = u_lo || u_hi;
    if (limits && (!u_lo || !u_hi)) return refuse("one of u_lo, u_hi without the other");
    if (limits && n_lim != 1 && n_lim != B) return refuse("n_lim neither 1 nor B");
    const PlantModel& Mo = parent.M;
    const int M = segments, L = T / M, MB = M * B, NB = n_alpha * MB, nq = Mo.nq, nu = Mo.nu, nc = Mo.nc, nb = Mo.nb(), nz = Mo.nz(), nw = Mo.nw, nr = nq + nc + nb;
    if (nu < 1 || 2 * nq > nz) return refuse("a model without controls");
    if (limits)
        for (size_t e = 0; e < (size_t)n_lim * nu; ++e) {
            if (u_lo[e] != u_lo[e] || u_hi[e] != u_hi[e]) return refuse("a NaN limit");
            if (u_lo[e] > u_hi[e]) return refuse("u_lo above u_hi");
        }
    PlantModel Mc{};
    bool rough = false;
    if (!plant_model_and_ground(model, B, n_terrain, terrain, &Mc, &rough)) return refuse("a terrain the model does not take");
    PlantCost C = plant_cost_of(*cost, T, nq, nu);
    if (const char* why = plant_cost_pointers(C)) return refuse(why);
    if (const char* why = plant_cost_sizes(C, B)) return refuse(why);
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, kk = (size_t)nu * n, block = (size_t)nr * n_cols, n_def = (size_t)(M - 1) * B * n, n_qs = (size_t)(L + 2) * MB * nq;
    if (!plant_all_finite(K, TB * kk) || !plant_all_finite(k, TB * nu)) return refuse("a non-finite entry of K or k");
    if (!plant_all_finite(qs_nom, n_qs) || !plant_all_finite(u_nom, TB * nu)) return refuse("a non-finite entry of qs_nom or u_nom");
    if (!plant_all_finite(dx_nodes, n_def)) return refuse("a non-finite entry of dx_nodes");
    const bool has_w = w != nullptr, mu_each = n_mu != 1, lim_each = limits && n_lim != 1, ter_each = rough && n_terrain != 1;
    // the candidates' rollout in the plant workspace, laid out as a closed-loop tape call of NB robots over L steps lays itself out
    const cimpc_feedback fb_shape{qs_nom, qs_nom, L, NB, 1, 1.0};      // only the shape is read
    const PlantRolloutCall cand{.model = model, .B = NB, .T = L, .steps_per_launch = steps_per_launch, .n_terrain = 0, .terrain = nullptr, .q0 = qs_nom,
                                .q1 = qs_nom, .u = {u_nom, L, NB, 1}, .w = {w, L, NB, 1}, .mu = mu, .n_mu = mu_each ? NB : 1, .h = h, .opts = opts, .q = qs,
                                .gamma = gamma, .b = b, .status = status, .iters = iters, .grad = PlantRolloutGrad{reg, n_cols, nullptr, nullptr, grad_status, true},
                                .loop = PlantRolloutLoop{&fb_shape, u_applied, nullptr, u_lo, u_hi, lim_each ? NB : 1}};
    const PlantRolloutLayout Lo = plant_rollout_layout(Mo, cand);
    const int n_ter = !rough ? 0 : ter_each ? NB : 1;
    std::vector<cimpc_terrain> ter;      // the candidates' terrains: robot b's for every (c, j)
    if (ter_each) for (int cj = 0; cj < n_alpha * M; ++cj) ter.insert(ter.end(), terrain, terrain + B);
    const size_t nA = (size_t)n_alpha * B;
    // the B-robot inputs in d_in, in the order they go up
    PlantCursor at;
    const PlantSpan i_q = at.take(n_qs), i_u = at.take(TB * nu), i_k = at.take(TB * nu), i_K = at.take(TB * kk), i_dx = at.take(n_def),
                    i_w = at.take(has_w ? (size_t)K_w * n_w * nw : 0), i_mu = at.take(mu_each ? (size_t)B : 0), i_dJ = at.take((size_t)2 * B), i_pn = at.take((size_t)B),
                    i_Dn = at.take((size_t)B), i_al = at.take((size_t)n_alpha), i_wt = at.take((size_t)n_weight);
    const PlantCostSpans i_cost = plant_cost_spans(at, C);
    const PlantSpan i_lo = at.take(limits ? (size_t)n_lim * nu : 0), i_hi = at.take(limits ? (size_t)n_lim * nu : 0);
    const size_t n_in = at.end();
    // d_out: the candidates' J, D, phi | the chosen segments as M B virtual robots | the stitched outputs
    const PlantSpan o_J = at.take(nA), o_Dc = at.take(nA), o_phi = at.take(nA), o_q = at.take(n_qs), o_z = at.take(TB * nz), o_u = at.take(TB * nu), o_us = at.take(TB * nu),
                    o_gv = at.take(TB * nc), o_bv = at.take(TB * nb), o_w = at.take(has_w ? TB * nw : 0), o_mu = at.take(mu_each ? (size_t)MB : 0), o_g = at.take(TB * nc),
                    o_b = at.take(TB * nb), o_def = at.take(n_def), o_D = at.take((size_t)B), o_Jn = at.take((size_t)B), o_lt = at.take((size_t)(T + 1) * B),
                    o_lq = at.take((size_t)(T + 1) * B * n), o_lr = at.take(TB * nu);
    const size_t n_out = at.end();
    const PlantSpan j_ok = at.take(nA), j_ch = at.take((size_t)B), j_conv = at.take(nA), j_stv = at.take(TB), j_itv = at.take(TB), j_st = at.take(TB), j_it = at.take(TB);
    const size_t n_int = at.end();

    const int dev = parent.device;
    PlantDeviceScope scope(dev);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok_ = false;
    PlantTapeBuffers buf;
    PlantWs* ws = plant_ws_open(dev);
    PlantStageWs& S = g_shooting_ws[dev];
    if (ws && plant_grow(&ws->d_in, &ws->cap_in, Lo.need_in) && plant_grow(&ws->d_out, &ws->cap_out, Lo.need_out) && plant_grow(&ws->d_st, &ws->cap_st, Lo.need_st) &&
        plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)n_ter) && plant_grow(&ws->d_z, &ws->cap_z, Lo.need_z) && plant_grow(&ws->d_fb, &ws->cap_fb, Lo.need_fb) &&
        plant_grow(&ws->d_grad, &ws->cap_grad, TB * block) && plant_grow(&ws->d_grad_st, &ws->cap_grad_st, TB) && S.grow(n_in, n_out, n_int) &&
        hipMalloc((void**)&buf.d_dz, TB * block * sizeof(double)) == hipSuccess) {      // the new tape's memory, the last to be allocated
        if (hipMalloc((void**)&buf.d_status, TB * sizeof(int)) != hipSuccess) buf.d_status = nullptr;
        buf.device = dev; buf.M = Mo;
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        ok_ = buf.d_status != nullptr;
        PlantStreamCopier copy{{st}, ok_};
        double *I = S.d_in, *O = S.d_out;
        int* N = S.d_int;
        copy.up(I, i_q, qs_nom); copy.up(I, i_u, u_nom); copy.up(I, i_k, k); copy.up(I, i_K, K); copy.up(I, i_dx, dx_nodes);
        copy.up(I, i_w, w); copy.up(I, i_mu, mu);      // w where it is given, mu where it is per robot
        copy.up(I, i_dJ, dJ); copy.up(I, i_pn, phi_nom); copy.up(I, i_Dn, D_nom); copy.up(I, i_al, alpha);
        copy.up(I, i_wt, weight);
        C = plant_cost_up(copy, I, i_cost, C);
        copy.up(I, i_lo, u_lo); copy.up(I, i_hi, u_hi);
        if (rough) copy.up(W.d_ter, PlantSpan{0, (size_t)n_ter}, ter_each ? ter.data() : terrain);
        double *dq = W.d_in + Lo.q.at, *du = W.d_in + Lo.u.at, *dw = W.d_in + Lo.w.at, *dmu = W.d_in + Lo.mu.at;
        double *d_fk = W.d_fb + Lo.fb_K.at, *d_fx = W.d_fb + Lo.x_ref.at, *d_ua = W.d_fb + Lo.u_applied.at, *d_fe = W.d_fb + Lo.fb_err.at;
        double *dg = W.d_out + Lo.gamma.at, *db = W.d_out + Lo.b.at;
        int *d_st = W.d_st + Lo.status.at, *d_it = W.d_st + Lo.iters.at;
        const double *c_lo = !limits ? nullptr : lim_each ? W.d_fb + Lo.u_lo.at : i_lo.on(I), *c_hi = !limits ? nullptr : lim_each ? W.d_fb + Lo.u_hi.at : i_hi.on(I);
        if (ok_) {
            const PlantShootExpand E{i_q.on(I), i_u.on(I), i_k.on(I), i_K.on(I), i_dx.on(I), i_w.or_null(I), i_mu.or_null(I), i_al.on(I),
                                     dq, du, d_fk, d_fx, dw, dmu, B, M, L, NB, nq, nu, nw, has_w ? K_w : 1, has_w ? n_w : 1, has_w ? hold_w : 1,
                                     i_lo.or_null(I), i_hi.or_null(I), lim_each ? W.d_fb + Lo.u_lo.at : nullptr,
                                     lim_each ? W.d_fb + Lo.u_hi.at : nullptr, n_lim};
            hipLaunchKernelGGL(plant_shoot_expand_kernel, dim3((unsigned)(L * NB)), dim3(LS_THREADS), 0, st, E);
            ok_ = hipGetLastError() == hipSuccess;
        }
        const PlantStepArrays R{dq, du, has_w ? dw : nullptr, mu_each ? dmu : nullptr, dg, db, d_st, d_it, mu[0], h, L, NB, 1, has_w ? L : 1, has_w ? NB : 1, 1,
                                mu_each ? NB : 1, W.d_z, PlantFeedback{d_fk, d_fx, L, NB, 1, 1.0}, d_ua, d_fe, PlantFeedbackLimits{c_lo, c_hi, lim_each ? NB : 1}};
        ok_ = ok_ && plant_step_chunks(Mo, rough, *opts, NB, L, steps_per_launch, R, rough ? W.d_ter : nullptr, n_ter, st);
        if (ok_) {
            const PlantShootCandCost Pc{C, dq, d_ua, d_st, o_J.on(O), o_Dc.on(O), j_conv.on(N), B, M, NB, n_alpha};
            hipLaunchKernelGGL(plant_shoot_cand_cost_kernel, dim3((unsigned)nA), dim3(LS_THREADS), 0, st, Pc);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {
            const PlantShootGather G{dq, W.d_z, d_ua, dg, db, has_w ? dw : nullptr, d_st, d_it, j_conv.on(N), o_J.on(O), o_Dc.on(O), i_pn.on(I), i_Dn.on(I), i_dJ.on(I), i_al.on(I),
                                     i_wt.on(I), armijo, n_alpha, n_weight, o_phi.on(O), j_ok.on(N), j_ch.on(N), o_q.on(O), o_z.on(O), o_u.on(O), o_us.on(O), o_gv.on(O), o_bv.on(O),
                                     o_w.or_null(O), o_mu.or_null(O), i_mu.or_null(I), j_stv.on(N), j_itv.on(N), B, M, L, NB, nq, nu, nc,
                                     nb, nz, nw};
            hipLaunchKernelGGL(plant_shoot_gather_kernel, dim3((unsigned)((L + 2) * MB)), dim3(LS_THREADS), 0, st, G);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {      // the chosen segments' step gradients, each on its own virtual robot's rows l, l+1 and the control its step applied
            const PlantSensSource src{o_z.on(O), nullptr, o_q.on(O), o_u.on(O), o_w.or_null(O), o_mu.or_null(O), j_stv.on(N), mu[0], h, MB, L, MB, 1,
                                      has_w ? L : 1, has_w ? MB : 1, 1, mu_each ? MB : 1};
            ok_ = plant_sensitivity_launch(Mo, (int)TB, src, rough ? W.d_ter : nullptr, !rough ? 0 : ter_each ? MB : 1, reg, n_cols, W.d_grad, W.d_grad_st, st);
        }
        if (ok_) {
            const PlantShootStitch Ss{C, o_q.on(O), o_us.on(O), o_gv.on(O), o_bv.on(O), W.d_grad, j_stv.on(N), j_itv.on(N), W.d_grad_st, o_g.on(O), o_b.on(O), buf.d_dz, j_st.on(N), j_it.on(N),
                                      buf.d_status, o_def.on(O), o_lt.on(O), o_lq.on(O), o_lr.on(O), B, M, T, nq, nu, nc, nb, (int)block};
            hipLaunchKernelGGL(plant_shoot_stitch_kernel, dim3((unsigned)((T + 1) * B)), dim3(LS_THREADS), 0, st, Ss);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {
            hipLaunchKernelGGL(plant_shoot_total_kernel, dim3((unsigned)((B + SHOOT_TOTAL_THREADS - 1) / SHOOT_TOTAL_THREADS)), dim3(SHOOT_TOTAL_THREADS), 0, st,
                               (const double*)o_def.on(O), (const double*)o_lt.on(O), o_D.on(O), o_Jn.on(O), B, M, T, nq);
            ok_ = hipGetLastError() == hipSuccess;
        }
        ok_ = ok_ && plant_restore_launch(j_ch.on(N), parent.d_dz, parent.d_status, buf.d_dz, buf.d_status, B, T, (int)block, st);
        copy.down(J, O, o_J); copy.down(D_cand, O, o_Dc); copy.down(phi, O, o_phi); copy.down(ok, N, j_ok); copy.down(choice, N, j_ch);
        copy.down(qs, O, o_q); copy.down(u_applied, O, o_us); copy.down(gamma, O, o_g); copy.down(b, O, o_b); copy.down(status, N, j_st);
        copy.down(iters, N, j_it); copy.down(defects, O, o_def); copy.down(D, O, o_D); copy.down(J_chosen, O, o_Jn);
        copy.down(lin_q, O, o_lq); copy.down(lin_r, O, o_lr); copy.down(grad_status, buf.d_status, PlantSpan{0, TB});
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
    }
    if (!ok_) (void)buf.release();
    ok_ = scope.leave(ok_);
    if (!ok_) { (void)buf.release(); return CIMPC_ERR_HIP; }
    *new_tape = new cimpc_plant_tape_s{buf, model, B, T, n_cols};
    return CIMPC_OK;
}
