// The forward pass of an iLQR iteration through contact (DESIGN.md sections 3, item 3f, and 5.5): n_alpha step lengths of every robot
// in ONE closed-loop rollout of n_alpha x B robots, their costs, the per-robot choice, and the tape of the chosen trajectories.
//
//   cimpc_plant_tape_linesearch   the B-robot inputs up once; plant_ls_expand_kernel writes what the step kernel reads for the
//                                 n_alpha B candidates; the closed-loop step kernel's chunks (plant_step_launch.h); plant_ls_cost_kernel
//                                 (J and convergence per candidate); plant_ls_gather_kernel (acceptance, choice, the chosen candidates'
//                                 rows compacted to B robots, lin_q and lin_r on them); ONE sensitivity launch over T x B entries into the
//                                 new tape; plant_ls_restore_kernel (the parent's blocks for a robot without an acceptable candidate);
//                                 one read-back, one synchronize
//   cimpc_plant_tape_linesearch_box  the same call under control limits: the expansion kernel writes the
//                                 limited open-loop rows limit(u_nom + alpha k) and the candidates' limit rows, and the candidates run the
//                                 limited law (the step kernel's third state); the existing entry is this one with null limits
//   cimpc_plant_tracking_cost     plant_cost.h on the host with a team of one
//   plant_linesearch_plan / _shared / _stages   what both entries validate, upload beside the expansion kernel and launch, on device pointers
//                                 (plant_stage_launch.h): the entries above call them, and so does the device-resident iLQR loop (plant_ilqr.hip)
//
// The kernels here move rows and run the short ordered chains of plant_cost.h; a wavefront per workgroup.  The time of a line search is
// the step kernel's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

// No fused multiply-adds in this translation unit: the cost rounds as the float64 restatement of the definition does.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_cost.h"
#include "plant_model.h"
#include "plant_rollout_call.h"
#include "plant_sensitivity.h"
#include "plant_stage_launch.h"
#include "plant_step_launch.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

// Entry e = t NB + r of the candidates' inputs, r = c B + b, from the parent's rows of robot b (all device memory): the open-loop row, the
// gain block, the x_ref row; at t = 0 also trajectory rows 0 and 1, mu (given per robot) and the w schedule (given per robot).
struct PlantLsExpand {
    const double *q_nom, *u_nom, *k, *K, *w, *mu, *alpha;      // w, mu: null when shared (the step kernel then reads the parent's)
    double *q, *u, *fb_K, *x_ref, *w_out, *mu_out;
    int B, NB, T, nq, nu, nw, K_w;
    const double *u_lo, *u_hi;      // n_lim x nu limits of the B robots, or both null: no limits
    double *lo_out, *hi_out;        // the candidates' NB rows (n_lim = B), or null (n_lim = 1: the one row serves them all)
    int n_lim;
};

__global__ __launch_bounds__(LS_THREADS) void plant_ls_expand_kernel(PlantLsExpand E) {
    const int e = blockIdx.x, lane = threadIdx.x;
    if (e >= E.T * E.NB) return;
    const int t = e / E.NB, r = e % E.NB, c = r / E.B, b = r % E.B, nq = E.nq, nu = E.nu, kk = nu * 2 * nq;
    const size_t from = (size_t)t * E.B + b;
    const double *lo = E.u_lo ? plant_feedback_limits(E.u_lo, E.n_lim, b, nu) : nullptr, *hi = E.u_lo ? plant_feedback_limits(E.u_hi, E.n_lim, b, nu) : nullptr;
    for (int i = lane; i < nu; i += LS_THREADS) {
        const double ubar = plant_candidate_control(E.u_nom[from * nu + i], E.alpha[c], E.k[from * nu + i]);
        E.u[(size_t)e * nu + i] = lo ? plant_feedback_limit(ubar, lo[i], hi[i]) : ubar;
    }
    for (int i = lane; i < kk; i += LS_THREADS) E.fb_K[(size_t)e * kk + i] = E.K[from * kk + i];
    const double *q0 = E.q_nom + from * nq, *q1 = E.q_nom + (from + E.B) * nq;
    for (int j = lane; j < 2 * nq; j += LS_THREADS) E.x_ref[(size_t)e * 2 * nq + j] = plant_candidate_target(q0, q1, nq, j);
    if (t != 0) return;
    for (int i = lane; i < nq; i += LS_THREADS) {
        E.q[(size_t)r * nq + i] = q0[i];
        E.q[((size_t)E.NB + r) * nq + i] = q1[i];
    }
    if (E.mu && lane == 0) E.mu_out[r] = E.mu[b];
    if (E.lo_out)
        for (int i = lane; i < nu; i += LS_THREADS) { E.lo_out[(size_t)r * nu + i] = lo[i]; E.hi_out[(size_t)r * nu + i] = hi[i]; }
    if (E.w)
        for (int i = lane; i < E.K_w * E.nw; i += LS_THREADS) {
            const int row = i / E.nw, j = i % E.nw;
            E.w_out[((size_t)row * E.NB + r) * E.nw + j] = E.w[((size_t)row * E.B + b) * E.nw + j];
        }
}

// J of candidate robot r and whether its T steps converged, from the rollout's own buffers
struct PlantLsCost {
    PlantCost C;
    const double *q, *u_applied;      // (T + 2) x NB x nq, T x NB x nu
    const int* status;                // T x NB
    double* J;                        // NB
    int* conv;                        // NB
    int B, NB;
};

__global__ __launch_bounds__(LS_THREADS) void plant_ls_cost_kernel(PlantLsCost P) {
    __shared__ double work[LS_MAX_WORK];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= P.NB) return;
    const int nq = P.C.nq, nu = P.C.nu;
    PlantCostWave team;
    const double J = plant_cost_trajectory(P.C, P.C.n_x == 1 ? 0 : r % P.B, P.q + (size_t)r * nq, (size_t)P.NB * nq, P.u_applied + (size_t)r * nu,
                                           (size_t)P.NB * nu, work, nullptr, 0, nullptr, 0, team);
    int all = 1;
    for (int t = lane; t < P.C.T; t += LS_THREADS) all &= P.status[(size_t)t * P.NB + r] != 0;
    all = __syncthreads_and(all);
    if (lane == 0) { P.J[r] = J; P.conv[r] = all; }
}

// Row t (0 .. T+1) of robot b's chosen candidate, compacted to B robots; every workgroup of a robot finds the choice again from J and conv
// (n_alpha <= 64 tests), the one of row 0 stores it with the acceptability flags.
struct PlantLsGather {
    PlantCost C;
    const double *q, *z, *u_applied, *gamma, *b;      // the candidates': NB robots
    const int *status, *iters, *conv;
    const double *J, *J_nom, *dV, *alpha;
    double armijo;
    int n_alpha;
    int *ok, *choice;
    double *Cq, *Cz, *Cu, *Cg, *Cb;                   // the chosen: B robots
    int *Cst, *Cit;
    double *lin_q, *lin_r;
    int B, NB, nc, nb, nz;
};

__global__ __launch_bounds__(LS_THREADS) void plant_ls_gather_kernel(PlantLsGather G) {
    __shared__ double work[LS_MAX_WORK];
    __shared__ int s_ok[PLANT_LS_MAX_ALPHA];
    const int e = blockIdx.x, lane = threadIdx.x, T = G.C.T, B = G.B;
    if (e >= (T + 2) * B) return;
    const int t = e / B, b = e % B, nq = G.C.nq, nu = G.C.nu;
    for (int c = lane; c < G.n_alpha; c += LS_THREADS)
        s_ok[c] = plant_candidate_acceptable(G.conv[c * B + b] != 0, G.J[c * B + b], G.J_nom[b], G.armijo, G.alpha[c], G.dV[2 * b], G.dV[2 * b + 1]) ? 1 : 0;
    __syncthreads();
    const int choice = plant_linesearch_choice(G.J + b, (size_t)B, s_ok, 1, G.n_alpha);
    if (t == 0) {
        for (int c = lane; c < G.n_alpha; c += LS_THREADS) G.ok[c * B + b] = s_ok[c];
        if (lane == 0) G.choice[b] = choice;
    }
    const int r = (choice < 0 ? 0 : choice) * B + b;
    const size_t from = (size_t)t * G.NB + r, to = (size_t)t * B + b;
    for (int i = lane; i < nq; i += LS_THREADS) G.Cq[to * nq + i] = G.q[from * nq + i];
    if (t > T) return;
    if (t < T) {
        for (int i = lane; i < G.nz; i += LS_THREADS) G.Cz[to * G.nz + i] = G.z[from * G.nz + i];
        for (int i = lane; i < nu; i += LS_THREADS) G.Cu[to * nu + i] = G.u_applied[from * nu + i];
        for (int i = lane; i < G.nc; i += LS_THREADS) G.Cg[to * G.nc + i] = G.gamma[from * G.nc + i];
        for (int i = lane; i < G.nb; i += LS_THREADS) G.Cb[to * G.nb + i] = G.b[from * G.nb + i];
        if (lane == 0) { G.Cst[to] = G.status[from]; G.Cit[to] = G.iters[from]; }
    }
    PlantCostWave team;
    (void)plant_cost_stage(G.C, t, G.C.n_x == 1 ? 0 : b, G.q + from * nq, G.q + (from + G.NB) * nq, t < T ? G.u_applied + from * nu : nullptr, work,
                           G.lin_q + to * 2 * nq, t < T ? G.lin_r + to * nu : nullptr, team);
}

// Entry e = t B + b of the new tape gets the parent's block and status where robot b has no acceptable candidate
__global__ __launch_bounds__(LS_THREADS) void plant_ls_restore_kernel(const int* choice, const double* parent_dz, const int* parent_status, double* dz,
                                                                     int* status, int B, int T, int block) {
    const int e = blockIdx.x;
    if (e >= T * B || choice[e % B] >= 0) return;
    for (int i = threadIdx.x; i < block; i += LS_THREADS) dz[(size_t)e * block + i] = parent_dz[(size_t)e * block + i];
    if (threadIdx.x == 0) status[e] = parent_status[e];
}

namespace {
// the entry's own buffers, beside the candidates' rollout in the plant workspace: the B-robot inputs, the B-robot outputs with J, the
// integer outputs (plant_linesearch_layout, plant_staging.h)
PlantStageWs g_linesearch_ws[PLANT_MAX_DEVICES];
}  // namespace

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int cimpc_plant_tracking_cost(int nq, int nu, int B, int T, const cimpc_tracking_cost* cost, const double* q, const double* u_applied,
                                         double* J, double* lin_q, double* lin_r) {
    using namespace cimpc;
    if (!cost || !q || !u_applied || !J || nq < 1 || nu < 1 || B < 1 || T < 1) return CIMPC_ERR_INVALID;
    const PlantCost C = plant_cost_of(*cost, T, nq, nu);
    if (!plant_cost_valid(C, B)) return CIMPC_ERR_INVALID;
    std::vector<double> work(plant_cost_work_doubles(nq, nu));
    PlantCostSolo team;
    const size_t n = (size_t)2 * nq;
    for (int b = 0; b < B; ++b)
        J[b] = plant_cost_trajectory(C, C.n_x == 1 ? 0 : b, q + (size_t)b * nq, (size_t)B * nq, u_applied + (size_t)b * nu, (size_t)B * nu, work.data(),
                                     lin_q ? lin_q + b * n : nullptr, B * n, lin_r ? lin_r + (size_t)b * nu : nullptr, (size_t)B * nu, team);
    return CIMPC_OK;
}

// ---- the launch code (plant_stage_launch.h): what both entries and the device-resident iLQR loop share ------------------------------
namespace cimpc {

const char* plant_linesearch_plan(const PlantLsCall& c, PlantLsPlan* P) {
    if (const char* why = plant_linesearch_refusal(c.n_alpha, c.alpha, c.armijo)) return why;
    if (const char* why = plant_cost_pointers(plant_cost_of(*c.cost, 1, 1, 1))) return why;
    if (!(c.h > 0.0)) return "h not positive";
    const cimpc_plant_tape tape = c.tape;
    const bool limits = c.u_lo || c.u_hi;
    if (limits && (!c.u_lo || !c.u_hi)) return "one of u_lo, u_hi without the other";
    if (limits && c.n_lim != 1 && c.n_lim != tape->B) return "n_lim neither 1 nor B";
    if (limits) {      // the limits' entries: the model's nu by the tape's model id alone
        PlantModel named{};
        if (!plant_model_by_id(tape->model, &named) || named.nu < 1) return "a model without controls or not the tape's";
        for (size_t e = 0; e < (size_t)c.n_lim * named.nu; ++e) {
            if (c.u_lo[e] != c.u_lo[e] || c.u_hi[e] != c.u_hi[e]) return "a NaN limit";
            if (c.u_lo[e] > c.u_hi[e]) return "u_lo above u_hi";
        }
    }
    const PlantTapeBuffers& parent = tape->buf;
    const int B = tape->B, T = tape->T, n_cols = tape->n_cols;
    if (parent.device < 0 || parent.device >= PLANT_MAX_DEVICES || !parent.d_dz || !parent.d_status) return "a closed tape";
    if (!plant_linesearch_fits(c.n_alpha, B, T)) return "n_alpha B T beyond an int";
    // everything cimpc_plant_rollout_tape validates for the B robots of the parent, on the arrays that stand in for its arguments
    const PlantRolloutCall parent_call{.model = tape->model, .B = B, .T = T, .steps_per_launch = c.steps_per_launch, .n_terrain = c.n_terrain,
                                       .terrain = c.terrain, .q0 = c.q_nom, .q1 = c.q_nom, .u = {c.u_nom, T, B, 1}, .w = {c.w, c.K_w, c.n_w, c.hold_w},
                                       .mu = c.mu, .n_mu = c.n_mu, .h = c.h, .opts = c.opts, .q = c.q, .gamma = c.gamma, .b = c.b, .status = c.status,
                                       .iters = c.iters, .grad = PlantRolloutGrad{c.reg, n_cols, nullptr, nullptr, c.grad_status, true}};
    PlantModel M{};
    bool rough = false;
    if (plant_rollout_check(parent_call, &M, &rough) != CIMPC_OK) return "an argument that cimpc_plant_rollout_tape refuses for the tape's B robots";
    const int nq = M.nq, nu = M.nu, nz = M.nz(), NB = c.n_alpha * B;
    if (M.kind != parent.M.kind || nq != parent.M.nq || nu < 1 || 2 * nq > nz) return "a model without controls or not the tape's";
    const PlantCost C = plant_cost_of(*c.cost, T, nq, nu);
    if (const char* why = plant_cost_sizes(C, B)) return why;
    // the candidates' rollout in the plant workspace, laid out as a closed-loop tape call of NB robots lays itself out
    const bool w_each = c.w && c.n_w != 1, mu_each = c.n_mu != 1;
    const cimpc_feedback fb_shape{c.q_nom, c.q_nom, T, NB, 1, 1.0};      // only the shape is read
    const PlantRolloutCall cand_call{.model = tape->model, .B = NB, .T = T, .steps_per_launch = c.steps_per_launch, .n_terrain = 0, .terrain = nullptr,
                                     .q0 = c.q_nom, .q1 = c.q_nom, .u = {c.u_nom, T, NB, 1}, .w = {c.w, c.K_w, w_each ? NB : 1, c.hold_w}, .mu = c.mu,
                                     .n_mu = mu_each ? NB : 1, .h = c.h, .opts = c.opts, .q = c.q, .gamma = c.gamma, .b = c.b, .status = c.status,
                                     .iters = c.iters, .grad = PlantRolloutGrad{c.reg, n_cols, nullptr, nullptr, c.grad_status, true},
                                     .loop = PlantRolloutLoop{&fb_shape, c.u_applied, nullptr, c.u_lo, c.u_hi, !limits || c.n_lim == 1 ? 1 : NB}};
    P->M = M; P->rough = rough; P->has_w = c.w != nullptr; P->w_each = w_each; P->mu_each = mu_each; P->limits = limits;
    P->lim_each = limits && c.n_lim != 1; P->ter_each = rough && c.n_terrain != 1;
    P->C = C; P->L = plant_rollout_layout(M, cand_call);
    P->model = tape->model; P->B = B; P->T = T; P->NB = NB; P->n_alpha = c.n_alpha; P->n_cols = n_cols; P->steps_per_launch = c.steps_per_launch;
    P->K_w = c.K_w; P->n_w = c.n_w; P->hold_w = c.hold_w; P->n_mu = c.n_mu; P->n_terrain = c.n_terrain;
    P->n_ter = !rough ? 0 : P->ter_each ? NB : 1; P->n_lim = c.n_lim;
    P->mu0 = c.mu[0]; P->h = c.h; P->armijo = c.armijo; P->reg = c.reg; P->opts = *c.opts;
    return nullptr;
}

std::vector<cimpc_terrain> plant_linesearch_terrains(const PlantLsPlan& P, const cimpc_terrain* terrain) {
    std::vector<cimpc_terrain> ter;
    if (P.ter_each) for (int c = 0; c < P.n_alpha; ++c) ter.insert(ter.end(), terrain, terrain + P.B);
    return ter;
}

bool plant_linesearch_shared(const PlantLsPlan& P, const double* w, const cimpc_terrain* terrain, const std::vector<cimpc_terrain>& ter, PlantWs& W,
                             hipStream_t st) {
    bool ok_ = true;
    if (P.has_w && !P.w_each)      // a shared schedule serves the candidates as it stands
        ok_ = hipMemcpyAsync(W.d_in + P.L.w.at, w, (size_t)P.K_w * P.M.nw * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    if (P.rough)
        ok_ = ok_ && hipMemcpyAsync(W.d_ter, P.ter_each ? ter.data() : terrain, (size_t)P.n_ter * sizeof(cimpc_terrain), hipMemcpyHostToDevice, st) == hipSuccess;
    return ok_;
}

bool plant_candidates_cost_launch(const PlantCost& C, const double* q, const double* u_applied, const int* status, double* J, int* conv, int B, int NB,
                                  hipStream_t st) {
    const PlantLsCost Pc{C, q, u_applied, status, J, conv, B, NB};
    hipLaunchKernelGGL(plant_ls_cost_kernel, dim3(NB), dim3(LS_THREADS), 0, st, Pc);
    return hipGetLastError() == hipSuccess;
}

bool plant_restore_launch(const int* choice, const double* parent_dz, const int* parent_status, double* dz, int* status, int B, int T, int block,
                          hipStream_t st) {
    hipLaunchKernelGGL(plant_ls_restore_kernel, dim3((unsigned)((size_t)T * B)), dim3(LS_THREADS), 0, st, choice, parent_dz, parent_status, dz, status, B, T, block);
    return hipGetLastError() == hipSuccess;
}

bool plant_linesearch_stages(const PlantLsPlan& P, const PlantLsArrays& A, PlantWs& W, hipStream_t st) {
    const PlantModel& M = P.M;
    const PlantRolloutLayout& L = P.L;
    const int B = P.B, T = P.T, NB = P.NB, nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), nz = M.nz(), nw = M.nw, nr = nq + nc + nb, n_cols = P.n_cols;
    const bool has_w = P.has_w, w_each = P.w_each, mu_each = P.mu_each, limits = P.limits, lim_each = P.lim_each, rough = P.rough;
    const size_t TB = (size_t)T * B, block = (size_t)nr * n_cols;
    // the candidates' limits: the one shared row where it stands, or NB rows the expansion kernel writes behind the loop's arrays
    const double *c_lo = !limits ? nullptr : lim_each ? W.d_fb + L.u_lo.at : A.u_lo, *c_hi = !limits ? nullptr : lim_each ? W.d_fb + L.u_hi.at : A.u_hi;
    double *dq = W.d_in + L.q.at, *du = W.d_in + L.u.at, *dw = W.d_in + L.w.at, *dmu = W.d_in + L.mu.at;
    double *d_fk = W.d_fb + L.fb_K.at, *d_fx = W.d_fb + L.x_ref.at, *d_ua = W.d_fb + L.u_applied.at, *d_fe = W.d_fb + L.fb_err.at;
    double *dg = W.d_out + L.gamma.at, *db = W.d_out + L.b.at;
    int *d_st = W.d_st + L.status.at, *d_it = W.d_st + L.iters.at;
    const PlantLsExpand E{A.q_nom, A.u_nom, A.k, A.K, w_each ? A.w : nullptr, mu_each ? A.mu : nullptr, A.alpha,
                          dq, du, d_fk, d_fx, dw, dmu, B, NB, T, nq, nu, nw, has_w ? P.K_w : 0, limits ? A.u_lo : nullptr, limits ? A.u_hi : nullptr,
                          lim_each ? W.d_fb + L.u_lo.at : nullptr, lim_each ? W.d_fb + L.u_hi.at : nullptr, P.n_lim};
    hipLaunchKernelGGL(plant_ls_expand_kernel, dim3(T * NB), dim3(LS_THREADS), 0, st, E);
    if (hipGetLastError() != hipSuccess) return false;
    const PlantStepArrays R{dq, du, has_w ? dw : nullptr, mu_each ? dmu : nullptr, dg, db, d_st, d_it, P.mu0, P.h, T, NB, 1, has_w ? P.K_w : 1,
                            w_each ? NB : 1, has_w ? P.hold_w : 1, mu_each ? NB : 1, W.d_z, PlantFeedback{d_fk, d_fx, T, NB, 1, 1.0}, d_ua, d_fe,
                            PlantFeedbackLimits{c_lo, c_hi, lim_each ? NB : 1}};
    if (!plant_step_chunks(M, rough, P.opts, NB, T, P.steps_per_launch, R, rough ? W.d_ter : nullptr, P.n_ter, st)) return false;
    if (!plant_candidates_cost_launch(A.C, dq, d_ua, d_st, A.J, A.conv, B, NB, st)) return false;
    const PlantLsGather G{A.C, dq, W.d_z, d_ua, dg, db, d_st, d_it, A.conv, A.J, A.J_nom, A.dV, A.alpha, P.armijo, P.n_alpha,
                          A.ok, A.choice, A.Cq, A.Cz, A.Cu, A.Cg, A.Cb, A.Cst, A.Cit, A.lin_q, A.lin_r, B, NB, nc, nb, nz};
    hipLaunchKernelGGL(plant_ls_gather_kernel, dim3((T + 2) * B), dim3(LS_THREADS), 0, st, G);
    if (hipGetLastError() != hipSuccess) return false;
    // the chosen trajectories' step gradients: an open-loop rollout of B robots on the controls their steps applied
    const PlantSensSource src{A.Cz, nullptr, A.Cq, A.Cu, !has_w ? nullptr : w_each ? A.w : dw, mu_each ? A.mu : nullptr, A.Cst,
                              P.mu0, P.h, B, T, B, 1, has_w ? P.K_w : 1, has_w ? P.n_w : 1, has_w ? P.hold_w : 1, P.n_mu};
    if (!plant_sensitivity_launch(M, (int)TB, src, rough ? W.d_ter : nullptr, rough ? P.n_terrain : 0, P.reg, n_cols, A.dz, A.status, st)) return false;
    return plant_restore_launch(A.choice, A.parent_dz, A.parent_status, A.dz, A.status, B, T, (int)block, st);
}

}  // namespace cimpc

// Both entries: u_lo, u_hi null (cimpc_plant_tape_linesearch) or n_lim x nu limits (cimpc_plant_tape_linesearch_box).
static int plant_tape_linesearch_call(const char* entry, cimpc_plant_tape tape, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                      const double* q_nom, const double* u_nom, const double* w, int K_w, int n_w, int hold_w,
                                      const double* mu, int n_mu, double h, const cimpc_ip_opts* opts, const double* K, const double* k,
                                      const double* dV, const double* J_nom, int n_alpha, const double* alpha, double armijo,
                                      const cimpc_tracking_cost* cost, double reg, double* J, int* ok, int* choice, double* q,
                                      double* u_applied, double* gamma, double* b, int* status, int* iters, double* lin_q, double* lin_r,
                                      int* grad_status, cimpc_plant_tape* new_tape, int n_lim, const double* u_lo, const double* u_hi) {
    using namespace cimpc;
    // every refusal leaves its reason where cimpc_last_error(NULL) finds it; what needs no tape is tested before the tape is looked at
    auto refuse = [entry](const std::string& why) { return plant_refuse(entry, why); };
    if (!new_tape) return refuse("null new_tape");
    *new_tape = nullptr;
    const PlantRequired required[] = {
        {"tape", tape}, {"q_nom", q_nom}, {"u_nom", u_nom}, {"mu", mu}, {"opts", opts}, {"K", K}, {"k", k}, {"dV", dV}, {"J_nom", J_nom}, {"alpha", alpha},
        {"cost", cost}, {"J", J}, {"ok", ok}, {"choice", choice}, {"q", q}, {"u_applied", u_applied}, {"gamma", gamma}, {"b", b}, {"status", status},
        {"iters", iters}, {"lin_q", lin_q}, {"lin_r", lin_r}, {"grad_status", grad_status}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
    PlantLsPlan P;
    if (const char* why = plant_linesearch_plan(PlantLsCall{tape, steps_per_launch, n_terrain, terrain, q_nom, u_nom, w, K_w, n_w, hold_w, mu, n_mu, h, opts,
                                                            n_alpha, alpha, armijo, cost, reg, q, u_applied, gamma, b, status, iters, grad_status, n_lim,
                                                            u_lo, u_hi}, &P))
        return refuse(why);
    const PlantTapeBuffers& parent = tape->buf;
    const PlantModel& M = P.M;
    const PlantRolloutLayout& L = P.L;
    const int B = P.B, T = P.T, n_cols = P.n_cols;
    const size_t TB = (size_t)T * B, block = (size_t)(M.nq + M.nc + M.nb()) * n_cols;
    // the B-robot inputs in d_in, J and the chosen candidates' rows in d_out, the integers in d_int
    const PlantLsLayout S = plant_linesearch_layout(M, P.C, PlantLsShape{B, T, P.n_alpha, P.K_w, P.n_lim, P.w_each, P.mu_each, P.limits});
    // the inputs the candidates' law is made of are finite, as cimpc_plant_rollout_feedback asks of K and x_ref
    if (!plant_all_finite(K, S.K.n)) return refuse("a non-finite entry of K");
    if (!plant_all_finite(k, S.k.n)) return refuse("a non-finite entry of k");
    if (!plant_all_finite(q_nom, S.q_nom.n)) return refuse("a non-finite entry of q_nom");
    if (!plant_all_finite(u_nom, S.u_nom.n)) return refuse("a non-finite entry of u_nom");
    const std::vector<cimpc_terrain> ter = plant_linesearch_terrains(P, terrain);      // the candidates' terrains: robot b's for every c

    const int dev = parent.device;
    PlantDeviceScope scope(dev);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok_ = false;
    PlantTapeBuffers buf;
    PlantWs* ws = plant_ws_open(dev);
    PlantStageWs& G = g_linesearch_ws[dev];
    if (ws && plant_grow(&ws->d_in, &ws->cap_in, L.need_in) && plant_grow(&ws->d_out, &ws->cap_out, L.need_out) && plant_grow(&ws->d_st, &ws->cap_st, L.need_st) &&
        plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)P.n_ter) && plant_grow(&ws->d_z, &ws->cap_z, L.need_z) && plant_grow(&ws->d_fb, &ws->cap_fb, L.need_fb) &&
        G.grow(S.need_in, S.need_out, S.need_int) &&
        hipMalloc((void**)&buf.d_dz, TB * block * sizeof(double)) == hipSuccess) {      // the new tape's memory, the last to be allocated
        if (hipMalloc((void**)&buf.d_status, TB * sizeof(int)) != hipSuccess) buf.d_status = nullptr;
        buf.device = dev; buf.M = M;
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        ok_ = buf.d_status != nullptr;
        PlantStreamCopier copy{{st}, ok_};
        double *I = G.d_in, *O = G.d_out;
        int* N = G.d_int;
        copy.up(I, S.q_nom, q_nom); copy.up(I, S.u_nom, u_nom); copy.up(I, S.k, k); copy.up(I, S.K, K);
        copy.up(I, S.w, w); copy.up(I, S.mu, mu);      // where they are per robot
        copy.up(I, S.dV, dV); copy.up(I, S.J_nom, J_nom); copy.up(I, S.alpha, alpha);
        const PlantCost C = plant_cost_up(copy, I, S.cost, P.C);
        copy.up(I, S.u_lo, u_lo); copy.up(I, S.u_hi, u_hi);
        ok_ = ok_ && plant_linesearch_shared(P, w, terrain, ter, W, st);
        if (ok_) {
            const PlantLsArrays A{S.q_nom.on(I), S.u_nom.on(I), S.k.on(I), S.K.on(I), S.w.or_null(I), S.mu.or_null(I), S.dV.on(I), S.J_nom.on(I), S.alpha.on(I),
                                  S.u_lo.or_null(I), S.u_hi.or_null(I), C, S.J.on(O), S.ok.on(N), S.choice.on(N), S.conv.on(N), S.q.on(O), S.z.on(O),
                                  S.u_applied.on(O), S.gamma.on(O), S.b.on(O), S.status.on(N), S.iters.on(N), S.lin_q.on(O), S.lin_r.on(O), parent.d_dz,
                                  parent.d_status, buf.d_dz, buf.d_status};
            ok_ = plant_linesearch_stages(P, A, W, st);
        }
        copy.down(J, O, S.J); copy.down(q, O, S.q); copy.down(u_applied, O, S.u_applied); copy.down(gamma, O, S.gamma);
        copy.down(b, O, S.b); copy.down(lin_q, O, S.lin_q); copy.down(lin_r, O, S.lin_r);
        copy.down(ok, N, S.ok); copy.down(choice, N, S.choice); copy.down(status, N, S.status); copy.down(iters, N, S.iters);
        copy.down(grad_status, buf.d_status, PlantSpan{0, TB});
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
    }
    if (!ok_) (void)buf.release();
    ok_ = scope.leave(ok_);
    if (!ok_) { (void)buf.release(); return CIMPC_ERR_HIP; }
    *new_tape = new cimpc_plant_tape_s{buf, tape->model, B, T, n_cols};
    return CIMPC_OK;
}

extern "C" int cimpc_plant_tape_linesearch(cimpc_plant_tape tape, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                           const double* q_nom, const double* u_nom, const double* w, int K_w, int n_w, int hold_w,
                                           const double* mu, int n_mu, double h, const cimpc_ip_opts* opts, const double* K, const double* k,
                                           const double* dV, const double* J_nom, int n_alpha, const double* alpha, double armijo,
                                           const cimpc_tracking_cost* cost, double reg, double* J, int* ok, int* choice, double* q,
                                           double* u_applied, double* gamma, double* b, int* status, int* iters, double* lin_q, double* lin_r,
                                           int* grad_status, cimpc_plant_tape* new_tape) {
    return plant_tape_linesearch_call("cimpc_plant_tape_linesearch", tape, steps_per_launch, n_terrain, terrain, q_nom, u_nom, w, K_w, n_w, hold_w, mu, n_mu,
                                      h, opts, K, k, dV, J_nom, n_alpha, alpha, armijo, cost, reg, J, ok, choice, q, u_applied, gamma, b, status, iters,
                                      lin_q, lin_r, grad_status, new_tape, 1, nullptr, nullptr);
}

// The line search under control limits: candidate c of robot b applies
// u_t = limit(limit(u_nom + alpha_c k_t) + K_t (x_ref_t - x_t)) with n_lim (1 or B) rows u_lo, u_hi of nu limits.  Acceptance, choice and the
// new tape - the open-loop tape of the chosen u_applied - are cimpc_plant_tape_linesearch's.
extern "C" int cimpc_plant_tape_linesearch_box(cimpc_plant_tape tape, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                               const double* q_nom, const double* u_nom, const double* w, int K_w, int n_w, int hold_w,
                                               const double* mu, int n_mu, double h, const cimpc_ip_opts* opts, const double* K, const double* k,
                                               const double* dV, const double* J_nom, int n_alpha, const double* alpha, double armijo,
                                               const cimpc_tracking_cost* cost, double reg, double* J, int* ok, int* choice, double* q,
                                               double* u_applied, double* gamma, double* b, int* status, int* iters, double* lin_q, double* lin_r,
                                               int* grad_status, cimpc_plant_tape* new_tape, int n_lim, const double* u_lo, const double* u_hi) {
    if ((u_lo == nullptr) != (u_hi == nullptr)) return cimpc::plant_refuse("cimpc_plant_tape_linesearch_box", "one of u_lo, u_hi without the other");
    return plant_tape_linesearch_call("cimpc_plant_tape_linesearch_box", tape, steps_per_launch, n_terrain, terrain, q_nom, u_nom, w, K_w, n_w, hold_w, mu,
                                      n_mu, h, opts, K, k, dV, J_nom, n_alpha, alpha, armijo, cost, reg, J, ok, choice, q, u_applied, gamma, b, status,
                                      iters, lin_q, lin_r, grad_status, new_tape, n_lim, u_lo, u_hi);
}
