// The sampling policy on the plant - predictive sampling and the MPPI mean (DESIGN.md sections 3, item 3k, and 5.5): a handle that keeps the
// problem and the plan of B robots on the device between control steps.  A control step rolls out N perturbed copies of the plan per robot
// in ONE open-loop rollout of N B robots, scores them with the tracking cost and keeps the best one (lam = 0) or their softmax mean (lam > 0):
//
//   the start rows up             q[0] = q0, q[1] = q1 into the handle's trajectory: 2 B nq doubles
//   plant_sample_begin_kernel     a workgroup per (row t, robot b): the shifted plan into the other control buffer, the goal window of step s into
//                                 the cost's x_goal / u_goal - the index rules of plant_mpc.h
//   n_iter times:
//     plant_sample_expand_kernel  a lane per (noise row, candidate robot, control): ONE Philox call, the candidate controls of the steps the row is
//                                 held over; further lanes copy rows 0 and 1 and, where it is per robot, mu to the N B candidates
//     plant_step_chunks           the existing open-loop step kernel on N B robots in the shared plant workspace, laid out by plant_rollout_layout
//     plant_ls_cost_kernel        J and convergence per candidate (plant_candidates_cost_launch, plant_stage_launch.h)
//     plant_sample_update_kernel  a workgroup per robot: eligibility, choice, weights, the new plan in place (plant_sample_update, plant_sample.h);
//                                 in predictive-sampling mode the last iteration also copies the chosen candidate's q, gamma, b, status, iters
//   one read-back, one synchronize
//
// No tape, no sensitivity launch, no backward pass.  The kernels here move rows and run short ordered chains; no result depends by a bit on
// the launch geometry.  The time of a control step is the step kernel's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

// No fused multiply-adds in this translation unit: the candidates and the mean round as the float64 restatement does.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_cost.h"
#include "plant_model.h"
#include "plant_mpc.h"
#include "plant_rollout_call.h"
#include "plant_sample.h"
#include "plant_stage_launch.h"
#include "plant_step_launch.h"
#include "plant_workspace.h"

namespace cimpc {

constexpr int SMP_THREADS = 256;

struct PlantSampleBegin {
    const double* u_plan;      // H x B x nu
    double* u_warm;
    const double *x_ref, *u_ref;      // (L + 1) x n_x x n, L x n_x x nu
    double *x_goal, *u_goal;          // (H + 1) x n_x x n, H x n_x x nu
    int B, H, L, n_x, nq, nu, s, shift;
};

__global__ __launch_bounds__(LS_THREADS) void plant_sample_begin_kernel(PlantSampleBegin P) {
    const int e = blockIdx.x, lane = threadIdx.x, B = P.B, H = P.H;
    if (e >= (H + 1) * B) return;
    const int t = e / B, b = e % B;
    if (t < H) plant_mpc_warm_start(P.u_warm, P.u_plan, t, b, P.shift, H, B, P.nu, lane, LS_THREADS);
    if (b < P.n_x) plant_mpc_window(P.x_goal, P.u_goal, P.x_ref, P.u_ref, P.s, t, b, H, P.L, P.n_x, 2 * P.nq, P.nu, lane, LS_THREADS);
}

// What the step kernel reads for the N B candidates (r = c B + b), from the B robots' rows: the controls u H x NB x nu, trajectory rows 0
// and 1, mu where it is per robot.  Items: n_rows NB nu noise items, then NB nq state items, then NB friction items.
struct PlantSampleExpand {
    const double *u_nom, *q01, *mu, *sigma;      // H x B x nu; 2 x B x nq; B or null; nu
    const double *u_lo, *u_hi;                   // n_lim x nu, or both null
    double *q, *u, *mu_out;
    int n_lim, B, N, H, nq, nu, noise_hold, n_rows;
    uint64_t seed;
    uint32_t draw;
};

__global__ __launch_bounds__(SMP_THREADS) void plant_sample_expand_kernel(PlantSampleExpand E) {
    size_t idx = (size_t)blockIdx.x * SMP_THREADS + threadIdx.x;
    const int B = E.B, nu = E.nu, nq = E.nq;
    const size_t NB = (size_t)E.N * B, n_noise = (size_t)E.n_rows * NB * nu;
    if (idx < n_noise) {
        const int i = (int)(idx % nu), j = (int)(idx / ((size_t)nu * NB));
        const size_t r = (idx / nu) % NB;
        const int c = (int)(r / B), b = (int)(r % B);
        const double eps = c == 0 ? 0.0 : plant_sample_eps(E.seed, E.draw, (uint32_t)b, (uint32_t)c, (uint32_t)j * (uint32_t)nu + (uint32_t)i);
        const double *lo = E.u_lo ? plant_feedback_limits(E.u_lo, E.n_lim, b, nu) : nullptr, *hi = E.u_lo ? plant_feedback_limits(E.u_hi, E.n_lim, b, nu) : nullptr;
        const long long t0 = (long long)j * E.noise_hold, t1 = t0 + E.noise_hold < E.H ? t0 + E.noise_hold : E.H;
        for (long long t = t0; t < t1; ++t)
            E.u[((size_t)t * NB + r) * nu + i] = plant_sample_candidate(E.u_nom[((size_t)t * B + b) * nu + i], E.sigma[i], eps, c, lo, hi, i);
        return;
    }
    idx -= n_noise;
    if (idx < NB * nq) {
        const size_t r = idx / nq, b = r % B;
        const int i = (int)(idx % nq);
        E.q[r * nq + i] = E.q01[b * nq + i];
        E.q[(NB + r) * nq + i] = E.q01[((size_t)B + b) * nq + i];
        return;
    }
    idx -= NB * nq;
    if (idx < NB && E.mu) E.mu_out[idx] = E.mu[idx % B];
}

struct PlantSampleTeam {
    __device__ int rank() const { return threadIdx.x; }
    __device__ int size() const { return SMP_THREADS; }
    __device__ void sync() const { __syncthreads(); }
};

// The chosen candidate's rows compacted to B robots (copy != 0: predictive sampling's last iteration), from the candidates' rollout
struct PlantSampleKeep {
    const double *q, *gamma, *b;      // the candidates': NB robots
    const int *status, *iters;
    double *Cq, *Cg, *Cb;             // the chosen: B robots
    int *Cst, *Cit;
    int* done;                        // B: the last iteration has a choice, whose steps all converged
    int nq, nc, nb, copy, last;
};

__global__ __launch_bounds__(SMP_THREADS) void plant_sample_update_kernel(PlantSampleUpdate P, PlantSampleKeep K) {
    const int b = blockIdx.x, lane = threadIdx.x, B = P.B, H = P.H;
    if (b >= B) return;
    PlantSampleTeam team;
    const int choice = plant_sample_update(P, b, team);
    if (K.last && lane == 0) K.done[b] = choice >= 0 ? 1 : 0;
    if (!K.copy) return;
    const size_t NB = (size_t)P.N * B, r = (size_t)(choice < 0 ? 0 : choice) * B + b;
    const int nq = K.nq, nc = K.nc, nb = K.nb;
    for (long long e = lane; e < (long long)(H + 2) * nq; e += SMP_THREADS) {
        const size_t t = (size_t)(e / nq), i = (size_t)(e % nq);
        K.Cq[(t * B + b) * nq + i] = K.q[(t * NB + r) * nq + i];
    }
    for (long long e = lane; e < (long long)H * nc; e += SMP_THREADS) {
        const size_t t = (size_t)(e / nc), i = (size_t)(e % nc);
        K.Cg[(t * B + b) * nc + i] = K.gamma[(t * NB + r) * nc + i];
    }
    for (long long e = lane; e < (long long)H * nb; e += SMP_THREADS) {
        const size_t t = (size_t)(e / nb), i = (size_t)(e % nb);
        K.Cb[(t * B + b) * nb + i] = K.b[(t * NB + r) * nb + i];
    }
    for (int t = lane; t < H; t += SMP_THREADS) {
        K.Cst[(size_t)t * B + b] = K.status[(size_t)t * NB + r];
        K.Cit[(size_t)t * B + b] = K.iters[(size_t)t * NB + r];
    }
}

}  // namespace cimpc

// What a cimpc_plant_sampler points to.  F and I are the handle's doubles and ints; the members named i_*, m_*, ... are their regions (plant_staging.h).
struct cimpc_plant_sampler_s {
    cimpc::PlantModel M{};
    cimpc::PlantCost C{};               // device pointers; T = H
    cimpc::PlantRolloutLayout Lw{};     // the candidates' rollout in the plant workspace: an open-loop call of N B robots
    cimpc_ip_opts opts{};
    bool rough = false, mu_each = false, ter_each = false, limits = false;
    int device = -1, model = 0, B = 0, H = 0, L = 0, n_x = 1, N = 0, NB = 0, n_iter = 0, noise_hold = 1, n_rows = 0, steps_per_launch = 0, n_mu = 1,
        n_terrain = 0, n_ter = 0, n_lim = 1;
    double mu0 = 0.0, h = 0.0, lam = 0.0;
    uint64_t seed = 0;
    bool has_plan = false, failed = false, has_state = false, traj_valid = false;
    int cur = 0;              // which of the two control buffers holds the plan
    int n_rollouts = 0;       // the B-robot rollouts cimpc_plant_sampler_plan has run
    double* F = nullptr;
    int* I = nullptr;
    cimpc_terrain* d_ter = nullptr;      // the candidates' terrains (n_ter), whose first n_terrain are the robots'
    std::vector<double> lo, hi;          // the limits on the host (n_lim x nu; empty: none), for the plans cimpc_plant_sampler_reset is given
    // doubles: the problem | the plan's two control buffers | the plan's trajectory | J, weights and unnormalised weights per iteration | the history
    // i_ref: Q | Qf | R | x_ref | u_ref, the cost over the reference's L steps; i_xg, i_ug: the goal window of a control step
    cimpc::PlantCostSpans i_ref;
    cimpc::PlantSpan i_mu, i_sig, i_xg, i_ug, i_lo, i_hi, p_u[2], m_q, m_g, m_b, o_J, o_w, o_wr, h_Jn, h_Jb;
    cimpc::PlantSpan j_st, j_it, j_conv, j_ok, j_ch, j_ne, j_done;
    size_t n_f = 0, n_i = 0;
};

namespace {
using namespace cimpc;

// Frees what the handle owns on its device (the caller holds g_plant_mu and has selected the device).
bool smp_release(cimpc_plant_sampler_s* h) {
    bool ok = plant_free(&h->F);
    ok = plant_free(&h->I) && ok;
    return plant_free(&h->d_ter) && ok;
}

const char* const SMP_FAILED = "a handle that met a HIP error refuses further use";

// the B robots' open-loop rollout of the plan on the handle's own arrays: bit for bit cimpc_plant_rollout on the plan
bool smp_roll_plan(cimpc_plant_sampler_s& S, PlantWs& W, hipStream_t st) {
    double* F = S.F;
    if (S.rough && hipMemcpyAsync(W.d_ter, S.d_ter, (size_t)S.n_terrain * sizeof(cimpc_terrain), hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    const PlantStepArrays R{S.m_q.on(F), S.p_u[S.cur].on(F), nullptr, S.i_mu.or_null(F), S.m_g.on(F), S.m_b.on(F), S.j_st.on(S.I), S.j_it.on(S.I), S.mu0, S.h,
                            S.H, S.B, 1, 1, 1, 1, S.n_mu, nullptr, PlantFeedback{}, nullptr, nullptr};
    return plant_step_chunks(S.M, S.rough, S.opts, S.B, S.H, S.steps_per_launch, R, S.rough ? W.d_ter : nullptr, S.rough ? S.n_terrain : 0, st);
}
}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int cimpc_plant_sample_noise(unsigned long long seed, unsigned int draw, int B, int N, int n_rows, int nu, double* eps) {
    using namespace cimpc;
    if (!eps) return plant_refuse("cimpc_plant_sample_noise", "null eps");
    if (B < 1 || N < 1 || n_rows < 1 || nu < 1) return plant_refuse("cimpc_plant_sample_noise", "B, N, n_rows or nu below 1");
    size_t at = 0;
    for (int j = 0; j < n_rows; ++j)
        for (int c = 0; c < N; ++c)
            for (int b = 0; b < B; ++b)
                for (int i = 0; i < nu; ++i)
                    eps[at++] = plant_sample_eps((uint64_t)seed, (uint32_t)draw, (uint32_t)b, (uint32_t)c, (uint32_t)j * (uint32_t)nu + (uint32_t)i);
    return CIMPC_OK;
}

extern "C" int cimpc_plant_sampler_create(int model, int B, int H, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain, const double* mu, int n_mu,
                                          double h, const cimpc_ip_opts* opts, const double* Q, const double* Qf, const double* R, int n_Q, int n_R, int L,
                                          int n_x, const double* x_ref, const double* u_ref, int N, const double* sigma, int noise_hold, double lam,
                                          int n_iter, unsigned long long seed, int n_lim, const double* u_lo, const double* u_hi, const double* u0,
                                          cimpc_plant_sampler* handle) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_sampler_create", why); };
    if (!handle) return refuse("null handle");
    *handle = nullptr;
    const PlantRequired required[] = {{"mu", mu}, {"opts", opts}, {"Q", Q}, {"Qf", Qf}, {"R", R}, {"x_ref", x_ref}, {"u_ref", u_ref}, {"u0", u0}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
    if (const char* why = plant_mpc_problem_refusal(H, L, n_iter)) return refuse(why);
    PlantModel named{};
    if (!plant_model_by_id(model, &named)) return refuse("an unknown model");
    if (B < 1) return refuse("B below 1");
    if (named.nu < 1) return refuse("a model without controls");
    if (const char* why = plant_sample_refusal(N, B, H, named.nu, sigma, noise_hold, lam, n_iter)) return refuse(why);
    if (const char* why = plant_cost_pointers(PlantCost{Q, Qf, R, x_ref, u_ref, n_Q, n_R, n_x, 1, 1, 1})) return refuse(why);
    if (!(h > 0.0)) return refuse("h not positive");
    const bool limits = u_lo || u_hi;
    if (limits && (!u_lo || !u_hi)) return refuse("one of u_lo, u_hi without the other");
    if (limits)
        if (const char* why = plant_limits_refusal(model, B, PlantRolloutLoop{nullptr, nullptr, nullptr, u_lo, u_hi, n_lim}, false)) return refuse(why);
    // everything cimpc_plant_rollout validates for the B robots, on arrays that stand in for its arguments: only that they are given is looked at
    static double stand_d;
    static int stand_i;
    const PlantRolloutCall robots{.model = model, .B = B, .T = H, .steps_per_launch = steps_per_launch, .n_terrain = n_terrain, .terrain = terrain,
                                  .q0 = &stand_d, .q1 = &stand_d, .u = {u0, H, B, 1}, .w = {nullptr, 1, 1, 1}, .mu = mu, .n_mu = n_mu, .h = h, .opts = opts,
                                  .q = &stand_d, .gamma = &stand_d, .b = &stand_d, .status = &stand_i, .iters = &stand_i};
    PlantModel M{};
    bool rough = false;
    if (plant_rollout_check(robots, &M, &rough) != CIMPC_OK) return refuse("an argument that cimpc_plant_rollout refuses for the B robots");
    const int nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), NB = N * B, T = H;
    const PlantCost Chost{Q, Qf, R, x_ref, u_ref, n_Q, n_R, n_x, T, nq, nu};
    if (const char* why = plant_cost_sizes(Chost, B)) return refuse(why);
    if ((long long)L + 1 > (1LL << 30) / ((long long)n_x * 2 * nq)) return refuse("a reference beyond 2^30 doubles");
    if (const char* why = plant_mpc_plan_refusal(u0, H, B, nu, limits ? u_lo : nullptr, limits ? u_hi : nullptr, n_lim)) return refuse(why);
    const bool mu_each = n_mu != 1, ter_each = rough && n_terrain != 1;
    // the candidates' rollout in the plant workspace, laid out as an open-loop rollout call of NB robots lays itself out
    const PlantRolloutCall cands{.model = model, .B = NB, .T = T, .steps_per_launch = steps_per_launch, .n_terrain = 0, .terrain = nullptr, .q0 = &stand_d,
                                 .q1 = &stand_d, .u = {u0, T, NB, 1}, .w = {nullptr, 1, 1, 1}, .mu = mu, .n_mu = mu_each ? NB : 1, .h = h, .opts = opts,
                                 .q = &stand_d, .gamma = &stand_d, .b = &stand_d, .status = &stand_i, .iters = &stand_i};

    auto* hd = new cimpc_plant_sampler_s{};
    cimpc_plant_sampler_s& S = *hd;
    S.M = M; S.C = Chost; S.Lw = plant_rollout_layout(M, cands); S.opts = *opts;
    S.rough = rough; S.mu_each = mu_each; S.ter_each = ter_each; S.limits = limits;
    S.model = model; S.B = B; S.H = H; S.L = L; S.n_x = n_x; S.N = N; S.NB = NB; S.n_iter = n_iter; S.noise_hold = noise_hold;
    S.n_rows = plant_sample_noise_rows(H, noise_hold); S.steps_per_launch = steps_per_launch; S.n_mu = n_mu; S.n_terrain = n_terrain;
    S.n_ter = !rough ? 0 : ter_each ? NB : 1; S.n_lim = limits ? n_lim : 1;
    S.mu0 = mu[0]; S.h = h; S.lam = lam; S.seed = (uint64_t)seed;
    if (limits) { S.lo.assign(u_lo, u_lo + (size_t)n_lim * nu); S.hi.assign(u_hi, u_hi + (size_t)n_lim * nu); }
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, nB = (size_t)B, nNB = (size_t)NB;
    const PlantCost reference{Q, Qf, R, x_ref, u_ref, n_Q, n_R, n_x, L, nq, nu};      // the weights, and x_ref, u_ref as the goals of L steps
    PlantCursor at;
    S.i_mu = at.take(mu_each ? nB : 0); S.i_sig = at.take((size_t)nu);
    S.i_ref = plant_cost_spans(at, reference);
    S.i_xg = at.take((size_t)(T + 1) * n_x * n); S.i_ug = at.take((size_t)T * n_x * nu);
    S.i_lo = at.take(limits ? (size_t)n_lim * nu : 0); S.i_hi = at.take(limits ? (size_t)n_lim * nu : 0);
    S.p_u[0] = at.take(TB * nu); S.p_u[1] = at.take(TB * nu);
    S.m_q = at.take((size_t)(T + 2) * B * nq); S.m_g = at.take(TB * nc); S.m_b = at.take(TB * nb);
    S.o_J = at.take((size_t)n_iter * nNB); S.o_w = at.take((size_t)n_iter * nNB); S.o_wr = at.take((size_t)n_iter * nNB);
    S.h_Jn = at.take((size_t)n_iter * B); S.h_Jb = at.take((size_t)n_iter * B);
    S.n_f = at.end();
    S.j_st = at.take(TB); S.j_it = at.take(TB); S.j_conv = at.take(nNB); S.j_ok = at.take(nNB); S.j_ch = at.take((size_t)n_iter * B);
    S.j_ne = at.take((size_t)n_iter * B); S.j_done = at.take(nB);
    S.n_i = at.end();
    std::vector<cimpc_terrain> ter;      // the candidates' terrains: robot b's for every c
    if (ter_each) for (int c = 0; c < N; ++c) ter.insert(ter.end(), terrain, terrain + B);

    int dev = 0;
    if (!plant_current_device(&dev)) { delete hd; return CIMPC_ERR_NO_DEVICE; }
    S.device = dev;
    const int rc = plant_handle_on_device(hd, [&]() {
        PlantWs* ws = plant_ws_open(dev);
        if (!ws) return false;
        bool ok_ = hipMalloc((void**)&S.F, S.n_f * sizeof(double)) == hipSuccess;
        if (!ok_) S.F = nullptr;
        if (ok_ && hipMalloc((void**)&S.I, S.n_i * sizeof(int)) != hipSuccess) { S.I = nullptr; ok_ = false; }
        if (ok_ && S.n_ter > 0 && hipMalloc((void**)&S.d_ter, (size_t)S.n_ter * sizeof(cimpc_terrain)) != hipSuccess) { S.d_ter = nullptr; ok_ = false; }
        hipStream_t st = ws->st;
        PlantStreamCopier copy{{st}, ok_};
        double* F = S.F;
        if (ok_) {
            ok_ = hipMemsetAsync(F, 0, S.n_f * sizeof(double), st) == hipSuccess && hipMemsetAsync(S.I, 0, S.n_i * sizeof(int), st) == hipSuccess;
            copy.up(F, S.i_mu, mu);      // where it is per robot
            copy.up(F, S.i_sig, sigma);
            (void)plant_cost_up(copy, F, S.i_ref, reference);
            copy.up(F, S.i_lo, u_lo); copy.up(F, S.i_hi, u_hi);
            copy.up(F, S.p_u[0], u0);
            if (rough) copy.up(S.d_ter, PlantSpan{0, (size_t)S.n_ter}, ter_each ? ter.data() : terrain);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // the host arrays are the caller's: nothing of them is read after the return
        if (!ok_) (void)smp_release(hd);
        return ok_;
    });
    if (rc != CIMPC_OK) { delete hd; return rc; }
    S.C = plant_cost_on(S.C, S.F, PlantCostSpans{S.i_ref.Q, S.i_ref.Qf, S.i_ref.R, S.i_xg, S.i_ug});      // the weights, and the goal window
    S.cur = 0; S.has_plan = true;
    *handle = hd;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_sampler_control(cimpc_plant_sampler handle, int s, int shift, const double* q0, const double* q1, double* u, double* J0,
                                           double* hist_J_nom, double* hist_J_best, int* hist_choice, int* hist_n_eligible, double* J, double* weights,
                                           int* converged) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_sampler_control", why); };
    const PlantRequired required[] = {{"handle", handle}, {"q0", q0}, {"q1", q1}, {"u", u}, {"J0", J0}, {"hist_J_nom", hist_J_nom},
                                      {"hist_J_best", hist_J_best}, {"hist_choice", hist_choice},
                                      {"hist_n_eligible", hist_n_eligible}, {"converged", converged}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
    cimpc_plant_sampler_s& S = *handle;
    if (S.failed) return refuse(SMP_FAILED);
    if (const char* why = plant_mpc_step_refusal(s, shift, S.has_plan)) return refuse(why);
    const PlantModel& M = S.M;
    const PlantRolloutLayout& Lw = S.Lw;
    const int B = S.B, H = S.H, N = S.N, NB = S.NB, nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), n_iter = S.n_iter;
    const size_t nB = (size_t)B, nNB = (size_t)NB, row = nB * nq;
    if (const char* why = plant_mpc_state_refusal(q0, q1, row)) return refuse(why);
    const int rc = plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        // the workspace grows only when another call has not yet made it as large: no allocation from the second control step on
        if (!ws || !plant_grow(&ws->d_in, &ws->cap_in, Lw.need_in) || !plant_grow(&ws->d_out, &ws->cap_out, Lw.need_out) ||
            !plant_grow(&ws->d_st, &ws->cap_st, Lw.need_st) || !plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)(S.n_ter > S.n_terrain ? S.n_ter : S.n_terrain)))
            return false;
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        bool ok_ = true;
        PlantStreamCopier copy{{st}, ok_};
        double* F = S.F;
        int* I = S.I;
        double *u_plan = S.p_u[S.cur].on(F), *u_nom = S.p_u[1 - S.cur].on(F);
        const double* d_mu = S.i_mu.or_null(F);
        copy.up(F, S.m_q.part(0, row), q0); copy.up(F, S.m_q.part(row, row), q1);      // 2 B nq doubles
        if (S.rough)      // the workspace's terrains, which another plant call may have overwritten
            ok_ = ok_ && hipMemcpyAsync(W.d_ter, S.d_ter, (size_t)S.n_ter * sizeof(cimpc_terrain), hipMemcpyDeviceToDevice, st) == hipSuccess;
        if (ok_) {
            const PlantSampleBegin Bg{u_plan, u_nom, S.i_ref.x_goal.on(F), S.i_ref.u_goal.on(F), S.i_xg.on(F), S.i_ug.on(F), B, H, S.L, S.n_x, nq, nu, s, shift};
            hipLaunchKernelGGL(plant_sample_begin_kernel, dim3((unsigned)((H + 1) * B)), dim3(LS_THREADS), 0, st, Bg);
            ok_ = hipGetLastError() == hipSuccess;
        }
        double *dq = W.d_in + Lw.q.at, *du = W.d_in + Lw.u.at, *dmu = W.d_in + Lw.mu.at, *dg = W.d_out + Lw.gamma.at, *db = W.d_out + Lw.b.at;
        int *d_st = W.d_st + Lw.status.at, *d_it = W.d_st + Lw.iters.at;
        const size_t items = (size_t)S.n_rows * nNB * nu + nNB * nq + nNB;
        for (int it = 0; it < n_iter && ok_; ++it) {
            const PlantSampleExpand E{u_nom, S.m_q.on(F), d_mu, S.i_sig.on(F), S.i_lo.or_null(F), S.i_hi.or_null(F), dq, du, dmu,
                                      S.n_lim, B, N, H, nq, nu, S.noise_hold, S.n_rows, S.seed, plant_sample_draw(s, n_iter, it)};
            hipLaunchKernelGGL(plant_sample_expand_kernel, dim3((unsigned)((items + SMP_THREADS - 1) / SMP_THREADS)), dim3(SMP_THREADS), 0, st, E);
            if (hipGetLastError() != hipSuccess) { ok_ = false; break; }
            const PlantStepArrays R{dq, du, nullptr, S.mu_each ? dmu : nullptr, dg, db, d_st, d_it, S.mu0, S.h, H, NB, 1, 1, 1, 1, S.mu_each ? NB : 1,
                                    nullptr, PlantFeedback{}, nullptr, nullptr};
            if (!plant_step_chunks(M, S.rough, S.opts, NB, H, S.steps_per_launch, R, S.rough ? W.d_ter : nullptr, S.n_ter, st)) { ok_ = false; break; }
            const size_t cand0 = (size_t)it * nNB, robot0 = (size_t)it * B;      // this iteration's rows of the per-iteration arrays
            double* Jit = S.o_J.part(cand0, nNB).on(F);
            if (!plant_candidates_cost_launch(S.C, dq, du, d_st, Jit, S.j_conv.on(I), B, NB, st)) { ok_ = false; break; }
            const PlantSampleUpdate U{Jit, S.j_conv.on(I), du, u_nom, S.i_lo.or_null(F), S.i_hi.or_null(F), S.n_lim, S.j_ok.on(I),
                                      S.o_wr.part(cand0, nNB).on(F), S.o_w.part(cand0, nNB).on(F), S.h_Jn.part(robot0, nB).on(F), S.h_Jb.part(robot0, nB).on(F),
                                      S.j_ch.part(robot0, nB).on(I), S.j_ne.part(robot0, nB).on(I),
                                      B, N, H, nu, S.lam};
            const int last = it + 1 == n_iter;
            const PlantSampleKeep K{dq, dg, db, d_st, d_it, S.m_q.on(F), S.m_g.on(F), S.m_b.on(F), S.j_st.on(I), S.j_it.on(I), S.j_done.on(I), nq, nc, nb,
                                    last && S.lam == 0.0 ? 1 : 0, last};
            hipLaunchKernelGGL(plant_sample_update_kernel, dim3((unsigned)B), dim3(SMP_THREADS), 0, st, U, K);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {      // down: what the signature names
            copy.down(u, F, S.p_u[1 - S.cur].part(0, nB * nu)); copy.down(J0, F, S.o_J.part(0, nB));
            copy.down(hist_J_nom, F, S.h_Jn); copy.down(hist_J_best, F, S.h_Jb); copy.down(hist_choice, I, S.j_ch); copy.down(hist_n_eligible, I, S.j_ne);
            copy.down(J, F, S.o_J); copy.down(weights, F, S.o_w);      // where they are asked for
            copy.down(converged, I, S.j_done);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
        return ok_;
    });
    if (rc != CIMPC_OK) return rc;
    S.cur = 1 - S.cur;      // the updated warm start is the plan now
    S.has_state = true;
    S.traj_valid = S.lam == 0.0;      // the mean has not been rolled out
    return CIMPC_OK;
}

extern "C" int cimpc_plant_sampler_plan(cimpc_plant_sampler handle, double* u, double* q, double* gamma, double* b, int* status, int* iters) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_sampler_plan", why); };
    if (!handle) return refuse("null handle");
    cimpc_plant_sampler_s& S = *handle;
    if (S.failed) return refuse(SMP_FAILED);
    if (!S.has_plan) return refuse("no plan loaded");
    const bool wants_rows = q || gamma || b || status || iters;
    return plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        hipStream_t st = ws->st;
        bool ok_ = true;
        if (wants_rows && S.has_state && !S.traj_valid) {      // one rollout of the B robots from the last (q0, q1), kept until the plan changes
            ok_ = plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)S.n_terrain) && smp_roll_plan(S, *ws, st);
            if (ok_) { S.traj_valid = true; ++S.n_rollouts; }
        }
        PlantStreamCopier copy{{st}, ok_};      // every output is optional
        copy.down(u, S.F, S.p_u[S.cur]); copy.down(q, S.F, S.m_q); copy.down(gamma, S.F, S.m_g);
        copy.down(b, S.F, S.m_b); copy.down(status, S.I, S.j_st); copy.down(iters, S.I, S.j_it);
        return (hipStreamSynchronize(st) == hipSuccess) && ok_;
    });
}

extern "C" int cimpc_plant_sampler_raw_weights(cimpc_plant_sampler handle, double* w) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_sampler_raw_weights", why); };
    if (!handle) return refuse("null handle");
    if (!w) return refuse("null w");
    cimpc_plant_sampler_s& S = *handle;
    if (S.failed) return refuse(SMP_FAILED);
    if (!S.has_state) return refuse("no control step yet");
    return plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        bool ok_ = true;
        PlantStreamCopier copy{{ws->st}, ok_};
        copy.down(w, S.F, S.o_wr);
        return (hipStreamSynchronize(ws->st) == hipSuccess) && ok_;
    });
}

extern "C" int cimpc_plant_sampler_reset(cimpc_plant_sampler handle, const double* u0) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_sampler_reset", why); };
    if (!handle) return refuse("null handle");
    if (!u0) return refuse("null u0");
    cimpc_plant_sampler_s& S = *handle;
    if (S.failed) return refuse(SMP_FAILED);
    const int nu = S.M.nu;
    if (const char* why = plant_mpc_plan_refusal(u0, S.H, S.B, nu, S.limits ? S.lo.data() : nullptr, S.limits ? S.hi.data() : nullptr, S.n_lim)) return refuse(why);
    const int rc = plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        bool ok_ = true;
        PlantStreamCopier copy{{ws->st}, ok_};
        copy.up(S.F, S.p_u[S.cur], u0);
        return (hipStreamSynchronize(ws->st) == hipSuccess) && ok_;
    });
    if (rc == CIMPC_OK) { S.has_plan = true; S.traj_valid = false; }
    return rc;
}

extern "C" int cimpc_plant_sampler_dims(cimpc_plant_sampler handle, int* model, int* B, int* H, int* L, int* N, int* n_iter, int* n_rollouts) {
    if (!handle) return CIMPC_ERR_INVALID;
    if (model) *model = handle->model;
    if (B) *B = handle->B;
    if (H) *H = handle->H;
    if (L) *L = handle->L;
    if (N) *N = handle->N;
    if (n_iter) *n_iter = handle->n_iter;
    if (n_rollouts) *n_rollouts = handle->n_rollouts;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_sampler_destroy(cimpc_plant_sampler handle) {
    using namespace cimpc;
    if (!handle) return CIMPC_OK;
    bool ok = false;
    {
        PlantDeviceScope scope(handle->device);      // no call is using the handle
        if (scope.rc() == CIMPC_OK) ok = scope.leave(smp_release(handle));
    }
    delete handle;
    return ok ? CIMPC_OK : CIMPC_ERR_HIP;
}
