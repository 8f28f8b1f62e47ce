// The receding-horizon iLQR policy (DESIGN.md sections 3, item 3j, and 5.5): a handle that keeps the problem and the plan of B robots on
// the device between control steps, so that a control step moves 2 B nq doubles up and one control row, the diagnostics and one int per
// iteration down.  A control step is, bit for bit, `plant.ilqr(device_loop=True)` on the goal window of step s from the shifted plan:
//
//   the start rows up             q[0] = q0, q[1] = q1 into the nominal's trajectory
//   plant_mpc_begin_kernel        a workgroup per (row t, robot b): the shifted plan into the nominal's control rows, the goal window of step s
//                                 into the cost's x_goal / u_goal (n_x columns), level 0, active 1, the n_active words and the history rows cleared
//   the first rollout             plant_step_chunks (the open-loop step kernel) on the nominal's own arrays, then ONE plant_sensitivity_launch
//                                 into the warm-start tape buffer, as cimpc_plant_rollout_tape makes them
//   plant_mpc_nominal_kernel      a wavefront per robot: J0, lin_q, lin_r of the nominal by plant_cost_trajectory (cimpc_plant_tracking_cost's bits)
//   n_iter x plant_ilqr_iteration the loop body of cimpc_plant_ilqr (plant_stage_launch.h); one int read per iteration, stop at 0 active
//   plant_mpc_converged_kernel    a work item per robot: whether every step of the final nominal converged
//
// The index rules are plant_mpc.h's.  The plan lives in two control buffers that alternate, so a shift never reads a row it writes.  The
// shared plant workspace is scratch for the candidates' rollout; the terrains another plant call may overwrite there are copied back in,
// device to device, at every control step from the handle's own.  These kernels move rows and run the ordered chains of plant_cost.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

// No fused multiply-adds in this translation unit: the cost rounds as cimpc_plant_tracking_cost does.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_boxqp.h"
#include "plant_cost.h"
#include "plant_ilqr.h"
#include "plant_model.h"
#include "plant_mpc.h"
#include "plant_riccati.h"
#include "plant_sensitivity.h"
#include "plant_stage_launch.h"
#include "plant_step_launch.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

constexpr int MPC_THREADS = LS_THREADS;

struct PlantMpcBegin {
    const double* u_plan;      // H x B x nu
    double* u_nom;
    const double *x_ref, *u_ref;      // (L + 1) x n_x x n, L x n_x x nu
    double *x_goal, *u_goal;          // (H + 1) x n_x x n, H x n_x x nu
    int *level, *active, *n_active;   // B, B, n_iter
    double *hist_J, *hist_alpha, *hist_rho;      // n_iter x B
    int* hist_accepted;
    int B, H, L, n_x, nq, nu, n_iter, s, shift;
};

__global__ __launch_bounds__(MPC_THREADS) void plant_mpc_begin_kernel(PlantMpcBegin P) {
    const int e = blockIdx.x, lane = threadIdx.x, B = P.B, H = P.H;
    if (e >= (H + 1) * B) return;
    const int t = e / B, b = e % B;
    if (t < H) plant_mpc_warm_start(P.u_nom, P.u_plan, t, b, P.shift, H, B, P.nu, lane, MPC_THREADS);
    if (b < P.n_x) plant_mpc_window(P.x_goal, P.u_goal, P.x_ref, P.u_ref, P.s, t, b, H, P.L, P.n_x, 2 * P.nq, P.nu, lane, MPC_THREADS);
    if (t != 0) return;
    if (lane == 0) plant_mpc_reset_robot(P.level + b, P.active + b);
    for (int it = lane; it < P.n_iter; it += MPC_THREADS) {
        const size_t at = (size_t)it * B + b;
        P.hist_J[at] = 0.0; P.hist_alpha[at] = 0.0; P.hist_rho[at] = 0.0; P.hist_accepted[at] = 0;
        if (b == 0) P.n_active[it] = 0;
    }
}

// J0[b], J[b] and the nominal's lin_q (H + 1) x B x n, lin_r H x B x nu from its q (H + 2) x B x nq and u H x B x nu
__global__ __launch_bounds__(MPC_THREADS) void plant_mpc_nominal_kernel(PlantCost C, const double* q, const double* u, double* lin_q, double* lin_r,
                                                                        double* J, double* J0, int B) {
    __shared__ double work[LS_MAX_WORK];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int nq = C.nq, nu = C.nu;
    const size_t n = (size_t)2 * nq;
    PlantCostWave team;
    const double Jb = plant_cost_trajectory(C, C.n_x == 1 ? 0 : b, q + (size_t)b * nq, (size_t)B * nq, u + (size_t)b * nu, (size_t)B * nu, work,
                                            lin_q + (size_t)b * n, (size_t)B * n, lin_r + (size_t)b * nu, (size_t)B * nu, team);
    if (threadIdx.x == 0) { J[b] = Jb; J0[b] = Jb; }
}

__global__ __launch_bounds__(MPC_THREADS) void plant_mpc_converged_kernel(const int* status, int* converged, int B, int H) {
    const int b = blockIdx.x * MPC_THREADS + threadIdx.x;
    if (b >= B) return;
    int all = 1;
    for (int t = 0; t < H; ++t) all &= status[(size_t)t * B + b] != 0;
    converged[b] = all;
}

}  // namespace cimpc

// What a cimpc_plant_mpc points to.  F and N are the handle's doubles and ints; the members named i_*, m_*, ... are offsets into them.
struct cimpc_plant_mpc_s {
    cimpc::PlantLsPlan P;
    int device = -1, model = 0, B = 0, H = 0, L = 0, n_x = 1, n_iter = 0;
    double rho_max = 0.0, tol = 0.0;
    bool has_plan = false, failed = false;
    int cur = 0;      // which of the two control buffers holds the plan
    double* F = nullptr;
    int* N = nullptr;
    cimpc_terrain* d_ter = nullptr;      // the candidates' terrains (P.n_ter), whose first n_terrain are the robots'
    cimpc::PlantTapeBuffers tapes[3];    // the warm-start nominal's, and the two that alternate
    std::vector<double> lo, hi;          // the limits on the host (n_lim x nu; empty: none), for the plans cimpc_plant_mpc_reset is given
    // doubles: the problem | the plan's two control buffers | the nominal | the gains | the rules' rows | the line search's outputs | the history
    size_t i_mu, i_al, i_lad, i_Q, i_Qf, i_R, i_xr, i_ur, i_xg, i_ug, i_lo, i_hi, p_u[2], m_q, m_g, m_b, m_lq, m_lr, m_J, m_J0, m_z, g_K, g_k, g_dV, r_rho,
        r_Jn, o_J, o_q, o_u, o_g, o_b, o_lq, o_lr, o_z, h_J, h_al, h_rho, n_f;
    size_t j_st, j_it, j_lev, j_act, j_lqs, j_cut, j_cl, j_ok, j_ch, j_cst, j_cit, j_conv, j_hacc, j_nact, j_done, n_i;
};

namespace {
using namespace cimpc;

int mpc_refuse(const char* entry, const std::string& why) {
    set_global_error(std::string(entry) + ": " + why);
    return CIMPC_ERR_INVALID;
}

// Frees what the handle owns on its device (the caller holds g_plant_mu and has selected the device).
bool mpc_release(cimpc_plant_mpc_s* h) {
    bool ok = true;
    for (auto& t : h->tapes) ok = t.release() && ok;
    if (h->F) ok = (hipFree(h->F) == hipSuccess) && ok;
    if (h->N) ok = (hipFree(h->N) == hipSuccess) && ok;
    if (h->d_ter) ok = (hipFree(h->d_ter) == hipSuccess) && ok;
    h->F = nullptr; h->N = nullptr; h->d_ter = nullptr;
    return ok;
}

// Runs `body` under the plant mutex on the handle's device; the current device is restored.
template <class Body>
int mpc_on_device(cimpc_plant_mpc_s* h, Body&& body) {
    std::lock_guard<std::mutex> lock(g_plant_mu);
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return CIMPC_ERR_NO_DEVICE;
    if (cur != h->device && hipSetDevice(h->device) != hipSuccess) return CIMPC_ERR_HIP;
    bool ok = body();
    if (cur != h->device) ok = (hipSetDevice(cur) == hipSuccess) && ok;
    if (!ok) h->failed = true;
    return ok ? CIMPC_OK : CIMPC_ERR_HIP;
}

const char* const MPC_FAILED = "a handle that met a HIP error refuses further use";
}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int cimpc_plant_mpc_create(int model, int B, int H, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain, const double* mu, int n_mu,
                                      double h, const cimpc_ip_opts* opts, const double* Q, const double* Qf, const double* R, int n_Q, int n_R, int L,
                                      int n_x, const double* x_ref, const double* u_ref, int n_alpha, const double* alpha, double armijo, double reg,
                                      int n_cols, int n_ladder, const double* ladder, double rho_max, double tol, int n_iter, int n_lim,
                                      const double* u_lo, const double* u_hi, const double* u0, cimpc_plant_mpc* handle) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return mpc_refuse("cimpc_plant_mpc_create", why); };
    if (!handle) return refuse("null handle");
    *handle = nullptr;
    const std::pair<const char*, const void*> required[] = {{"mu", mu}, {"opts", opts}, {"Q", Q}, {"Qf", Qf}, {"R", R}, {"x_ref", x_ref}, {"u_ref", u_ref},
                                                            {"alpha", alpha}, {"ladder", ladder}, {"u0", u0}};
    for (const auto& [name, p] : required) if (!p) return refuse(std::string("null ") + name);
    if (const char* why = plant_mpc_problem_refusal(H, L, n_iter)) return refuse(why);
    if (const char* why = plant_ilqr_refusal(n_iter, n_ladder, ladder, rho_max, tol)) return refuse(why);
    // the stand-in for the parent tape of cimpc_plant_ilqr: its sizes and model; its memory is the handle's, allocated below
    static double stand_d;
    static int stand_i;
    cimpc_plant_tape_s shape{};
    if (!plant_model_by_id(model, &shape.buf.M)) return refuse("an unknown model");
    shape.buf.device = 0; shape.buf.d_dz = &stand_d; shape.buf.d_status = &stand_i;
    shape.model = model; shape.B = B; shape.T = H; shape.n_cols = n_cols;
    if (B < 1) return refuse("B below 1");
    const cimpc_tracking_cost cost{Q, Qf, R, x_ref, u_ref, n_Q, n_R, n_x};
    double* const outd = &stand_d;      // the outputs of a line search call: only that they are given is looked at
    int* const outi = &stand_i;
    PlantLsPlan P;
    if (const char* why = plant_linesearch_plan(PlantLsCall{&shape, steps_per_launch, n_terrain, terrain, u0, u0, nullptr, 1, 1, 1, mu, n_mu, h, opts, n_alpha,
                                                            alpha, armijo, &cost, reg, outd, outd, outd, outd, outi, outi, outi, n_lim, u_lo, u_hi}, &P))
        return refuse(why);
    const PlantModel& M = P.M;
    const int nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), nz = M.nz(), nr = nq + nc + nb, NB = P.NB, T = H;
    if (n_cols < 2 * nq + nu || !plant_riccati_fits(nq, nu)) return refuse("a model without controls, or a tape without the control columns");
    if (nu > PLANT_BOXQP_MAX_M || plant_riccati_box_lds(nq, nu) > PLANT_RIC_MAX_LDS) return refuse("a model too large for the limited pass");
    if (T > (1 << 30)) return refuse("laps T beyond 2^30");
    if ((long long)L + 1 > (1LL << 30) / ((long long)n_x * 2 * nq)) return refuse("a reference beyond 2^30 doubles");
    if (const char* why = plant_mpc_plan_refusal(u0, H, B, nu, P.limits ? u_lo : nullptr, P.limits ? u_hi : nullptr, n_lim)) return refuse(why);

    auto* hd = new cimpc_plant_mpc_s{};
    cimpc_plant_mpc_s& S = *hd;
    S.P = P; S.model = model; S.B = B; S.H = H; S.L = L; S.n_x = n_x; S.n_iter = n_iter;
    S.rho_max = rho_max; S.tol = tol;
    const bool limits = P.limits, mu_each = P.mu_each;
    if (limits) { S.lo.assign(u_lo, u_lo + (size_t)n_lim * nu); S.hi.assign(u_hi, u_hi + (size_t)n_lim * nu); }
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, kk = (size_t)nu * n, block = (size_t)nr * n_cols, nB = (size_t)B;
    size_t at = 0;
    auto next = [&at](size_t cnt) { const size_t o = at; at += cnt; return o; };
    S.i_mu = next(mu_each ? nB : 0); S.i_al = next((size_t)n_alpha); S.i_lad = next((size_t)n_ladder); S.i_Q = next((size_t)n_Q * n * n); S.i_Qf = next(n * n);
    S.i_R = next((size_t)n_R * nu * nu); S.i_xr = next((size_t)(L + 1) * n_x * n); S.i_ur = next((size_t)L * n_x * nu);
    S.i_xg = next((size_t)(T + 1) * n_x * n); S.i_ug = next((size_t)T * n_x * nu); S.i_lo = next(limits ? (size_t)n_lim * nu : 0);
    S.i_hi = next(limits ? (size_t)n_lim * nu : 0);
    S.p_u[0] = next(TB * nu); S.p_u[1] = next(TB * nu);
    S.m_q = next((size_t)(T + 2) * B * nq); S.m_g = next(TB * nc); S.m_b = next(TB * nb); S.m_lq = next((size_t)(T + 1) * B * n); S.m_lr = next(TB * nu);
    S.m_J = next(nB); S.m_J0 = next(nB); S.m_z = next(TB * nz);
    S.g_K = next(TB * kk); S.g_k = next(TB * nu); S.g_dV = next(2 * nB); S.r_rho = next(nB); S.r_Jn = next(nB);
    S.o_J = next((size_t)NB); S.o_q = next((size_t)(T + 2) * B * nq); S.o_u = next(TB * nu); S.o_g = next(TB * nc); S.o_b = next(TB * nb);
    S.o_lq = next((size_t)(T + 1) * B * n); S.o_lr = next(TB * nu); S.o_z = next(TB * nz);
    S.h_J = next((size_t)n_iter * B); S.h_al = next((size_t)n_iter * B); S.h_rho = next((size_t)n_iter * B); S.n_f = at;
    at = 0;
    S.j_st = next(TB); S.j_it = next(TB); S.j_lev = next(nB); S.j_act = next(nB); S.j_lqs = next(nB); S.j_cut = next(nB); S.j_cl = next(TB);
    S.j_ok = next((size_t)NB); S.j_ch = next(nB); S.j_cst = next(TB); S.j_cit = next(TB); S.j_conv = next((size_t)NB); S.j_hacc = next((size_t)n_iter * B);
    S.j_nact = next((size_t)n_iter); S.j_done = next(nB); S.n_i = at;
    const std::vector<cimpc_terrain> ter = plant_linesearch_terrains(P, terrain);      // the candidates' terrains: robot b's for every c

    int dev = 0;
    if (!plant_current_device(&dev)) { delete hd; return CIMPC_ERR_NO_DEVICE; }
    S.device = dev;
    const int rc = mpc_on_device(hd, [&]() {
        PlantWs* ws = plant_ws_open(dev);
        if (!ws) return false;
        bool ok_ = hipMalloc((void**)&S.F, S.n_f * sizeof(double)) == hipSuccess;
        if (!ok_) S.F = nullptr;
        if (ok_ && hipMalloc((void**)&S.N, S.n_i * sizeof(int)) != hipSuccess) { S.N = nullptr; ok_ = false; }
        if (ok_ && P.n_ter > 0 && hipMalloc((void**)&S.d_ter, (size_t)P.n_ter * sizeof(cimpc_terrain)) != hipSuccess) { S.d_ter = nullptr; ok_ = false; }
        for (auto& t : S.tapes) {
            if (!ok_) break;
            t.device = dev; t.M = M;
            if (hipMalloc((void**)&t.d_dz, TB * block * sizeof(double)) != hipSuccess) { t.d_dz = nullptr; ok_ = false; }
            if (ok_ && hipMalloc((void**)&t.d_status, TB * sizeof(int)) != hipSuccess) { t.d_status = nullptr; ok_ = false; }
        }
        hipStream_t st = ws->st;
        auto up = [&](auto* d, const auto* hsrc, size_t cnt) { ok_ = ok_ && hipMemcpyAsync(d, hsrc, cnt * sizeof(*d), hipMemcpyHostToDevice, st) == hipSuccess; };
        double* F = S.F;
        if (ok_) {
            ok_ = hipMemsetAsync(F, 0, S.n_f * sizeof(double), st) == hipSuccess && hipMemsetAsync(S.N, 0, S.n_i * sizeof(int), st) == hipSuccess;
            if (mu_each) up(F + S.i_mu, mu, nB);
            up(F + S.i_al, alpha, (size_t)n_alpha); up(F + S.i_lad, ladder, (size_t)n_ladder);
            up(F + S.i_Q, Q, (size_t)n_Q * n * n); up(F + S.i_Qf, Qf, n * n); up(F + S.i_R, R, (size_t)n_R * nu * nu);
            up(F + S.i_xr, x_ref, (size_t)(L + 1) * n_x * n); up(F + S.i_ur, u_ref, (size_t)L * n_x * nu);
            if (limits) { up(F + S.i_lo, u_lo, (size_t)n_lim * nu); up(F + S.i_hi, u_hi, (size_t)n_lim * nu); }
            up(F + S.p_u[0], u0, TB * nu);
            if (P.rough) up(S.d_ter, P.ter_each ? ter.data() : terrain, (size_t)P.n_ter);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // the host arrays are the caller's: nothing of them is read after the return
        if (!ok_) (void)mpc_release(hd);
        return ok_;
    });
    if (rc != CIMPC_OK) { delete hd; return rc; }
    S.P.C.Q = S.F + S.i_Q; S.P.C.Qf = S.F + S.i_Qf; S.P.C.R = S.F + S.i_R; S.P.C.x_goal = S.F + S.i_xg; S.P.C.u_goal = S.F + S.i_ug;
    S.cur = 0; S.has_plan = true;
    *handle = hd;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_mpc_control(cimpc_plant_mpc handle, int s, int shift, const double* q0, const double* q1, double* u, double* J0, double* hist_J,
                                       double* hist_alpha, double* hist_rho, int* hist_accepted, int* n_done, int* converged) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return mpc_refuse("cimpc_plant_mpc_control", why); };
    const std::pair<const char*, const void*> required[] = {{"handle", handle}, {"q0", q0}, {"q1", q1}, {"u", u}, {"J0", J0}, {"hist_J", hist_J},
                                                            {"hist_alpha", hist_alpha}, {"hist_rho", hist_rho}, {"hist_accepted", hist_accepted},
                                                            {"n_done", n_done}, {"converged", converged}};
    for (const auto& [name, p] : required) if (!p) return refuse(std::string("null ") + name);
    cimpc_plant_mpc_s& S = *handle;
    if (S.failed) return refuse(MPC_FAILED);
    if (const char* why = plant_mpc_step_refusal(s, shift, S.has_plan)) return refuse(why);
    const PlantLsPlan& P = S.P;
    const PlantModel& M = P.M;
    const PlantRolloutLayout& Lw = P.L;
    const int B = S.B, H = S.H, T = H, nq = M.nq, nu = M.nu, n_iter = S.n_iter;
    const size_t TB = (size_t)T * B, nB = (size_t)B, row = nB * nq;
    if (const char* why = plant_mpc_state_refusal(q0, q1, row)) return refuse(why);
    int done = 0;
    const int rc = mpc_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        // the workspace grows only when another call has not yet made it as large: no allocation from the second control step on
        if (!ws || !plant_grow(&ws->d_in, &ws->cap_in, Lw.need_in) || !plant_grow(&ws->d_out, &ws->cap_out, Lw.need_out) ||
            !plant_grow(&ws->d_st, &ws->cap_st, Lw.need_st) || !plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)P.n_ter) ||
            !plant_grow(&ws->d_z, &ws->cap_z, Lw.need_z) || !plant_grow(&ws->d_fb, &ws->cap_fb, Lw.need_fb))
            return false;
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        bool ok_ = true;
        auto up = [&](auto* d, const auto* hsrc, size_t cnt) { ok_ = ok_ && hipMemcpyAsync(d, hsrc, cnt * sizeof(*d), hipMemcpyHostToDevice, st) == hipSuccess; };
        auto down = [&](auto* hdst, const auto* d, size_t cnt) { ok_ = ok_ && hipMemcpyAsync(hdst, d, cnt * sizeof(*d), hipMemcpyDeviceToHost, st) == hipSuccess; };
        double* F = S.F;
        int* N = S.N;
        double *u_plan = F + S.p_u[S.cur], *u_nom = F + S.p_u[1 - S.cur];
        const double* d_mu = P.mu_each ? F + S.i_mu : nullptr;
        up(F + S.m_q, q0, row); up(F + S.m_q + row, q1, row);      // up: 2 B nq doubles
        if (P.rough)      // the workspace's terrains, which another plant call may have overwritten
            ok_ = ok_ && hipMemcpyAsync(W.d_ter, S.d_ter, (size_t)P.n_ter * sizeof(cimpc_terrain), hipMemcpyDeviceToDevice, st) == hipSuccess;
        if (ok_) {
            const PlantMpcBegin Bg{u_plan, u_nom, F + S.i_xr, F + S.i_ur, F + S.i_xg, F + S.i_ug, N + S.j_lev, N + S.j_act, N + S.j_nact, F + S.h_J, F + S.h_al,
                                   F + S.h_rho, N + S.j_hacc, B, H, S.L, S.n_x, nq, nu, n_iter, s, shift};
            hipLaunchKernelGGL(plant_mpc_begin_kernel, dim3((unsigned)((H + 1) * B)), dim3(MPC_THREADS), 0, st, Bg);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {      // the first rollout of the control step, as cimpc_plant_rollout_tape runs it: rows are kept whether or not a step converged
            const PlantStepArrays R{F + S.m_q, u_nom, nullptr, d_mu, F + S.m_g, F + S.m_b, N + S.j_st, N + S.j_it, P.mu0, P.h, H, B, 1, 1, 1, 1, P.n_mu,
                                    F + S.m_z, PlantFeedback{}, nullptr, nullptr};
            ok_ = plant_step_chunks(M, P.rough, P.opts, B, T, P.steps_per_launch, R, P.rough ? W.d_ter : nullptr, P.rough ? P.n_terrain : 0, st);
        }
        if (ok_) {
            const PlantSensSource src{F + S.m_z, nullptr, F + S.m_q, u_nom, nullptr, d_mu, N + S.j_st, P.mu0, P.h, B, H, B, 1, 1, 1, 1, P.n_mu};
            ok_ = plant_sensitivity_launch(M, (int)TB, src, P.rough ? W.d_ter : nullptr, P.rough ? P.n_terrain : 0, P.reg, P.n_cols, S.tapes[0].d_dz,
                                           S.tapes[0].d_status, st);
        }
        if (ok_) {
            hipLaunchKernelGGL(plant_mpc_nominal_kernel, dim3((unsigned)B), dim3(MPC_THREADS), 0, st, P.C, (const double*)(F + S.m_q), (const double*)u_nom,
                               F + S.m_lq, F + S.m_lr, F + S.m_J, F + S.m_J0, B);
            ok_ = hipGetLastError() == hipSuccess;
        }
        const bool limits = P.limits;
        const PlantIlqrArrays A{F + S.i_lad, N + S.j_lev, N + S.j_act, F + S.m_J, F + S.r_rho, F + S.r_Jn, F + S.m_q, u_nom, F + S.m_g, F + S.m_b, F + S.m_lq,
                                F + S.m_lr, N + S.j_st, N + S.j_it, F + S.g_K, F + S.g_k, F + S.g_dV, N + S.j_lqs, N + S.j_cut, N + S.j_cl,
                                limits ? F + S.i_lo : nullptr, limits ? F + S.i_hi : nullptr, F + S.i_al, nullptr, d_mu, P.C, F + S.o_J, N + S.j_ok, N + S.j_ch,
                                N + S.j_conv, F + S.o_q, F + S.o_z, F + S.o_u, F + S.o_g, F + S.o_b, N + S.j_cst, N + S.j_cit, F + S.o_lq, F + S.o_lr,
                                F + S.h_J, F + S.h_al, F + S.h_rho, N + S.j_hacc, N + S.j_nact, S.rho_max, S.tol};
        for (int it = 0; it < n_iter && ok_; ++it) {      // iteration 0's parent is the warm-start nominal's buffer; then the two alternate
            const PlantTapeBuffers& parent = S.tapes[it == 0 ? 0 : 1 + ((it - 1) & 1)];
            PlantTapeBuffers& fresh = S.tapes[1 + (it & 1)];
            ok_ = plant_ilqr_iteration(P, A, it, parent.d_dz, parent.d_status, fresh.d_dz, fresh.d_status, W, st);
            int n_active = 0;      // the iteration's one read
            down(&n_active, N + S.j_nact + it, (size_t)1);
            ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;
            if (ok_) done = it + 1;
            if (n_active == 0) break;
        }
        if (ok_) {
            hipLaunchKernelGGL(plant_mpc_converged_kernel, dim3((unsigned)((B + MPC_THREADS - 1) / MPC_THREADS)), dim3(MPC_THREADS), 0, st,
                               (const int*)(N + S.j_st), N + S.j_done, B, H);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {      // down: what the signature names
            const size_t hn = (size_t)done * B;
            down(u, u_nom, nB * nu); down(J0, F + S.m_J0, nB);
            down(hist_J, F + S.h_J, hn); down(hist_alpha, F + S.h_al, hn); down(hist_rho, F + S.h_rho, hn); down(hist_accepted, N + S.j_hacc, hn);
            down(converged, N + S.j_done, nB);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
        return ok_;
    });
    if (rc != CIMPC_OK) return rc;
    S.cur = 1 - S.cur;      // the nominal is the plan now
    *n_done = done;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_mpc_plan(cimpc_plant_mpc handle, double* u, double* q, double* gamma, double* b, int* status, int* iters) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return mpc_refuse("cimpc_plant_mpc_plan", why); };
    if (!handle) return refuse("null handle");
    cimpc_plant_mpc_s& S = *handle;
    if (S.failed) return refuse(MPC_FAILED);
    if (!S.has_plan) return refuse("no plan loaded");
    const PlantModel& M = S.P.M;
    const size_t TB = (size_t)S.H * S.B;
    return mpc_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        hipStream_t st = ws->st;
        bool ok_ = true;
        auto down = [&](auto* hdst, const auto* d, size_t cnt) {
            if (hdst) ok_ = ok_ && hipMemcpyAsync(hdst, d, cnt * sizeof(*d), hipMemcpyDeviceToHost, st) == hipSuccess;
        };
        down(u, S.F + S.p_u[S.cur], TB * M.nu); down(q, S.F + S.m_q, (size_t)(S.H + 2) * S.B * M.nq); down(gamma, S.F + S.m_g, TB * M.nc);
        down(b, S.F + S.m_b, TB * M.nb()); down(status, S.N + S.j_st, TB); down(iters, S.N + S.j_it, TB);
        return (hipStreamSynchronize(st) == hipSuccess) && ok_;
    });
}

extern "C" int cimpc_plant_mpc_reset(cimpc_plant_mpc handle, const double* u0) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return mpc_refuse("cimpc_plant_mpc_reset", why); };
    if (!handle) return refuse("null handle");
    if (!u0) return refuse("null u0");
    cimpc_plant_mpc_s& S = *handle;
    if (S.failed) return refuse(MPC_FAILED);
    const PlantLsPlan& P = S.P;
    const int nu = P.M.nu;
    if (const char* why = plant_mpc_plan_refusal(u0, S.H, S.B, nu, P.limits ? S.lo.data() : nullptr, P.limits ? S.hi.data() : nullptr, P.n_lim)) return refuse(why);
    const size_t cnt = (size_t)S.H * S.B * nu;
    const int rc = mpc_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        const bool ok_ = hipMemcpyAsync(S.F + S.p_u[S.cur], u0, cnt * sizeof(double), hipMemcpyHostToDevice, ws->st) == hipSuccess;
        return (hipStreamSynchronize(ws->st) == hipSuccess) && ok_;
    });
    if (rc == CIMPC_OK) S.has_plan = true;
    return rc;
}

extern "C" int cimpc_plant_mpc_dims(cimpc_plant_mpc handle, int* model, int* B, int* H, int* L, int* n_iter) {
    if (!handle) return CIMPC_ERR_INVALID;
    if (model) *model = handle->model;
    if (B) *B = handle->B;
    if (H) *H = handle->H;
    if (L) *L = handle->L;
    if (n_iter) *n_iter = handle->n_iter;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_mpc_destroy(cimpc_plant_mpc handle) {
    using namespace cimpc;
    if (!handle) return CIMPC_OK;
    bool ok = true;
    {
        std::lock_guard<std::mutex> lock(g_plant_mu);      // no call is using the handle
        int cur = -1;
        const int dev = handle->device;
        ok = hipGetDevice(&cur) == hipSuccess && (cur == dev || hipSetDevice(dev) == hipSuccess);
        if (ok) {
            ok = mpc_release(handle);
            if (cur != dev) ok = (hipSetDevice(cur) == hipSuccess) && ok;
        }
    }
    delete handle;
    return ok ? CIMPC_OK : CIMPC_ERR_HIP;
}
