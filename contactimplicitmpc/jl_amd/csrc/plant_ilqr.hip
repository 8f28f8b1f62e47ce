// The device-resident iLQR loop (DESIGN.md sections 3, item 3h, and 5.5): every iteration of `plant.ilqr` in ONE call.  The stages are
// the ones the host loop drives through cimpc_plant_tape_lqr_box and cimpc_plant_tape_linesearch_box, launched by the same code
// (plant_stage_launch.h) on arrays that never leave the device; between them the kernels here run the loop's rules (plant_ilqr.h):
//
//   plant_ilqr_rho_kernel       before the backward pass: rho_b[b] = ladder[level[b]]
//   plant_riccati_kernel<true, true>   with the rho array, the nominal's lin_q, lin_r and controls, and null limits when none are given
//   plant_ilqr_nominal_kernel   J_nom[b] from active, J and the backward pass's status
//   the line search's kernels   expand, the step kernel's chunks, cost, gather, ONE sensitivity launch, restore
//   plant_ilqr_commit_kernel    a workgroup per (row t, robot b): where choice[b] >= 0 the chosen rows become the nominal's (q, u_applied,
//                               gamma, b, status, iters, lin_q, lin_r), elsewhere they stay; row 0's workgroup updates level, active, J,
//                               writes the history row and counts the robot into n_active[iteration] if it is still active
//
// plant_ilqr_iteration (plant_stage_launch.h) is that body on device pointers; the entry here calls it once per iteration, and so does the
// receding-horizon policy (plant_mpc.hip), whose handle keeps the arrays between control steps.
//
// The weights, goals, limits, w, mu, the terrains (with the per-candidate copy) and the alphas go up once.  Per iteration the host reads
// ONE int, n_active, and stops at 0 as the Python loop does; everything else comes down once, at the end.  Two tape buffers are
// allocated once and alternate (iteration 1's parent is the caller's tape, which is only read); the final one is returned, the other freed.
// These kernels move rows and run short ordered chains: the time of an iteration is the step kernel's and the Riccati kernel's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

// No fused multiply-adds in this translation unit: the rules round as the NumPy lines of plant.ilqr do.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_boxqp.h"
#include "plant_cost.h"
#include "plant_ilqr.h"
#include "plant_model.h"
#include "plant_riccati.h"
#include "plant_stage_launch.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

constexpr int ILQR_THREADS = 64;

__global__ __launch_bounds__(ILQR_THREADS) void plant_ilqr_rho_kernel(const double* ladder, const int* level, double* rho_b, int B) {
    const int b = blockIdx.x * ILQR_THREADS + threadIdx.x;
    if (b < B) rho_b[b] = plant_ilqr_rho(ladder, level[b]);
}

__global__ __launch_bounds__(ILQR_THREADS) void plant_ilqr_nominal_kernel(const int* active, const double* J, const int* lq_status, double* J_nom, int B) {
    const int b = blockIdx.x * ILQR_THREADS + threadIdx.x;
    if (b < B) J_nom[b] = plant_ilqr_nominal_cost(active[b], lq_status[b], J[b]);
}

// Row t (0 .. T+1) of robot b: the line search's chosen rows (C*) into the nominal's (N*) where the robot has an acceptable candidate
struct PlantIlqrCommit {
    const int* choice;
    const double *Cq, *Cu, *Cg, *Cb, *Clq, *Clr;
    const int *Cst, *Cit;
    double *Nq, *Nu, *Ng, *Nb, *Nlq, *Nlr;
    int *Nst, *Nit;
    const double *J_cand, *alpha, *ladder;      // NB, n_alpha, n_ladder
    int *level, *active;
    double* J;
    double *hist_J, *hist_alpha, *hist_rho;     // this iteration's rows of B
    int *hist_accepted, *n_active;              // this iteration's row of B, and its word
    double rho_max, tol;
    int B, T, nq, nu, nc, nb;
};

__global__ __launch_bounds__(ILQR_THREADS) void plant_ilqr_commit_kernel(PlantIlqrCommit P) {
    const int e = blockIdx.x, lane = threadIdx.x, T = P.T, B = P.B;
    if (e >= (T + 2) * B) return;
    const int t = e / B, b = e % B, nq = P.nq, nu = P.nu, n = 2 * nq, choice = P.choice[b];
    if (t == 0 && lane == 0) {      // nothing else in this launch reads or writes the robot's state
        PlantIlqrRobot s{P.level[b], P.active[b], P.J[b]};
        const PlantIlqrRow row = plant_ilqr_update(&s, choice, P.J_cand + b, (size_t)B, P.alpha, P.ladder, P.rho_max, P.tol);
        P.level[b] = s.level; P.active[b] = s.active; P.J[b] = s.J;
        P.hist_J[b] = row.J; P.hist_alpha[b] = row.alpha; P.hist_rho[b] = row.rho; P.hist_accepted[b] = row.accepted;
        if (s.active) atomicAdd(P.n_active, 1);
    }
    if (choice < 0) return;
    const size_t at = (size_t)t * B + b;
    for (int i = lane; i < nq; i += ILQR_THREADS) P.Nq[at * nq + i] = P.Cq[at * nq + i];
    if (t > T) return;
    for (int i = lane; i < n; i += ILQR_THREADS) P.Nlq[at * n + i] = P.Clq[at * n + i];
    if (t == T) return;
    for (int i = lane; i < nu; i += ILQR_THREADS) { P.Nu[at * nu + i] = P.Cu[at * nu + i]; P.Nlr[at * nu + i] = P.Clr[at * nu + i]; }
    for (int i = lane; i < P.nc; i += ILQR_THREADS) P.Ng[at * P.nc + i] = P.Cg[at * P.nc + i];
    for (int i = lane; i < P.nb; i += ILQR_THREADS) P.Nb[at * P.nb + i] = P.Cb[at * P.nb + i];
    if (lane == 0) { P.Nst[at] = P.Cst[at]; P.Nit[at] = P.Cit[at]; }
}

bool plant_ilqr_iteration(const PlantLsPlan& P, const PlantIlqrArrays& A, int it, const double* parent_dz, const int* parent_status, double* dz,
                          int* status, PlantWs& W, hipStream_t st) {
    const PlantModel& M = P.M;
    const PlantCost& C = A.C;
    const int B = P.B, T = P.T, nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), nr = nq + nc + nb;
    const unsigned rows = (unsigned)((B + ILQR_THREADS - 1) / ILQR_THREADS);
    hipLaunchKernelGGL(plant_ilqr_rho_kernel, dim3(rows), dim3(ILQR_THREADS), 0, st, A.ladder, A.level, A.rho_b, B);
    if (hipGetLastError() != hipSuccess) return false;
    PlantRiccati R{parent_dz, parent_status, C.Q, C.Qf, C.R, A.Nlq, A.Nlr, A.K, A.k, nullptr, nullptr, A.dV,
                   A.lq_status, A.n_cut, B, T, nq, nu, nr, P.n_cols, 1, C.n_Q, C.n_R, T, 0.0};
    R.rho_b = A.rho_b; R.n_rho = B; R.clamped = A.clamped;
    if (P.limits) { R.u_lo = A.u_lo; R.u_hi = A.u_hi; R.u_nom = A.Nu; R.n_lim = P.n_lim; }
    if (!plant_riccati_box_launch(R, st)) return false;
    hipLaunchKernelGGL(plant_ilqr_nominal_kernel, dim3(rows), dim3(ILQR_THREADS), 0, st, A.active, A.J, A.lq_status, A.J_nom, B);
    if (hipGetLastError() != hipSuccess) return false;
    const PlantLsArrays S{A.Nq, A.Nu, A.k, A.K, A.w, A.mu, A.dV, A.J_nom, A.alpha, A.u_lo, A.u_hi, C, A.J_cand, A.ok, A.choice, A.conv, A.Cq, A.Cz,
                          A.Cu, A.Cg, A.Cb, A.Cst, A.Cit, A.Clq, A.Clr, parent_dz, parent_status, dz, status};
    if (!plant_linesearch_stages(P, S, W, st)) return false;
    const size_t row = (size_t)it * B;
    const PlantIlqrCommit Cm{A.choice, A.Cq, A.Cu, A.Cg, A.Cb, A.Clq, A.Clr, A.Cst, A.Cit, A.Nq, A.Nu, A.Ng, A.Nb, A.Nlq, A.Nlr, A.Nst, A.Nit,
                             A.J_cand, A.alpha, A.ladder, A.level, A.active, A.J, A.hist_J + row, A.hist_alpha + row, A.hist_rho + row,
                             A.hist_accepted + row, A.n_active + it, A.rho_max, A.tol, B, T, nq, nu, nc, nb};
    hipLaunchKernelGGL(plant_ilqr_commit_kernel, dim3((unsigned)((T + 2) * B)), dim3(ILQR_THREADS), 0, st, Cm);
    return hipGetLastError() == hipSuccess;
}

namespace {
// grow-only device buffers of the entry, per device, next to the plant workspace whose buffers (the candidates' rollout), stream and
// mutex it uses: every double and every int of the loop
struct IlqrWs { double* d_f = nullptr; int* d_i = nullptr; size_t cap_f = 0, cap_i = 0; };
IlqrWs g_ilqr_ws[PLANT_MAX_DEVICES];
}  // namespace

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int cimpc_plant_ilqr(cimpc_plant_tape tape, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain, const double* q_nom,
                                const double* u_nom, const double* gamma_nom, const double* b_nom, const int* status_nom, const int* iters_nom,
                                const double* J_nom, const double* lin_q_nom, const double* lin_r_nom, const double* w, int K_w, int n_w, int hold_w,
                                const double* mu, int n_mu, double h, const cimpc_ip_opts* opts, const cimpc_tracking_cost* cost, int n_alpha,
                                const double* alpha, double armijo, double reg, int n_ladder, const double* ladder, double rho_max, double tol,
                                int max_iter, int n_lim, const double* u_lo, const double* u_hi, double* q, double* u_applied, double* gamma,
                                double* b, int* status, int* iters, double* lin_q, double* lin_r, int* grad_status, double* hist_J,
                                double* hist_alpha, double* hist_rho, int* hist_accepted, int* n_iter, double* K, double* k, double* dV,
                                int* lq_status, int* n_cut, int* clamped, cimpc_plant_tape* new_tape) {
    using namespace cimpc;
    // every refusal leaves its reason where cimpc_last_error(NULL) finds it; what needs no tape is tested before the tape is looked at
    auto refuse = [](const std::string& why) { set_global_error("cimpc_plant_ilqr: " + why); return CIMPC_ERR_INVALID; };
    if (!new_tape) return refuse("null new_tape");
    *new_tape = nullptr;
    const std::pair<const char*, const void*> required[] = {
        {"tape", tape}, {"q_nom", q_nom}, {"u_nom", u_nom}, {"gamma_nom", gamma_nom}, {"b_nom", b_nom}, {"status_nom", status_nom}, {"iters_nom", iters_nom},
        {"J_nom", J_nom}, {"lin_q_nom", lin_q_nom}, {"lin_r_nom", lin_r_nom}, {"mu", mu}, {"opts", opts}, {"cost", cost}, {"alpha", alpha},
        {"ladder", ladder}, {"q", q}, {"u_applied", u_applied}, {"gamma", gamma}, {"b", b}, {"status", status}, {"iters", iters}, {"lin_q", lin_q},
        {"lin_r", lin_r}, {"grad_status", grad_status}, {"hist_J", hist_J}, {"hist_alpha", hist_alpha}, {"hist_rho", hist_rho},
        {"hist_accepted", hist_accepted}, {"n_iter", n_iter}};
    for (const auto& [name, p] : required) if (!p) return refuse(std::string("null ") + name);
    if (const char* why = plant_ilqr_refusal(max_iter, n_ladder, ladder, rho_max, tol)) return refuse(why);
    // what cimpc_plant_tape_linesearch_box refuses
    PlantLsPlan P;
    if (const char* why = plant_linesearch_plan(PlantLsCall{tape, steps_per_launch, n_terrain, terrain, q_nom, u_nom, w, K_w, n_w, hold_w, mu, n_mu, h, opts,
                                                            n_alpha, alpha, armijo, cost, reg, q, u_applied, gamma, b, status, iters, grad_status, n_lim,
                                                            u_lo, u_hi}, &P))
        return refuse(why);
    const PlantTapeBuffers& caller = tape->buf;
    const PlantModel& M = P.M;
    const PlantRolloutLayout& L = P.L;
    PlantCost C = P.C;
    const int B = P.B, T = P.T, n_cols = P.n_cols, nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), nz = M.nz(), nw = M.nw, nr = nq + nc + nb, NB = P.NB;
    const bool limits = P.limits, w_each = P.w_each, mu_each = P.mu_each;
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, kk = (size_t)nu * n, block = (size_t)nr * n_cols, nB = (size_t)B;
    // what cimpc_plant_tape_lqr_box refuses of a limited pass with linear terms, one lap and every step's gains kept
    if (n_cols < 2 * nq + nu || !plant_riccati_fits(nq, nu)) return refuse("a model without controls, or a tape without the control columns");
    if (nu > PLANT_BOXQP_MAX_M || plant_riccati_box_lds(nq, nu) > PLANT_RIC_MAX_LDS) return refuse("a model too large for the limited pass");
    if (T > (1 << 30)) return refuse("laps T beyond 2^30");
    auto finite = [](const double* a, size_t cnt) { for (size_t i = 0; i < cnt; ++i) if (!std::isfinite(a[i])) return false; return true; };
    if (!finite(q_nom, (size_t)(T + 2) * B * nq)) return refuse("a non-finite entry of q_nom");
    if (!finite(u_nom, TB * nu)) return refuse("a non-finite entry of u_nom");

    // the doubles: what goes up once | the nominal | the gains | the rules' rows | the line search's outputs | the history
    size_t at = 0;
    auto next = [&at](size_t cnt) { const size_t o = at; at += cnt; return o; };
    const size_t i_w = next(w_each ? (size_t)K_w * B * nw : 0), i_mu = next(mu_each ? nB : 0), i_al = next((size_t)n_alpha), i_lad = next((size_t)n_ladder),
                 i_Q = next((size_t)C.n_Q * n * n), i_Qf = next(n * n), i_R = next((size_t)C.n_R * nu * nu), i_xg = next((size_t)(T + 1) * C.n_x * n),
                 i_ug = next((size_t)T * C.n_x * nu), i_lo = next(limits ? (size_t)n_lim * nu : 0), i_hi = next(limits ? (size_t)n_lim * nu : 0);
    const size_t m_q = next((size_t)(T + 2) * B * nq), m_u = next(TB * nu), m_g = next(TB * nc), m_b = next(TB * nb), m_lq = next((size_t)(T + 1) * B * n),
                 m_lr = next(TB * nu), m_J = next(nB);
    const size_t g_K = next(TB * kk), g_k = next(TB * nu), g_dV = next(2 * nB), r_rho = next(nB), r_Jn = next(nB);
    const size_t o_J = next((size_t)NB), o_q = next((size_t)(T + 2) * B * nq), o_u = next(TB * nu), o_g = next(TB * nc), o_b = next(TB * nb),
                 o_lq = next((size_t)(T + 1) * B * n), o_lr = next(TB * nu), o_z = next(TB * nz);
    const size_t h_J = next((size_t)max_iter * B), h_al = next((size_t)max_iter * B), h_rho = next((size_t)max_iter * B), n_f = at;
    at = 0;      // the integers
    const size_t j_st = next(TB), j_it = next(TB), j_lev = next(nB), j_act = next(nB), j_lqs = next(nB), j_cut = next(nB), j_cl = next(TB),
                 j_ok = next((size_t)NB), j_ch = next(nB), j_cst = next(TB), j_cit = next(TB), j_conv = next((size_t)NB), j_hacc = next((size_t)max_iter * B),
                 j_nact = next((size_t)max_iter), n_i = at;
    const std::vector<cimpc_terrain> ter = plant_linesearch_terrains(P, terrain);      // the candidates' terrains: robot b's for every c
    const std::vector<int> ones(nB, 1);

    std::lock_guard<std::mutex> lock(g_plant_mu);
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return CIMPC_ERR_NO_DEVICE;
    const int dev = caller.device;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return CIMPC_ERR_HIP;
    bool ok_ = false;
    int done = 0;
    PlantTapeBuffers bufs[2];      // iteration i writes bufs[i & 1] and reads bufs[(i - 1) & 1] (iteration 0: the caller's tape)
    PlantWs* ws = plant_ws_open(dev);
    IlqrWs& S = g_ilqr_ws[dev];
    if (ws && plant_grow(&ws->d_in, &ws->cap_in, L.need_in) && plant_grow(&ws->d_out, &ws->cap_out, L.need_out) && plant_grow(&ws->d_st, &ws->cap_st, L.need_st) &&
        plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)P.n_ter) && plant_grow(&ws->d_z, &ws->cap_z, L.need_z) && plant_grow(&ws->d_fb, &ws->cap_fb, L.need_fb) &&
        plant_grow(&S.d_f, &S.cap_f, n_f) && plant_grow(&S.d_i, &S.cap_i, n_i)) {
        ok_ = true;
        for (int s = 0; s < (max_iter > 1 ? 2 : 1) && ok_; ++s) {      // the tapes' memory, the last to be allocated
            bufs[s].device = dev; bufs[s].M = M;
            ok_ = hipMalloc((void**)&bufs[s].d_dz, TB * block * sizeof(double)) == hipSuccess;
            if (ok_ && hipMalloc((void**)&bufs[s].d_status, TB * sizeof(int)) != hipSuccess) { bufs[s].d_status = nullptr; ok_ = false; }
        }
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        auto up = [&](auto* d, const auto* hsrc, size_t cnt) { ok_ = ok_ && hipMemcpyAsync(d, hsrc, cnt * sizeof(*d), hipMemcpyHostToDevice, st) == hipSuccess; };
        auto down = [&](auto* hdst, const auto* d, size_t cnt) { ok_ = ok_ && hipMemcpyAsync(hdst, d, cnt * sizeof(*d), hipMemcpyDeviceToHost, st) == hipSuccess; };
        double* F = S.d_f;
        int* N = S.d_i;
        // up, once
        if (w_each) up(F + i_w, w, (size_t)K_w * B * nw);
        if (mu_each) up(F + i_mu, mu, nB);
        up(F + i_al, alpha, (size_t)n_alpha); up(F + i_lad, ladder, (size_t)n_ladder);
        up(F + i_Q, C.Q, (size_t)C.n_Q * n * n); up(F + i_Qf, C.Qf, n * n); up(F + i_R, C.R, (size_t)C.n_R * nu * nu);
        up(F + i_xg, C.x_goal, (size_t)(T + 1) * C.n_x * n); up(F + i_ug, C.u_goal, (size_t)T * C.n_x * nu);
        if (limits) { up(F + i_lo, u_lo, (size_t)n_lim * nu); up(F + i_hi, u_hi, (size_t)n_lim * nu); }
        up(F + m_q, q_nom, (size_t)(T + 2) * B * nq); up(F + m_u, u_nom, TB * nu); up(F + m_g, gamma_nom, TB * nc); up(F + m_b, b_nom, TB * nb);
        up(F + m_lq, lin_q_nom, (size_t)(T + 1) * B * n); up(F + m_lr, lin_r_nom, TB * nu); up(F + m_J, J_nom, nB);
        up(N + j_st, status_nom, TB); up(N + j_it, iters_nom, TB); up(N + j_act, ones.data(), nB);
        ok_ = ok_ && hipMemsetAsync(N + j_lev, 0, nB * sizeof(int), st) == hipSuccess && hipMemsetAsync(N + j_nact, 0, (size_t)max_iter * sizeof(int), st) == hipSuccess;
        ok_ = ok_ && plant_linesearch_shared(P, w, terrain, ter, W, st);
        C.Q = F + i_Q; C.Qf = F + i_Qf; C.R = F + i_R; C.x_goal = F + i_xg; C.u_goal = F + i_ug;
        const PlantIlqrArrays A{F + i_lad, N + j_lev, N + j_act, F + m_J, F + r_rho, F + r_Jn, F + m_q, F + m_u, F + m_g, F + m_b, F + m_lq, F + m_lr,
                                N + j_st, N + j_it, F + g_K, F + g_k, F + g_dV, N + j_lqs, N + j_cut, N + j_cl, limits ? F + i_lo : nullptr,
                                limits ? F + i_hi : nullptr, F + i_al, w_each ? F + i_w : nullptr, mu_each ? F + i_mu : nullptr, C, F + o_J, N + j_ok,
                                N + j_ch, N + j_conv, F + o_q, F + o_z, F + o_u, F + o_g, F + o_b, N + j_cst, N + j_cit, F + o_lq, F + o_lr,
                                F + h_J, F + h_al, F + h_rho, N + j_hacc, N + j_nact, rho_max, tol};
        for (int it = 0; it < max_iter && ok_; ++it) {
            const PlantTapeBuffers& parent = it == 0 ? caller : bufs[(it - 1) & 1];
            PlantTapeBuffers& fresh = bufs[it & 1];
            ok_ = plant_ilqr_iteration(P, A, it, parent.d_dz, parent.d_status, fresh.d_dz, fresh.d_status, W, st);
            int n_active = 0;      // the iteration's one read
            down(&n_active, N + j_nact + it, (size_t)1);
            ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;
            if (ok_) done = it + 1;
            if (n_active == 0) break;
        }
        if (ok_) {      // down, once
            const PlantTapeBuffers& last = bufs[(done - 1) & 1];
            const size_t hn = (size_t)done * B;
            down(q, F + m_q, (size_t)(T + 2) * B * nq); down(u_applied, F + m_u, TB * nu); down(gamma, F + m_g, TB * nc); down(b, F + m_b, TB * nb);
            down(lin_q, F + m_lq, (size_t)(T + 1) * B * n); down(lin_r, F + m_lr, TB * nu); down(status, N + j_st, TB); down(iters, N + j_it, TB);
            down(grad_status, last.d_status, TB);
            down(hist_J, F + h_J, hn); down(hist_alpha, F + h_al, hn); down(hist_rho, F + h_rho, hn); down(hist_accepted, N + j_hacc, hn);
            if (K) down(K, F + g_K, TB * kk);
            if (k) down(k, F + g_k, TB * nu);
            if (dV) down(dV, F + g_dV, 2 * nB);
            if (lq_status) down(lq_status, N + j_lqs, nB);
            if (n_cut) down(n_cut, N + j_cut, nB);
            if (clamped) down(clamped, N + j_cl, TB);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
    }
    const int keep = ok_ ? (done - 1) & 1 : -1;
    for (int s = 0; s < 2; ++s)
        if (s != keep) ok_ = bufs[s].release() && ok_;
    if (!ok_ && keep >= 0) (void)bufs[keep].release();
    if (cur != dev) {
        const bool back = hipSetDevice(cur) == hipSuccess;
        if (!back && ok_) (void)bufs[keep].release();
        ok_ = back && ok_;
    }
    if (!ok_) return CIMPC_ERR_HIP;
    *n_iter = done;
    *new_tape = new cimpc_plant_tape_s{bufs[keep], tape->model, B, T, n_cols};
    return CIMPC_OK;
}
