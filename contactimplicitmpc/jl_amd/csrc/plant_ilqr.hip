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
// the entry's own buffers, beside the candidates' rollout in the plant workspace: every double of the loop in d_in, every int in d_int
PlantStageWs g_ilqr_ws[PLANT_MAX_DEVICES];
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
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_ilqr", why); };
    if (!new_tape) return refuse("null new_tape");
    *new_tape = nullptr;
    const PlantRequired required[] = {
        {"tape", tape}, {"q_nom", q_nom}, {"u_nom", u_nom}, {"gamma_nom", gamma_nom}, {"b_nom", b_nom}, {"status_nom", status_nom}, {"iters_nom", iters_nom},
        {"J_nom", J_nom}, {"lin_q_nom", lin_q_nom}, {"lin_r_nom", lin_r_nom}, {"mu", mu}, {"opts", opts}, {"cost", cost}, {"alpha", alpha},
        {"ladder", ladder}, {"q", q}, {"u_applied", u_applied}, {"gamma", gamma}, {"b", b}, {"status", status}, {"iters", iters}, {"lin_q", lin_q},
        {"lin_r", lin_r}, {"grad_status", grad_status}, {"hist_J", hist_J}, {"hist_alpha", hist_alpha}, {"hist_rho", hist_rho},
        {"hist_accepted", hist_accepted}, {"n_iter", n_iter}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
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
    const int B = P.B, T = P.T, n_cols = P.n_cols, nq = M.nq, nu = M.nu, nc = M.nc, nb = M.nb(), nz = M.nz(), nw = M.nw, nr = nq + nc + nb, NB = P.NB;
    const bool limits = P.limits, w_each = P.w_each, mu_each = P.mu_each;
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, kk = (size_t)nu * n, block = (size_t)nr * n_cols, nB = (size_t)B, traj = (size_t)(T + 2) * B * nq;
    // what cimpc_plant_tape_lqr_box refuses of a limited pass with linear terms, one lap and every step's gains kept
    if (n_cols < 2 * nq + nu || !plant_riccati_fits(nq, nu)) return refuse("a model without controls, or a tape without the control columns");
    if (nu > PLANT_BOXQP_MAX_M || plant_riccati_box_lds(nq, nu) > PLANT_RIC_MAX_LDS) return refuse("a model too large for the limited pass");
    if (T > (1 << 30)) return refuse("laps T beyond 2^30");
    if (!plant_all_finite(q_nom, traj)) return refuse("a non-finite entry of q_nom");
    if (!plant_all_finite(u_nom, TB * nu)) return refuse("a non-finite entry of u_nom");

    // the doubles: what goes up once | the nominal | the gains | the rules' rows | the line search's outputs | the history
    PlantCursor at;
    const PlantSpan i_w = at.take(w_each ? (size_t)K_w * B * nw : 0), i_mu = at.take(mu_each ? nB : 0), i_al = at.take((size_t)n_alpha),
                    i_lad = at.take((size_t)n_ladder);
    const PlantCostSpans i_cost = plant_cost_spans(at, P.C);
    const PlantSpan i_lo = at.take(limits ? (size_t)n_lim * nu : 0), i_hi = at.take(limits ? (size_t)n_lim * nu : 0);
    const PlantSpan m_q = at.take(traj), m_u = at.take(TB * nu), m_g = at.take(TB * nc), m_b = at.take(TB * nb), m_lq = at.take((size_t)(T + 1) * B * n),
                    m_lr = at.take(TB * nu), m_J = at.take(nB);
    const PlantSpan g_K = at.take(TB * kk), g_k = at.take(TB * nu), g_dV = at.take(2 * nB), r_rho = at.take(nB), r_Jn = at.take(nB);
    const PlantSpan o_J = at.take((size_t)NB), o_q = at.take(traj), o_u = at.take(TB * nu), o_g = at.take(TB * nc), o_b = at.take(TB * nb),
                    o_lq = at.take((size_t)(T + 1) * B * n), o_lr = at.take(TB * nu), o_z = at.take(TB * nz);
    const PlantSpan h_J = at.take((size_t)max_iter * B), h_al = at.take((size_t)max_iter * B), h_rho = at.take((size_t)max_iter * B);
    const size_t n_f = at.end();
    // the integers
    const PlantSpan j_st = at.take(TB), j_it = at.take(TB), j_lev = at.take(nB), j_act = at.take(nB), j_lqs = at.take(nB), j_cut = at.take(nB), j_cl = at.take(TB),
                    j_ok = at.take((size_t)NB), j_ch = at.take(nB), j_cst = at.take(TB), j_cit = at.take(TB), j_conv = at.take((size_t)NB),
                    j_hacc = at.take((size_t)max_iter * B), j_nact = at.take((size_t)max_iter);
    const size_t n_i = at.end();
    const std::vector<cimpc_terrain> ter = plant_linesearch_terrains(P, terrain);      // the candidates' terrains: robot b's for every c
    const std::vector<int> ones(nB, 1);

    const int dev = caller.device;
    PlantDeviceScope scope(dev);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok_ = false;
    int done = 0;
    PlantTapeBuffers bufs[2];      // iteration i writes bufs[i & 1] and reads bufs[(i - 1) & 1] (iteration 0: the caller's tape)
    PlantWs* ws = plant_ws_open(dev);
    PlantStageWs& S = g_ilqr_ws[dev];
    if (ws && plant_grow(&ws->d_in, &ws->cap_in, L.need_in) && plant_grow(&ws->d_out, &ws->cap_out, L.need_out) && plant_grow(&ws->d_st, &ws->cap_st, L.need_st) &&
        plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)P.n_ter) && plant_grow(&ws->d_z, &ws->cap_z, L.need_z) && plant_grow(&ws->d_fb, &ws->cap_fb, L.need_fb) &&
        S.grow(n_f, 0, n_i)) {
        ok_ = true;
        for (int s = 0; s < (max_iter > 1 ? 2 : 1) && ok_; ++s) {      // the tapes' memory, the last to be allocated
            bufs[s].device = dev; bufs[s].M = M;
            ok_ = hipMalloc((void**)&bufs[s].d_dz, TB * block * sizeof(double)) == hipSuccess;
            if (ok_ && hipMalloc((void**)&bufs[s].d_status, TB * sizeof(int)) != hipSuccess) { bufs[s].d_status = nullptr; ok_ = false; }
        }
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        PlantStreamCopier copy{{st}, ok_};
        double* F = S.d_in;
        int* N = S.d_int;
        // the problem and the nominal go to the device, once
        copy.up(F, i_w, w); copy.up(F, i_mu, mu);      // where they are per robot
        copy.up(F, i_al, alpha); copy.up(F, i_lad, ladder);
        const PlantCost C = plant_cost_up(copy, F, i_cost, P.C);
        copy.up(F, i_lo, u_lo); copy.up(F, i_hi, u_hi);
        copy.up(F, m_q, q_nom); copy.up(F, m_u, u_nom); copy.up(F, m_g, gamma_nom); copy.up(F, m_b, b_nom);
        copy.up(F, m_lq, lin_q_nom); copy.up(F, m_lr, lin_r_nom); copy.up(F, m_J, J_nom);
        copy.up(N, j_st, status_nom); copy.up(N, j_it, iters_nom); copy.up(N, j_act, ones.data());
        ok_ = ok_ && hipMemsetAsync(j_lev.on(N), 0, j_lev.n * sizeof(int), st) == hipSuccess && hipMemsetAsync(j_nact.on(N), 0, j_nact.n * sizeof(int), st) == hipSuccess;
        ok_ = ok_ && plant_linesearch_shared(P, w, terrain, ter, W, st);
        const PlantIlqrArrays A{i_lad.on(F), j_lev.on(N), j_act.on(N), m_J.on(F), r_rho.on(F), r_Jn.on(F), m_q.on(F), m_u.on(F), m_g.on(F), m_b.on(F), m_lq.on(F),
                                m_lr.on(F), j_st.on(N), j_it.on(N), g_K.on(F), g_k.on(F), g_dV.on(F), j_lqs.on(N), j_cut.on(N), j_cl.on(N), i_lo.or_null(F),
                                i_hi.or_null(F), i_al.on(F), i_w.or_null(F), i_mu.or_null(F), C, o_J.on(F), j_ok.on(N), j_ch.on(N), j_conv.on(N), o_q.on(F),
                                o_z.on(F), o_u.on(F), o_g.on(F), o_b.on(F), j_cst.on(N), j_cit.on(N), o_lq.on(F), o_lr.on(F), h_J.on(F), h_al.on(F),
                                h_rho.on(F), j_hacc.on(N), j_nact.on(N), rho_max, tol};
        for (int it = 0; it < max_iter && ok_; ++it) {
            const PlantTapeBuffers& parent = it == 0 ? caller : bufs[(it - 1) & 1];
            PlantTapeBuffers& fresh = bufs[it & 1];
            ok_ = plant_ilqr_iteration(P, A, it, parent.d_dz, parent.d_status, fresh.d_dz, fresh.d_status, W, st);
            int n_active = 0;      // the iteration's one read
            copy.down(&n_active, N, j_nact.part((size_t)it, 1));
            ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;
            if (ok_) done = it + 1;
            if (n_active == 0) break;
        }
        if (ok_) {      // down, once
            const PlantTapeBuffers& last = bufs[(done - 1) & 1];
            const size_t hn = (size_t)done * B;      // the history rows that were written
            copy.down(q, F, m_q); copy.down(u_applied, F, m_u); copy.down(gamma, F, m_g); copy.down(b, F, m_b);
            copy.down(lin_q, F, m_lq); copy.down(lin_r, F, m_lr); copy.down(status, N, j_st); copy.down(iters, N, j_it);
            copy.down(grad_status, last.d_status, PlantSpan{0, TB});
            copy.down(hist_J, F, h_J.part(0, hn)); copy.down(hist_alpha, F, h_al.part(0, hn)); copy.down(hist_rho, F, h_rho.part(0, hn));
            copy.down(hist_accepted, N, j_hacc.part(0, hn));
            copy.down(K, F, g_K); copy.down(k, F, g_k); copy.down(dV, F, g_dV);      // the optional outputs: where they are given
            copy.down(lq_status, N, j_lqs); copy.down(n_cut, N, j_cut); copy.down(clamped, N, j_cl);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // this stream only
    }
    const int keep = ok_ ? (done - 1) & 1 : -1;
    for (int s = 0; s < 2; ++s)
        if (s != keep) ok_ = bufs[s].release() && ok_;
    if (!ok_ && keep >= 0) (void)bufs[keep].release();
    if (!scope.leave(ok_)) {
        if (ok_) (void)bufs[keep].release();      // the device could not be restored: the new tape does not outlive the call
        return CIMPC_ERR_HIP;
    }
    *n_iter = done;
    *new_tape = new cimpc_plant_tape_s{bufs[keep], tape->model, B, T, n_cols};
    return CIMPC_OK;
}
