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

// What a cimpc_plant_mpc points to.  F and N are the handle's doubles and ints; the members named i_*, m_*, ... are their regions (plant_staging.h).
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
    // i_ref: Q | Qf | R | x_ref | u_ref, the cost over the reference's L steps; i_xg, i_ug: the goal window of a control step
    cimpc::PlantCostSpans i_ref;
    cimpc::PlantSpan i_mu, i_al, i_lad, i_xg, i_ug, i_lo, i_hi, p_u[2], m_q, m_g, m_b, m_lq, m_lr, m_J, m_J0, m_z, g_K, g_k, g_dV, r_rho, r_Jn, o_J, o_q, o_u, o_g,
        o_b, o_lq, o_lr, o_z, h_J, h_al, h_rho;
    cimpc::PlantSpan j_st, j_it, j_lev, j_act, j_lqs, j_cut, j_cl, j_ok, j_ch, j_cst, j_cit, j_conv, j_hacc, j_nact, j_done;
    size_t n_f = 0, n_i = 0;
};

namespace {
using namespace cimpc;

// Frees what the handle owns on its device (the caller holds g_plant_mu and has selected the device).
bool mpc_release(cimpc_plant_mpc_s* h) {
    bool ok = true;
    for (auto& t : h->tapes) ok = t.release() && ok;
    ok = plant_free(&h->F) && ok;
    ok = plant_free(&h->N) && ok;
    return plant_free(&h->d_ter) && ok;
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
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_mpc_create", why); };
    if (!handle) return refuse("null handle");
    *handle = nullptr;
    const PlantRequired required[] = {{"mu", mu}, {"opts", opts}, {"Q", Q}, {"Qf", Qf}, {"R", R}, {"x_ref", x_ref}, {"u_ref", u_ref},
                                      {"alpha", alpha}, {"ladder", ladder}, {"u0", u0}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
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
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, kk = (size_t)nu * n, block = (size_t)nr * n_cols, nB = (size_t)B, traj = (size_t)(T + 2) * B * nq;
    const PlantCost reference = plant_cost_of(cost, L, nq, nu);      // the weights, and x_ref, u_ref as the goals of L steps
    PlantCursor at;
    S.i_mu = at.take(mu_each ? nB : 0); S.i_al = at.take((size_t)n_alpha); S.i_lad = at.take((size_t)n_ladder);
    S.i_ref = plant_cost_spans(at, reference);
    S.i_xg = at.take((size_t)(T + 1) * n_x * n); S.i_ug = at.take((size_t)T * n_x * nu);
    S.i_lo = at.take(limits ? (size_t)n_lim * nu : 0); S.i_hi = at.take(limits ? (size_t)n_lim * nu : 0);
    S.p_u[0] = at.take(TB * nu); S.p_u[1] = at.take(TB * nu);
    S.m_q = at.take(traj); S.m_g = at.take(TB * nc); S.m_b = at.take(TB * nb); S.m_lq = at.take((size_t)(T + 1) * B * n); S.m_lr = at.take(TB * nu);
    S.m_J = at.take(nB); S.m_J0 = at.take(nB); S.m_z = at.take(TB * nz);
    S.g_K = at.take(TB * kk); S.g_k = at.take(TB * nu); S.g_dV = at.take(2 * nB); S.r_rho = at.take(nB); S.r_Jn = at.take(nB);
    S.o_J = at.take((size_t)NB); S.o_q = at.take(traj); S.o_u = at.take(TB * nu); S.o_g = at.take(TB * nc); S.o_b = at.take(TB * nb);
    S.o_lq = at.take((size_t)(T + 1) * B * n); S.o_lr = at.take(TB * nu); S.o_z = at.take(TB * nz);
    S.h_J = at.take((size_t)n_iter * B); S.h_al = at.take((size_t)n_iter * B); S.h_rho = at.take((size_t)n_iter * B);
    S.n_f = at.end();
    S.j_st = at.take(TB); S.j_it = at.take(TB); S.j_lev = at.take(nB); S.j_act = at.take(nB); S.j_lqs = at.take(nB); S.j_cut = at.take(nB); S.j_cl = at.take(TB);
    S.j_ok = at.take((size_t)NB); S.j_ch = at.take(nB); S.j_cst = at.take(TB); S.j_cit = at.take(TB); S.j_conv = at.take((size_t)NB);
    S.j_hacc = at.take((size_t)n_iter * B); S.j_nact = at.take((size_t)n_iter); S.j_done = at.take(nB);
    S.n_i = at.end();
    const std::vector<cimpc_terrain> ter = plant_linesearch_terrains(P, terrain);      // the candidates' terrains: robot b's for every c

    int dev = 0;
    if (!plant_current_device(&dev)) { delete hd; return CIMPC_ERR_NO_DEVICE; }
    S.device = dev;
    const int rc = plant_handle_on_device(hd, [&]() {
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
        PlantStreamCopier copy{{st}, ok_};
        double* F = S.F;
        if (ok_) {
            ok_ = hipMemsetAsync(F, 0, S.n_f * sizeof(double), st) == hipSuccess && hipMemsetAsync(S.N, 0, S.n_i * sizeof(int), st) == hipSuccess;
            copy.up(F, S.i_mu, mu);      // where it is per robot
            copy.up(F, S.i_al, alpha); copy.up(F, S.i_lad, ladder);
            (void)plant_cost_up(copy, F, S.i_ref, reference);
            copy.up(F, S.i_lo, u_lo); copy.up(F, S.i_hi, u_hi);
            copy.up(F, S.p_u[0], u0);
            if (P.rough) copy.up(S.d_ter, PlantSpan{0, (size_t)P.n_ter}, P.ter_each ? ter.data() : terrain);
        }
        ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;      // the host arrays are the caller's: nothing of them is read after the return
        if (!ok_) (void)mpc_release(hd);
        return ok_;
    });
    if (rc != CIMPC_OK) { delete hd; return rc; }
    S.P.C = plant_cost_on(S.P.C, S.F, PlantCostSpans{S.i_ref.Q, S.i_ref.Qf, S.i_ref.R, S.i_xg, S.i_ug});      // the weights, and the goal window
    S.cur = 0; S.has_plan = true;
    *handle = hd;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_mpc_control(cimpc_plant_mpc handle, int s, int shift, const double* q0, const double* q1, double* u, double* J0, double* hist_J,
                                       double* hist_alpha, double* hist_rho, int* hist_accepted, int* n_done, int* converged) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_mpc_control", why); };
    const PlantRequired required[] = {{"handle", handle}, {"q0", q0}, {"q1", q1}, {"u", u}, {"J0", J0}, {"hist_J", hist_J},
                                      {"hist_alpha", hist_alpha}, {"hist_rho", hist_rho}, {"hist_accepted", hist_accepted},
                                      {"n_done", n_done}, {"converged", converged}};
    if (const char* name = plant_first_null(required)) return refuse(std::string("null ") + name);
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
    const int rc = plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        // the workspace grows only when another call has not yet made it as large: no allocation from the second control step on
        if (!ws || !plant_grow(&ws->d_in, &ws->cap_in, Lw.need_in) || !plant_grow(&ws->d_out, &ws->cap_out, Lw.need_out) ||
            !plant_grow(&ws->d_st, &ws->cap_st, Lw.need_st) || !plant_grow(&ws->d_ter, &ws->cap_ter, (size_t)P.n_ter) ||
            !plant_grow(&ws->d_z, &ws->cap_z, Lw.need_z) || !plant_grow(&ws->d_fb, &ws->cap_fb, Lw.need_fb))
            return false;
        PlantWs& W = *ws;
        hipStream_t st = W.st;
        bool ok_ = true;
        PlantStreamCopier copy{{st}, ok_};
        double* F = S.F;
        int* N = S.N;
        double *u_plan = S.p_u[S.cur].on(F), *u_nom = S.p_u[1 - S.cur].on(F);
        const double* d_mu = S.i_mu.or_null(F);
        copy.up(F, S.m_q.part(0, row), q0); copy.up(F, S.m_q.part(row, row), q1);      // 2 B nq doubles
        if (P.rough)      // the workspace's terrains, which another plant call may have overwritten
            ok_ = ok_ && hipMemcpyAsync(W.d_ter, S.d_ter, (size_t)P.n_ter * sizeof(cimpc_terrain), hipMemcpyDeviceToDevice, st) == hipSuccess;
        if (ok_) {
            const PlantMpcBegin Bg{u_plan, u_nom, S.i_ref.x_goal.on(F), S.i_ref.u_goal.on(F), S.i_xg.on(F), S.i_ug.on(F), S.j_lev.on(N), S.j_act.on(N), S.j_nact.on(N), S.h_J.on(F), S.h_al.on(F),
                                   S.h_rho.on(F), S.j_hacc.on(N), B, H, S.L, S.n_x, nq, nu, n_iter, s, shift};
            hipLaunchKernelGGL(plant_mpc_begin_kernel, dim3((unsigned)((H + 1) * B)), dim3(MPC_THREADS), 0, st, Bg);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {      // the first rollout of the control step, as cimpc_plant_rollout_tape runs it: rows are kept whether or not a step converged
            const PlantStepArrays R{S.m_q.on(F), u_nom, nullptr, d_mu, S.m_g.on(F), S.m_b.on(F), S.j_st.on(N), S.j_it.on(N), P.mu0, P.h, H, B, 1, 1, 1, 1, P.n_mu,
                                    S.m_z.on(F), PlantFeedback{}, nullptr, nullptr};
            ok_ = plant_step_chunks(M, P.rough, P.opts, B, T, P.steps_per_launch, R, P.rough ? W.d_ter : nullptr, P.rough ? P.n_terrain : 0, st);
        }
        if (ok_) {
            const PlantSensSource src{S.m_z.on(F), nullptr, S.m_q.on(F), u_nom, nullptr, d_mu, S.j_st.on(N), P.mu0, P.h, B, H, B, 1, 1, 1, 1, P.n_mu};
            ok_ = plant_sensitivity_launch(M, (int)TB, src, P.rough ? W.d_ter : nullptr, P.rough ? P.n_terrain : 0, P.reg, P.n_cols, S.tapes[0].d_dz,
                                           S.tapes[0].d_status, st);
        }
        if (ok_) {
            hipLaunchKernelGGL(plant_mpc_nominal_kernel, dim3((unsigned)B), dim3(MPC_THREADS), 0, st, P.C, (const double*)S.m_q.on(F), (const double*)u_nom,
                               S.m_lq.on(F), S.m_lr.on(F), S.m_J.on(F), S.m_J0.on(F), B);
            ok_ = hipGetLastError() == hipSuccess;
        }
        const PlantIlqrArrays A{S.i_lad.on(F), S.j_lev.on(N), S.j_act.on(N), S.m_J.on(F), S.r_rho.on(F), S.r_Jn.on(F), S.m_q.on(F), u_nom, S.m_g.on(F), S.m_b.on(F), S.m_lq.on(F),
                                S.m_lr.on(F), S.j_st.on(N), S.j_it.on(N), S.g_K.on(F), S.g_k.on(F), S.g_dV.on(F), S.j_lqs.on(N), S.j_cut.on(N), S.j_cl.on(N),
                                S.i_lo.or_null(F), S.i_hi.or_null(F), S.i_al.on(F), nullptr, d_mu, P.C, S.o_J.on(F), S.j_ok.on(N), S.j_ch.on(N),
                                S.j_conv.on(N), S.o_q.on(F), S.o_z.on(F), S.o_u.on(F), S.o_g.on(F), S.o_b.on(F), S.j_cst.on(N), S.j_cit.on(N), S.o_lq.on(F), S.o_lr.on(F),
                                S.h_J.on(F), S.h_al.on(F), S.h_rho.on(F), S.j_hacc.on(N), S.j_nact.on(N), S.rho_max, S.tol};
        for (int it = 0; it < n_iter && ok_; ++it) {      // iteration 0's parent is the warm-start nominal's buffer; then the two alternate
            const PlantTapeBuffers& parent = S.tapes[it == 0 ? 0 : 1 + ((it - 1) & 1)];
            PlantTapeBuffers& fresh = S.tapes[1 + (it & 1)];
            ok_ = plant_ilqr_iteration(P, A, it, parent.d_dz, parent.d_status, fresh.d_dz, fresh.d_status, W, st);
            int n_active = 0;      // the iteration's one read
            copy.down(&n_active, N, S.j_nact.part((size_t)it, 1));
            ok_ = (hipStreamSynchronize(st) == hipSuccess) && ok_;
            if (ok_) done = it + 1;
            if (n_active == 0) break;
        }
        if (ok_) {
            hipLaunchKernelGGL(plant_mpc_converged_kernel, dim3((unsigned)((B + MPC_THREADS - 1) / MPC_THREADS)), dim3(MPC_THREADS), 0, st,
                               (const int*)S.j_st.on(N), S.j_done.on(N), B, H);
            ok_ = hipGetLastError() == hipSuccess;
        }
        if (ok_) {      // down: what the signature names
            const size_t hn = (size_t)done * B;      // the history rows that were written
            copy.down(u, F, S.p_u[1 - S.cur].part(0, nB * nu)); copy.down(J0, F, S.m_J0);
            copy.down(hist_J, F, S.h_J.part(0, hn)); copy.down(hist_alpha, F, S.h_al.part(0, hn)); copy.down(hist_rho, F, S.h_rho.part(0, hn));
            copy.down(hist_accepted, N, S.j_hacc.part(0, hn));
            copy.down(converged, N, S.j_done);
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
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_mpc_plan", why); };
    if (!handle) return refuse("null handle");
    cimpc_plant_mpc_s& S = *handle;
    if (S.failed) return refuse(MPC_FAILED);
    if (!S.has_plan) return refuse("no plan loaded");
    return plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        hipStream_t st = ws->st;
        bool ok_ = true;
        PlantStreamCopier copy{{st}, ok_};      // every output is optional
        copy.down(u, S.F, S.p_u[S.cur]); copy.down(q, S.F, S.m_q); copy.down(gamma, S.F, S.m_g);
        copy.down(b, S.F, S.m_b); copy.down(status, S.N, S.j_st); copy.down(iters, S.N, S.j_it);
        return (hipStreamSynchronize(st) == hipSuccess) && ok_;
    });
}

extern "C" int cimpc_plant_mpc_reset(cimpc_plant_mpc handle, const double* u0) {
    using namespace cimpc;
    auto refuse = [](const std::string& why) { return plant_refuse("cimpc_plant_mpc_reset", why); };
    if (!handle) return refuse("null handle");
    if (!u0) return refuse("null u0");
    cimpc_plant_mpc_s& S = *handle;
    if (S.failed) return refuse(MPC_FAILED);
    const PlantLsPlan& P = S.P;
    const int nu = P.M.nu;
    if (const char* why = plant_mpc_plan_refusal(u0, S.H, S.B, nu, P.limits ? S.lo.data() : nullptr, P.limits ? S.hi.data() : nullptr, P.n_lim)) return refuse(why);
    const int rc = plant_handle_on_device(handle, [&]() {
        PlantWs* ws = plant_ws_open(S.device);
        if (!ws) return false;
        bool ok_ = true;
        PlantStreamCopier copy{{ws->st}, ok_};
        copy.up(S.F, S.p_u[S.cur], u0);
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
    bool ok = false;
    {
        PlantDeviceScope scope(handle->device);      // no call is using the handle
        if (scope.rc() == CIMPC_OK) ok = scope.leave(mpc_release(handle));
    }
    delete handle;
    return ok ? CIMPC_OK : CIMPC_ERR_HIP;
}
