// A loss backpropagated through a device rollout (DESIGN.md sections 3, item 3b, and 5.5): the tape of a rollout's step gradients,
// kept on the device, and the reverse chain over it.
//
//   cimpc_plant_rollout_tape   cimpc_plant_rollout_grad whose sensitivity launch writes dz and its status into device memory the tape
//                              owns (plant_rollout_to_tape, plant_kernel.hip); dz never crosses the bus
//   cimpc_plant_tape_vjp       cotangents (gq, ggamma, gb) up, ONE launch of plant_adjoint_kernel, the small gradients down
//   cimpc_plant_rollout_tape_feedback, cimpc_plant_tape_vjp_feedback   the two for a closed-loop rollout (plant_feedback.h): the tape also
//                              owns the gain rows, the chain runs the feedback statements and returns g_xref_step when asked to
//   cimpc_plant_rollout_tape_feedback_limits   the closed loop under control limits (item 3i): the tape also owns the mask of clamped
//                              controls, and cimpc_plant_tape_vjp_feedback on it launches the third instantiation of the chain
//
// plant_adjoint_kernel: a workgroup of one wavefront per robot walks t = T-1 .. 0 through the statements of plant_adjoint.h.  D_t
// (nr x n_cols doubles, column-major as the sensitivity kernel wrote it) sits in LDS, loaded by the whole wavefront with consecutive
// lanes on consecutive doubles; block t-1 is loaded into registers before step t's arithmetic and stored to the other LDS buffer after
// it (the blocks do not depend on the chain), the first STAGE_DOUBLES doubles per lane that way and whatever a larger block has left at
// the store.  a = [lambda[t+2]; ggamma[t]; gb[t]] and the three live rows of lambda are in LDS too; lane c owns columns c, c + 64, ...
// and adds its column's nr terms in ascending r.  Only lambda[0], lambda[1] and the per-step outputs reach global memory.
#include <hip/hip_runtime.h>
#include <climits>
#include <mutex>
#include <new>
#include <string>

// No fused multiply-adds in this translation unit: the chain rounds as the float64 restatement of the definition does, whatever the
// compiler would make of `v += d * a`.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_adjoint.h"
#include "plant_model.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

constexpr int ADJ_THREADS = 64;
constexpr int STAGE_DOUBLES = 32;      // per lane: a block of up to 2048 doubles is wholly in flight during a step

// the wavefront as the team of plant_adjoint.h
struct PlantAdjointWave {
    double stage[STAGE_DOUBLES];
    __device__ int rank() const { return threadIdx.x; }
    __device__ int size() const { return ADJ_THREADS; }
    __device__ void sync() const { __syncthreads(); }
    __device__ void fetch_issue(const double* src, int n) {
#pragma unroll
        for (int k = 0; k < STAGE_DOUBLES; ++k) {
            const int i = k * ADJ_THREADS + (int)threadIdx.x;
            stage[k] = i < n ? src[i] : 0.0;
        }
    }
    __device__ void fetch_commit(double* dst, const double* src, int n) {
#pragma unroll
        for (int k = 0; k < STAGE_DOUBLES; ++k) {
            const int i = k * ADJ_THREADS + (int)threadIdx.x;
            if (i < n) dst[i] = stage[k];
        }
        for (int i = STAGE_DOUBLES * ADJ_THREADS + (int)threadIdx.x; i < n; i += ADJ_THREADS) dst[i] = src[i];
    }
};

// FB: PLANT_CHAIN_OPEN, PLANT_CHAIN_LOOP (a closed-loop tape's chain, with the feedback statements of plant_feedback.h) or
// PLANT_CHAIN_CLAMP (a limited closed-loop tape's, which also reads the tape's mask of clamped controls)
template <int FB>
__global__ __launch_bounds__(ADJ_THREADS) void plant_adjoint_kernel(PlantAdjoint P) {
    extern __shared__ __attribute__((aligned(16))) double adj_lds[];      // plant_adjoint_lds(nr, n_cols, nq), + plant_adjoint_feedback_doubles with P.fb.K
    const int rb = blockIdx.x;
    if (rb >= P.B) return;                                                 // uniform over the workgroup
    PlantAdjointWave team;
    plant_adjoint_chain_as<FB>(P, rb, adj_lds, team);
}

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
namespace {
// A rollout whose call asks for a tape (call.grad->tape): *tape is the new tape, or null when the call is refused or fails.
int rollout_tape_impl(const cimpc::PlantRolloutCall& call, cimpc_plant_tape* tape) {
    if (!tape) return CIMPC_ERR_INVALID;
    *tape = nullptr;
    cimpc::PlantTapeBuffers buf;
    const int rc = cimpc::plant_rollout_to_tape(call, &buf);
    if (rc != CIMPC_OK) return rc;
    *tape = new cimpc_plant_tape_s{buf, call.model, call.B, call.T, call.grad->n_cols};
    return CIMPC_OK;
}
}  // namespace

extern "C" int cimpc_plant_rollout_tape_feedback(int model, int B, int T, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                                 const double* q0, const double* q1, const double* u, int K_u, int n_u, int hold_u,
                                                 const double* w, int K_w, int n_w, int hold_w, const double* mu, int n_mu, double h,
                                                 const cimpc_ip_opts* opts, double* q, double* gamma, double* b, int* status, int* iters,
                                                 double reg, int n_cols, double* z, int* grad_status, cimpc_plant_tape* tape,
                                                 const cimpc_feedback* fb, double* u_applied, double* fb_err) {
    return rollout_tape_impl({PLANT_ROLLOUT_CALL_BASE, .grad = cimpc::PlantRolloutGrad{reg, n_cols, z, nullptr, grad_status, true},
                              .loop = cimpc::PlantRolloutLoop{fb, u_applied, fb_err}}, tape);
}

// cimpc_plant_rollout_tape_feedback under control limits: the rollout runs under the limited law, the tape
// also owns the mask of clamped controls, and the words come back in clamped (T x B).  Every refusal of the limits leaves its reason for
// cimpc_last_error(NULL), before any device is touched.
extern "C" int cimpc_plant_rollout_tape_feedback_limits(int model, int B, int T, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                                        const double* q0, const double* q1, const double* u, int K_u, int n_u, int hold_u,
                                                        const double* w, int K_w, int n_w, int hold_w, const double* mu, int n_mu, double h,
                                                        const cimpc_ip_opts* opts, double* q, double* gamma, double* b, int* status, int* iters,
                                                        double reg, int n_cols, double* z, int* grad_status, cimpc_plant_tape* tape,
                                                        const cimpc_feedback* fb, double* u_applied, double* fb_err, int n_lim, const double* u_lo,
                                                        const double* u_hi, int* clamped) {
    const cimpc::PlantRolloutLoop loop{fb, u_applied, fb_err, u_lo, u_hi, n_lim, clamped};
    if (const char* why = cimpc::plant_limits_refusal(model, B, loop, true)) {
        if (tape) *tape = nullptr;
        cimpc::set_global_error(std::string("cimpc_plant_rollout_tape_feedback_limits: ") + why);
        return CIMPC_ERR_INVALID;
    }
    const int rc = rollout_tape_impl({PLANT_ROLLOUT_CALL_BASE, .grad = cimpc::PlantRolloutGrad{reg, n_cols, z, nullptr, grad_status, true}, .loop = loop}, tape);
    if (rc == CIMPC_ERR_INVALID) cimpc::set_global_error("cimpc_plant_rollout_tape_feedback_limits: an argument that cimpc_plant_rollout_tape_feedback refuses");
    return rc;
}

extern "C" int cimpc_plant_rollout_tape(int model, int B, int T, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain,
                                        const double* q0, const double* q1, const double* u, int K_u, int n_u, int hold_u, const double* w,
                                        int K_w, int n_w, int hold_w, const double* mu, int n_mu, double h, const cimpc_ip_opts* opts,
                                        double* q, double* gamma, double* b, int* status, int* iters, double reg, int n_cols, double* z,
                                        int* grad_status, cimpc_plant_tape* tape) {
    return rollout_tape_impl({PLANT_ROLLOUT_CALL_BASE, .grad = cimpc::PlantRolloutGrad{reg, n_cols, z, nullptr, grad_status, true}}, tape);
}

extern "C" int cimpc_plant_tape_dims(cimpc_plant_tape tape, int* model, int* B, int* T, int* n_cols) {
    if (!tape) return CIMPC_ERR_INVALID;
    if (model) *model = tape->model;
    if (B) *B = tape->B;
    if (T) *T = tape->T;
    if (n_cols) *n_cols = tape->n_cols;
    return CIMPC_OK;
}

extern "C" int cimpc_plant_tape_destroy(cimpc_plant_tape tape) {
    using namespace cimpc;
    if (!tape) return CIMPC_OK;
    bool ok = false;
    {
        PlantDeviceScope scope(tape->buf.device);      // no call is walking the tape
        if (scope.rc() == CIMPC_OK) ok = scope.leave(tape->buf.release());
    }
    delete tape;
    return ok ? CIMPC_OK : CIMPC_ERR_HIP;
}

// Validate (no device needed), then on the tape's device and the plant workspace's private stream: one upload (gq | ggamma | gb, those
// given), one launch, one read-back (g_q0 | g_q1 | g_u_step | g_w_step | g_mu | g_h, n_cut), one synchronize.  A closed-loop tape's chain always runs the
// feedback statements; g_xref_step (T x B x 2nq, may be null) is theirs and is refused on an open-loop tape.  A tape that owns a mask of
// clamped controls (cimpc_plant_rollout_tape_feedback_limits) launches the PLANT_CHAIN_CLAMP instantiation, which needs no more LDS.
extern "C" int cimpc_plant_tape_vjp_feedback(cimpc_plant_tape tape, const double* gq, const double* ggamma, const double* gb, double* g_q0,
                                    double* g_q1, double* g_u_step, double* g_w_step, double* g_mu, double* g_h, int* n_cut,
                                    double* g_xref_step) {
    using namespace cimpc;
    if (!tape || (!gq && !ggamma && !gb) || !g_q0 || !g_q1 || !g_u_step || !n_cut) return CIMPC_ERR_INVALID;
    const PlantTapeBuffers& buf = tape->buf;
    const PlantFeedback fb{buf.d_fb_K, nullptr, buf.K_f, buf.n_f, buf.hold_f, buf.n_sample};      // the chain does not need x_ref
    if (g_xref_step && !fb.K) return CIMPC_ERR_INVALID;
    const PlantModel& M = buf.M;
    const int B = tape->B, T = tape->T, n_cols = tape->n_cols;
    const size_t nq = M.nq, nu = M.nu, nw = M.nw, nc = M.nc, nb = M.nb(), TB = (size_t)T * B;
    const size_t c_mu = 2 * nq + nu + nw;                              // the columns of theta = [q0; q1; u1; w1; mu; h]
    if ((g_w_step && (size_t)n_cols < c_mu) || (g_mu && (size_t)n_cols < c_mu + 1) || (g_h && (size_t)n_cols < c_mu + 2)) return CIMPC_ERR_INVALID;
    const int nr = (int)(nq + nc + nb);
    const size_t lds = (plant_adjoint_work_doubles(nr, n_cols, (int)nq) + (fb.K ? plant_adjoint_feedback_doubles((int)nu, (int)nq) : 0)) * sizeof(double);
    if (!plant_adjoint_fits(nr, n_cols, (int)nq) || lds > PLANT_ADJ_MAX_LDS) return CIMPC_ERR_INVALID;
    const size_t n_x = g_xref_step ? TB * 2 * nq : 0;
    // the staging buffers: cotangents in, gradients out, in the order of the argument list
    const size_t n_gq = gq ? (size_t)(T + 2) * B * nq : 0, n_gg = ggamma ? TB * nc : 0, n_gb = gb ? TB * nb : 0;
    const size_t n_q = (size_t)B * nq, n_u = TB * nu, n_w = g_w_step ? TB * nw : 0, n_m = g_mu ? (size_t)B : 0, n_h = g_h ? (size_t)B : 0;
    PlantDeviceScope scope(buf.device);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok = false;
    PlantWs* ws = plant_ws_open(buf.device);
    if (ws && plant_grow(&ws->d_adj_in, &ws->cap_adj_in, n_gq + n_gg + n_gb) && plant_grow(&ws->d_adj_out, &ws->cap_adj_out, 2 * n_q + n_u + n_w + n_m + n_h) &&
        plant_grow(&ws->d_adj_cut, &ws->cap_adj_cut, (size_t)B) && (!n_x || plant_grow(&ws->d_adj_xref, &ws->cap_adj_xref, n_x))) {
        hipStream_t st = ws->st;
        double* d_gq = ws->d_adj_in; double* d_gg = d_gq + n_gq; double* d_gb = d_gg + n_gg;
        double* d_q0 = ws->d_adj_out; double* d_q1 = d_q0 + n_q; double* d_u = d_q1 + n_q; double* d_w = d_u + n_u; double* d_m = d_w + n_w;
        double* d_h = d_m + n_m;
        ok = true;
        if (gq) ok = hipMemcpyAsync(d_gq, gq, n_gq * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok && ggamma) ok = hipMemcpyAsync(d_gg, ggamma, n_gg * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok && gb) ok = hipMemcpyAsync(d_gb, gb, n_gb * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            PlantAdjoint P{buf.d_dz, buf.d_status, gq ? d_gq : nullptr, ggamma ? d_gg : nullptr, gb ? d_gb : nullptr, d_q0, d_q1, d_u,
                                 g_w_step ? d_w : nullptr, g_mu ? d_m : nullptr, g_h ? d_h : nullptr, ws->d_adj_cut, B, T, (int)nq, (int)nu,
                                 (int)nw, (int)nc, (int)nb, n_cols};
            if (fb.K) { P.fb = fb; P.g_xref_step = g_xref_step ? ws->d_adj_xref : nullptr; P.clamped = buf.d_clamped; }
            auto kernel = !fb.K ? plant_adjoint_kernel<PLANT_CHAIN_OPEN> : buf.d_clamped ? plant_adjoint_kernel<PLANT_CHAIN_CLAMP> : plant_adjoint_kernel<PLANT_CHAIN_LOOP>;
            ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
            if (ok) {
                hipLaunchKernelGGL(kernel, dim3(B), dim3(ADJ_THREADS), lds, st, P);
                ok = hipGetLastError() == hipSuccess;
            }
        }
        if (ok) ok = hipMemcpyAsync(g_q0, d_q0, n_q * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
                     hipMemcpyAsync(g_q1, d_q1, n_q * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
                     hipMemcpyAsync(g_u_step, d_u, n_u * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
                     hipMemcpyAsync(n_cut, ws->d_adj_cut, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess;
        if (ok && g_w_step) ok = hipMemcpyAsync(g_w_step, d_w, n_w * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        if (ok && g_mu) ok = hipMemcpyAsync(g_mu, d_m, n_m * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        if (ok && g_xref_step) ok = hipMemcpyAsync(g_xref_step, ws->d_adj_xref, n_x * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        if (ok && g_h) ok = hipMemcpyAsync(g_h, d_h, n_h * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = (hipStreamSynchronize(st) == hipSuccess) && ok;      // this stream only
    }
    return scope.leave(ok) ? CIMPC_OK : CIMPC_ERR_HIP;
}

extern "C" int cimpc_plant_tape_vjp(cimpc_plant_tape tape, const double* gq, const double* ggamma, const double* gb, double* g_q0,
                                    double* g_q1, double* g_u_step, double* g_w_step, double* g_mu, double* g_h, int* n_cut) {
    return cimpc_plant_tape_vjp_feedback(tape, gq, ggamma, gb, g_q0, g_q1, g_u_step, g_w_step, g_mu, g_h, n_cut, nullptr);
}
