// Forward tangents through a rollout's tape (DESIGN.md sections 3, item 3d, and 5.5): the Jacobian-vector product of the whole
// trajectory with respect to the rollout's inputs, many directions per launch.
//
//   cimpc_plant_tape_jvp            tangents (dq0, dq1, du_step, dw_step, dmu, dh; those given) up, ONE launch of plant_tangent_kernel,
//                                   the trajectory tangents (dq, dgamma, db) and n_cut down
//   cimpc_plant_tape_jvp_feedback   the same with dxref_step in and du_applied out, on a closed-loop tape; a closed-loop tape's chain
//                                   runs the feedback statements through either entry, and the tape of a limited closed loop
//                                   (item 3i) launches the third instantiation, which reads the tape's mask of clamped controls
//
// plant_tangent_kernel: grid (B, direction groups), a workgroup of TAN_THREADS = 256 (four wavefronts, one per SIMD of the CU) walks
// t = 0 .. T-1 through the statements of plant_tangent.h for one robot and plant_tangent_group(...) directions.  D_t (nr x n_cols
// doubles, column-major as the sensitivity kernel wrote it) sits in LDS ONCE for the group; block t+1 is loaded into registers before
// step t's arithmetic and stored to the other LDS buffer after it, as plant_adjoint_kernel does backwards.  A work item is one (row r,
// direction d) pair, r fastest across lanes: consecutive lanes read consecutive doubles of a column of D_t, x[c] of a direction is a
// broadcast.  x, the three live rows of dq and de of every direction are in LDS too; only the trajectory tangents reach global memory.
#include <hip/hip_runtime.h>
#include <mutex>

// No fused multiply-adds in this translation unit: the chain rounds as the float64 restatement of the definition does.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "plant_model.h"
#include "plant_tangent.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

constexpr int TAN_THREADS = 256;
constexpr int TAN_STAGE_DOUBLES = 12;      // per lane: a block of up to 3072 doubles is wholly in flight during a step

// the workgroup as the team of plant_tangent.h
struct PlantTangentGroup {
    double stage[TAN_STAGE_DOUBLES];
    __device__ int rank() const { return threadIdx.x; }
    __device__ int size() const { return TAN_THREADS; }
    __device__ void sync() const { __syncthreads(); }
    __device__ void fetch_issue(const double* src, int n) {
#pragma unroll
        for (int k = 0; k < TAN_STAGE_DOUBLES; ++k) {
            const int i = k * TAN_THREADS + (int)threadIdx.x;
            stage[k] = i < n ? src[i] : 0.0;
        }
    }
    __device__ void fetch_commit(double* dst, const double* src, int n) {
#pragma unroll
        for (int k = 0; k < TAN_STAGE_DOUBLES; ++k) {
            const int i = k * TAN_THREADS + (int)threadIdx.x;
            if (i < n) dst[i] = stage[k];
        }
        for (int i = TAN_STAGE_DOUBLES * TAN_THREADS + (int)threadIdx.x; i < n; i += TAN_THREADS) dst[i] = src[i];
    }
};

// FB: PLANT_TANGENT_OPEN, PLANT_TANGENT_LOOP (a closed-loop tape's chain, with the feedback statements of plant_feedback.h) or
// PLANT_TANGENT_CLAMP (a limited closed-loop tape's, which also reads the tape's mask of clamped controls)
template <int FB>
__global__ __launch_bounds__(TAN_THREADS) void plant_tangent_kernel(PlantTangent P, int group) {
    extern __shared__ __attribute__((aligned(16))) double tan_lds[];      // plant_tangent_lds(nr, n_cols, nq, nu, FB, group)
    const int rb = blockIdx.x, d0 = (int)blockIdx.y * group;
    if (rb >= P.B || d0 >= P.n_dir) return;                                // uniform over the workgroup
    const int nd = P.n_dir - d0 < group ? P.n_dir - d0 : group;
    PlantTangentGroup team;
    plant_tangent_chain_as<FB>(P, rb, d0, nd, tan_lds, team);
}

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
// Validate (no device needed), then on the tape's device and the plant workspace's private stream: one upload (the tangents given, in
// the order of the argument list), one launch, one read-back (dq | dgamma | db | du_applied, those asked for, and n_cut), one
// synchronize.
extern "C" int cimpc_plant_tape_jvp_feedback(cimpc_plant_tape tape, int n_dir, const double* dq0, const double* dq1, const double* du_step,
                                             const double* dw_step, const double* dmu, const double* dh, double* dq, double* dgamma, double* db,
                                             int* n_cut, const double* dxref_step, double* du_applied) {
    using namespace cimpc;
    if (!tape || n_dir < 1 || (!dq0 && !dq1 && !du_step && !dw_step && !dmu && !dh && !dxref_step) || !dq || !n_cut) return CIMPC_ERR_INVALID;
    const PlantTapeBuffers& buf = tape->buf;
    const PlantFeedback fb{buf.d_fb_K, nullptr, buf.K_f, buf.n_f, buf.hold_f, buf.n_sample};      // the chain does not need x_ref
    if ((dxref_step || du_applied) && !fb.K) return CIMPC_ERR_INVALID;
    const PlantModel& M = buf.M;
    const int B = tape->B, T = tape->T, n_cols = tape->n_cols;
    const size_t nq = M.nq, nu = M.nu, nw = M.nw, nc = M.nc, nb = M.nb(), TB = (size_t)T * B, nD = (size_t)n_dir;
    const size_t c_mu = 2 * nq + nu + nw;                              // the columns of theta = [q0; q1; u1; w1; mu; h]
    if ((dw_step && (size_t)n_cols < c_mu) || (dmu && (size_t)n_cols < c_mu + 1) || (dh && (size_t)n_cols < c_mu + 2)) return CIMPC_ERR_INVALID;
    const int nr = (int)(nq + nc + nb);
    const int group = plant_tangent_group(nr, n_cols, (int)nq, (int)nu, fb.K != nullptr);
    if (group < 1) return CIMPC_ERR_INVALID;
    const int per = n_dir < group ? n_dir : group;                     // a launch of fewer directions asks for no more LDS than they need
    const size_t n_groups = (nD + per - 1) / per;
    if (n_groups > 65535) return CIMPC_ERR_INVALID;                  // the grid's second dimension
    const size_t lds = plant_tangent_lds(nr, n_cols, (int)nq, (int)nu, fb.K != nullptr, per);
    // the staging buffers: tangents in, trajectory tangents out, in the order of the argument list
    const size_t i_q0 = dq0 ? nD * B * nq : 0, i_q1 = dq1 ? nD * B * nq : 0, i_u = du_step ? nD * TB * nu : 0, i_w = dw_step ? nD * TB * nw : 0,
                 i_m = dmu ? nD * B : 0, i_h = dh ? nD * B : 0, i_x = dxref_step ? nD * TB * 2 * nq : 0;
    const size_t o_q = nD * (size_t)(T + 2) * B * nq, o_g = dgamma ? nD * TB * nc : 0, o_b = db ? nD * TB * nb : 0, o_u = du_applied ? nD * TB * nu : 0;
    PlantDeviceScope scope(buf.device);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok = false;
    PlantWs* ws = plant_ws_open(buf.device);
    if (ws && plant_grow(&ws->d_tan_in, &ws->cap_tan_in, i_q0 + i_q1 + i_u + i_w + i_m + i_h + i_x) &&
        plant_grow(&ws->d_tan_out, &ws->cap_tan_out, o_q + o_g + o_b + o_u) && plant_grow(&ws->d_tan_cut, &ws->cap_tan_cut, (size_t)B)) {
        hipStream_t st = ws->st;
        double* d_q0 = ws->d_tan_in; double* d_q1 = d_q0 + i_q0; double* d_u = d_q1 + i_q1; double* d_w = d_u + i_u; double* d_m = d_w + i_w;
        double* d_h = d_m + i_m; double* d_x = d_h + i_h;
        double* d_dq = ws->d_tan_out; double* d_dg = d_dq + o_q; double* d_db = d_dg + o_g; double* d_ua = d_db + o_b;
        const auto up = [&](double* dst, const double* src, size_t n) {
            return !src || hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
        };
        const auto down = [&](double* dst, const double* src, size_t n) {
            return !dst || hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        };
        ok = up(d_q0, dq0, i_q0) && up(d_q1, dq1, i_q1) && up(d_u, du_step, i_u) && up(d_w, dw_step, i_w) && up(d_m, dmu, i_m) && up(d_h, dh, i_h) &&
             up(d_x, dxref_step, i_x);
        if (ok) {
            PlantTangent P{buf.d_dz, buf.d_status, dq0 ? d_q0 : nullptr, dq1 ? d_q1 : nullptr, du_step ? d_u : nullptr, dw_step ? d_w : nullptr,
                           dmu ? d_m : nullptr, dh ? d_h : nullptr, d_dq, dgamma ? d_dg : nullptr, db ? d_db : nullptr, ws->d_tan_cut, B, T,
                           (int)nq, (int)nu, (int)nw, (int)nc, (int)nb, n_cols, n_dir};
            if (fb.K) { P.fb = fb; P.dxref_step = dxref_step ? d_x : nullptr; P.du_applied = du_applied ? d_ua : nullptr; P.clamped = buf.d_clamped; }
            auto kernel = !fb.K ? plant_tangent_kernel<PLANT_TANGENT_OPEN> : buf.d_clamped ? plant_tangent_kernel<PLANT_TANGENT_CLAMP> : plant_tangent_kernel<PLANT_TANGENT_LOOP>;
            ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
            if (ok) {
                hipLaunchKernelGGL(kernel, dim3(B, (unsigned)n_groups), dim3(TAN_THREADS), lds, st, P, per);
                ok = hipGetLastError() == hipSuccess;
            }
        }
        if (ok) ok = down(dq, d_dq, o_q) && down(dgamma, d_dg, o_g) && down(db, d_db, o_b) && down(du_applied, d_ua, o_u) &&
                     hipMemcpyAsync(n_cut, ws->d_tan_cut, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = (hipStreamSynchronize(st) == hipSuccess) && ok;      // this stream only
    }
    return scope.leave(ok) ? CIMPC_OK : CIMPC_ERR_HIP;
}

extern "C" int cimpc_plant_tape_jvp(cimpc_plant_tape tape, int n_dir, const double* dq0, const double* dq1, const double* du_step,
                                    const double* dw_step, const double* dmu, const double* dh, double* dq, double* dgamma, double* db, int* n_cut) {
    return cimpc_plant_tape_jvp_feedback(tape, n_dir, dq0, dq1, du_step, dw_step, dmu, dh, dq, dgamma, db, n_cut, nullptr, nullptr);
}
