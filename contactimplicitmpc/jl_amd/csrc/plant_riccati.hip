// The LQ backward pass over a rollout's tape (DESIGN.md sections 3, item 3e, and 5.5): time-varying LQR gains K_t, and with linear
// cost terms the feedforward k_t, the value's P0, p0 and the expected decrease dV, along the trajectory every robot of the tape took.
//
//   cimpc_plant_tape_lqr   the weights (Q, Qf, R, and q, r where given) up in ONE copy, ONE launch of plant_riccati_kernel, the gains,
//                          the value terms, status and n_cut down in ONE copy
//
// plant_riccati_kernel: one workgroup of RIC_THREADS = 256 (four wavefronts, one per SIMD of the CU) per robot walks laps T steps
// downwards through the statements of plant_riccati.h.  P, the step's matrices and both orientations of the transposed factors (Du',
// K', Dcl') sit in LDS, so that every left factor is read along the lanes (tvlqr_kernel's note: a stride of n = 36 doubles is an 8-way
// bank conflict); the products are the register tiles of plant_riccati_product (2 x 3, as tile_product of gains.hip), over the nonzero
// blocks of A_t and B_t alone.  Only the nq x (2nq + nu) corner of D_t is read from the tape; the next step's corner is loaded into
// registers before a step's arithmetic and stored to the other LDS buffer after it.  The chain is a latency chain; the robots are the
// parallelism.  62 KB of LDS at the largest model (n = 36, m = 12), 24 KB at the quadruped.
// gfx950, -O3: plant_riccati_kernel<false> 118 VGPRs, <true> 129 VGPRs, no scratch and no spills (see profiles/plant_riccati.json).
//
//   cimpc_plant_tape_lqr_box   the limited pass (plant_boxqp.h): the same call with a rho per robot, control
//                              limits and the tape's applied controls; plant_riccati_kernel<true, true>, the only instantiation that holds
//                              the box QP, with plant_boxqp.h's work behind the chain's in LDS (64 KB at the largest model)
//   cimpc_plant_tape_lqr_shooting   the limited pass with the defect hook of plant_riccati.h (multiple shooting):
//                              plant_riccati_shoot_kernel, a kernel of its own so that the instantiations above keep their names and
//                              their instructions; the node's defect is staged behind the box QP's work (64.5 KB at the largest model)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

// No fused multiply-adds in this translation unit: the chain rounds as the float64 restatement of the definition does.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "gains.h"
#include "plant_model.h"
#include "plant_riccati.h"
#include "plant_stage_launch.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

constexpr int RIC_THREADS = 256;
constexpr int RIC_STAGE_DOUBLES = 4;      // per lane: a corner of up to 1024 doubles (18 x 48 = 864 at the largest model) is wholly in flight

// the workgroup as the team of plant_riccati.h
using PlantRiccatiGroup = PlantCornerTeam<RIC_THREADS, RIC_STAGE_DOUBLES>;

template <bool LIN, bool BOX = false>      // LIN: the chain with the linear cost terms q, r; BOX: with control limits and a rho per robot
__global__ __launch_bounds__(RIC_THREADS) void plant_riccati_kernel(PlantRiccati L) {
    extern __shared__ __attribute__((aligned(16))) double ric_lds[];      // plant_riccati_lds(nq, nu), BOX: plant_riccati_box_lds(nq, nu)
    const int rb = blockIdx.x;
    if (rb >= L.B) return;                                                // uniform over the workgroup
    PlantRiccatiGroup team;
    plant_riccati_chain_as<LIN, BOX>(L, rb, ric_lds, team);
}

// the limited chain with the defect hook: L.defects and L.seg_len set, plant_riccati_shoot_lds(nq, nu) of LDS
__global__ __launch_bounds__(RIC_THREADS) void plant_riccati_shoot_kernel(PlantRiccati L) {
    extern __shared__ __attribute__((aligned(16))) double ric_lds[];
    const int rb = blockIdx.x;
    if (rb >= L.B) return;                                                // uniform over the workgroup
    PlantRiccatiGroup team;
    plant_riccati_chain_as<true, true, true>(L, rb, ric_lds, team);
}

namespace {
PlantStageWs g_riccati_ws[PLANT_MAX_DEVICES];      // d_in: the packed upload; d_out: the packed read-back, its ints included
}  // namespace

// The limited chain for a caller whose arrays are on the device already (plant_stage_launch.h): cimpc_plant_tape_lqr_box below, and the
// device-resident iLQR loop of plant_ilqr.hip.
bool plant_riccati_box_launch(const PlantRiccati& L, hipStream_t st) {
    const size_t lds = plant_riccati_box_lds(L.nq, L.nu);
    auto kernel = plant_riccati_kernel<true, true>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    hipLaunchKernelGGL(kernel, dim3(L.B), dim3(RIC_THREADS), lds, st, L);
    return hipGetLastError() == hipSuccess;
}

// The limited chain with the defect hook, beside it: L.defects and L.seg_len set, every pointer on the device.
static bool plant_riccati_shoot_launch(const PlantRiccati& L, hipStream_t st) {
    const size_t lds = plant_riccati_shoot_lds(L.nq, L.nu);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(plant_riccati_shoot_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    hipLaunchKernelGGL(plant_riccati_shoot_kernel, dim3(L.B), dim3(RIC_THREADS), lds, st, L);
    return hipGetLastError() == hipSuccess;
}

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
// Validate (no device needed), lay the two packs out (plant_staging.h: an array's extent is stated once, where its region is taken), then
// on the tape's device and the plant workspace's private stream: one upload (Q | Qf | R | q | r, and
// for the limited pass rho | u_lo | u_hi | u_nom), one launch, one read-back (K | k | P0 | p0 | dV | status | n_cut | clamped), one
// synchronize.  box: the call came through cimpc_plant_tape_lqr_box; every refusal leaves its reason for cimpc_last_error(NULL).
// shoot: it came through cimpc_plant_tape_lqr_shooting, with defects ((T / seg_len - 1) x B x 2nq) behind u_nom in the upload.
static int plant_tape_lqr_call(const char* entry, bool box, cimpc_plant_tape tape, int laps, int n_Q, const double* Q, const double* Qf, int n_R,
                               const double* R, const double* q, const double* r, int n_rho, const double* rho_b, int n_keep, double* K, double* k,
                               double* P0, double* p0, double* dV, int* status, int* n_cut, int n_lim, const double* u_lo, const double* u_hi,
                               const double* u_nom, int* clamped, bool shoot = false, int seg_len = 0, const double* defects = nullptr) {
    using namespace cimpc;
    auto refuse = [entry](const char* why) { return plant_refuse(entry, why); };
    if (!tape || !Q || !Qf || !R || !K || !status || !n_cut || !rho_b) return refuse("a null tape, Q, Qf, R, K, status, n_cut or rho");
    if (laps < 1 || n_Q < 1 || n_R < 1 || n_keep < 1) return refuse("laps, n_Q, n_R or n_keep below 1");
    const bool limits = u_lo || u_hi;
    if (limits) {                                                         // what the limited pass needs, each by its own reason
        if (!u_lo || !u_hi) return refuse("one of u_lo, u_hi without the other");
        if (!u_nom) return refuse("limits without u_nom");
        if (laps > 1) return refuse("limits with laps > 1");
        if (!q || !r) return refuse("limits without q, r");
    }
    if ((q != nullptr) != (r != nullptr)) return refuse("one of q, r without the other");
    if (laps > 1 && q) return refuse("linear terms with laps > 1");       // a periodic chain has no linear terms
    if (!q && (k || p0 || dV)) return refuse("k, p0 or dV without q, r");
    const int B = tape->B, T = tape->T, n_cols = tape->n_cols;
    if (shoot) {                                                          // what the defect hook needs, each by its own reason
        if (!defects) return refuse("null defects");
        if (!q || !r) return refuse("defects without q, r");
        if (laps > 1) return refuse("defects with laps > 1");
        if (seg_len < 1 || T % seg_len != 0) return refuse("T not divisible by segment_len");
    }
    if (n_rho != 1 && n_rho != B) return refuse("n_rho neither 1 nor B");
    if (limits && n_lim != 1 && n_lim != B) return refuse("n_lim neither 1 nor B");
    for (int b = 0; b < n_rho; ++b)
        if (!(rho_b[b] >= 0.0) || !std::isfinite(rho_b[b])) return refuse("a rho that is negative or not finite");
    if (!q && (n_rho != 1 || clamped)) return refuse("a rho per robot or clamped without q, r");
    if (limits) {                                                         // the limits' entries: the model's nu by the tape's model id alone
        PlantModel named{};
        if (!plant_model_by_id(tape->model, &named) || named.nu < 1) return refuse("a model without controls");
        for (size_t e = 0; e < (size_t)n_lim * named.nu; ++e) {
            if (u_lo[e] != u_lo[e] || u_hi[e] != u_hi[e]) return refuse("a NaN limit");
            if (u_lo[e] > u_hi[e]) return refuse("u_lo above u_hi");
        }
    }
    const PlantTapeBuffers& buf = tape->buf;
    if (B < 1 || T < 1 || buf.device < 0 || buf.device >= PLANT_MAX_DEVICES || !buf.d_dz || !buf.d_status) return refuse("a closed or empty tape");
    if ((n_Q != 1 && n_Q != T) || (n_R != 1 && n_R != T) || n_keep > T) return refuse("n_Q or n_R neither 1 nor T, or n_keep above T");
    if ((long long)laps * T > (1 << 30)) return refuse("laps T beyond 2^30");
    const PlantModel& M = buf.M;
    const int nq = M.nq, nu = M.nu, nr = M.nq + M.nc + M.nb();
    if (nu < 1 || n_cols < 2 * nq + nu || !plant_riccati_fits(nq, nu)) return refuse("a model without controls, or a tape without the control columns");
    if (box && q && (nu > PLANT_BOXQP_MAX_M || plant_riccati_box_lds(nq, nu) > PLANT_RIC_MAX_LDS)) return refuse("a model too large for the limited pass");
    if (limits && !plant_all_finite(u_nom, (size_t)T * B * nu)) return refuse("a non-finite entry of u_nom");
    const size_t n = (size_t)2 * nq, m = (size_t)nu, nn = n * n, mm = m * m, nB = (size_t)B;
    const size_t n_def = shoot ? (size_t)(T / seg_len - 1) * B * n : 0;
    if (!plant_all_finite(defects, n_def)) return refuse("a non-finite entry of defects");
    const bool boxed = box && q;                                          // the limited chain: plant_riccati_kernel<true, true>
    const double rho = rho_b[0];
    // the packed upload, in the order of the argument list; an array the call does not have takes no room
    PlantCursor at;
    const PlantSpan i_Q = at.take((size_t)n_Q * nn), i_Qf = at.take(nn), i_R = at.take((size_t)n_R * mm), i_q = at.take(q ? (size_t)(T + 1) * nB * n : 0),
                    i_r = at.take(r ? (size_t)T * nB * m : 0), i_rho = at.take(boxed ? (size_t)n_rho : 0), i_lo = at.take(limits ? (size_t)n_lim * m : 0),
                    i_hi = at.take(limits ? (size_t)n_lim * m : 0), i_un = at.take(limits ? (size_t)T * nB * m : 0), i_def = at.take(n_def);
    const size_t n_in = at.end();
    // the packed read-back; status | n_cut are 2 B ints in B doubles, clamped n_keep x B ints in doubles behind them
    const PlantSpan o_K = at.take((size_t)n_keep * nB * m * n), o_k = at.take(k ? (size_t)n_keep * nB * m : 0), o_P = at.take(P0 ? nB * nn : 0),
                    o_p = at.take(p0 ? nB * n : 0), o_V = at.take(dV ? nB * 2 : 0), o_st = at.take(nB),
                    o_cl = at.take(boxed && clamped ? ((size_t)n_keep * nB + 1) / 2 : 0);
    const size_t n_out = at.end();
    std::vector<double> up(n_in);
    const std::unique_ptr<double[]> out(new double[n_out]);      // not value-initialized: K alone is 36 MB at quadruped B = 256, T = 100
    bool packed = true;
    PlantCopier<PlantHostCopy> pack{{}, packed};
    pack.up(up.data(), i_Q, Q); pack.up(up.data(), i_Qf, Qf); pack.up(up.data(), i_R, R); pack.up(up.data(), i_q, q); pack.up(up.data(), i_r, r);
    pack.up(up.data(), i_rho, rho_b); pack.up(up.data(), i_lo, u_lo); pack.up(up.data(), i_hi, u_hi); pack.up(up.data(), i_un, u_nom);
    pack.up(up.data(), i_def, defects);
    const size_t lds = shoot ? plant_riccati_shoot_lds(nq, nu) : boxed ? plant_riccati_box_lds(nq, nu) : plant_riccati_lds(nq, nu);
    PlantDeviceScope scope(buf.device);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    bool ok = false;
    PlantWs* ws = plant_ws_open(buf.device);
    PlantStageWs& W = g_riccati_ws[buf.device];
    if (ws && W.grow(n_in, n_out, 0)) {
        hipStream_t st = ws->st;
        double* I = W.d_in;
        double* O = W.d_out;
        int* d_status = reinterpret_cast<int*>(o_st.on(O));
        ok = hipMemcpyAsync(I, up.data(), n_in * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            PlantRiccati L{buf.d_dz, buf.d_status, i_Q.on(I), i_Qf.on(I), i_R.on(I), i_q.or_null(I), i_r.or_null(I),
                           o_K.on(O), o_k.or_null(O), o_P.or_null(O), o_p.or_null(O), o_V.or_null(O),
                           d_status, d_status + B, B, T, nq, nu, nr, n_cols, laps, n_Q, n_R, n_keep, rho};
            if (boxed) {
                L.rho_b = i_rho.on(I); L.n_rho = n_rho;
                if (limits) { L.u_lo = i_lo.on(I); L.u_hi = i_hi.on(I); L.u_nom = i_un.on(I); L.n_lim = n_lim; }
                if (clamped) L.clamped = reinterpret_cast<int*>(o_cl.on(O));
            }
            if (shoot) {
                L.defects = i_def.on(I); L.seg_len = seg_len;
                ok = plant_riccati_shoot_launch(L, st);
            } else if (boxed) {
                ok = plant_riccati_box_launch(L, st);
            } else {
                auto kernel = q ? plant_riccati_kernel<true> : plant_riccati_kernel<false>;
                ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
                if (ok) {
                    hipLaunchKernelGGL(kernel, dim3(B), dim3(RIC_THREADS), lds, st, L);
                    ok = hipGetLastError() == hipSuccess;
                }
            }
        }
        if (ok) ok = hipMemcpyAsync(out.get(), O, n_out * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = (hipStreamSynchronize(st) == hipSuccess) && ok;      // this stream only
    }
    if (!scope.leave(ok)) return CIMPC_ERR_HIP;
    pack.down(K, out.get(), o_K); pack.down(k, out.get(), o_k); pack.down(P0, out.get(), o_P); pack.down(p0, out.get(), o_p); pack.down(dV, out.get(), o_V);
    const int* words = reinterpret_cast<const int*>(o_st.on(out.get()));      // status | n_cut
    pack.down(status, words, PlantSpan{0, nB}); pack.down(n_cut, words, PlantSpan{nB, nB});
    if (o_cl.n) pack.down(clamped, reinterpret_cast<const int*>(o_cl.on(out.get())), PlantSpan{0, (size_t)n_keep * nB});
    return CIMPC_OK;
}

extern "C" int cimpc_plant_tape_lqr(cimpc_plant_tape tape, int laps, int n_Q, const double* Q, const double* Qf, int n_R, const double* R,
                                    const double* q, const double* r, double rho, int n_keep, double* K, double* k, double* P0, double* p0,
                                    double* dV, int* status, int* n_cut) {
    return plant_tape_lqr_call("cimpc_plant_tape_lqr", false, tape, laps, n_Q, Q, Qf, n_R, R, q, r, 1, &rho, n_keep, K, k, P0, p0, dV, status, n_cut,
                               1, nullptr, nullptr, nullptr, nullptr);
}

// The limited pass: cimpc_plant_tape_lqr with rho as n_rho (1 or B) values, and n_lim (1 or B) rows of limits u_lo, u_hi (both null: no
// limits) about the tape's applied controls u_nom (T x B x nu); clamped (n_keep x B, may be null): bit i set where control i was clamped.
extern "C" int cimpc_plant_tape_lqr_box(cimpc_plant_tape tape, int laps, int n_Q, const double* Q, const double* Qf, int n_R, const double* R,
                                        const double* q, const double* r, int n_rho, const double* rho, int n_keep, double* K, double* k,
                                        double* P0, double* p0, double* dV, int* status, int* n_cut, int n_lim, const double* u_lo,
                                        const double* u_hi, const double* u_nom, int* clamped) {
    return plant_tape_lqr_call("cimpc_plant_tape_lqr_box", true, tape, laps, n_Q, Q, Qf, n_R, R, q, r, n_rho, rho, n_keep, K, k, P0, p0, dV, status,
                               n_cut, n_lim, u_lo, u_hi, u_nom, clamped);
}

// The limited pass with defects (multiple shooting): cimpc_plant_tape_lqr_box on a tape whose horizon is cut
// into T / segment_len segments, with the defect of node j = 1 .. (defects, (T / segment_len - 1) x B x 2nq) entering the value's linear term
// at the walk step of t = j segment_len - 1:  p <- p + P d.  Needs q, r and laps = 1.
extern "C" int cimpc_plant_tape_lqr_shooting(cimpc_plant_tape tape, int n_Q, const double* Q, const double* Qf, int n_R, const double* R,
                                             const double* q, const double* r, int n_rho, const double* rho, int n_keep, double* K, double* k,
                                             double* P0, double* p0, double* dV, int* status, int* n_cut, int n_lim, const double* u_lo,
                                             const double* u_hi, const double* u_nom, int* clamped, int segment_len, const double* defects) {
    return plant_tape_lqr_call("cimpc_plant_tape_lqr_shooting", true, tape, 1, n_Q, Q, Qf, n_R, R, q, r, n_rho, rho, n_keep, K, k, P0, p0, dV, status,
                               n_cut, n_lim, u_lo, u_hi, u_nom, clamped, true, segment_len, defects);
}
