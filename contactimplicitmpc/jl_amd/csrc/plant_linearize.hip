// The plant models linearized on the device: LinearizedStep(s, z, θ, κ) = (r0, rz0, rθ0) of the reference
// (src/controller/linearized_step.jl:10-31, implicit_dynamics.jl:37-50) from the residuals of plant_model.h, for N knots in one call.
// One workgroup per knot; the nz + nθ Jacobian columns are strided over its lanes: lane c, c + NT, ... evaluates the residual on
// dual numbers (z on Dual, θ on DualTh, κ = 0) with tangent 1 on z[c] or on θ[c - nz] and writes column c of rz0 or rθ0 - exact
// derivatives, the scheme of plant_step_kernel's Jacobian with θ seeded too.  One plain double evaluation at the caller's κ gives r0.
// Outputs are column-major, the layout cimpc_set_linearization takes.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

// No fused multiply-adds in this translation unit, the residuals of plant_model.h included: every operation rounds as IEEE double, so
// an entry does not depend on which instantiation computed it (a flat knot of a terrain batch is the no-terrain call bit for bit)
// and kappa leaves r0's bilinear rows by one subtraction each.  The kernel runs when tables are built, not per step.
#pragma clang fp contract(off)

#include "../../../include/cimpc.h"
#include "plant_ground.h"
#include "plant_linearize.h"
#include "plant_model.h"
#include "plant_workspace.h"

namespace cimpc {

// Lanes of a knot's workgroup: one pass over the nz + nth columns where at most three wavefronts hold them (28, 35, 41 | 77, 119 | 167)
constexpr int linearize_threads(int NZ, int NTH) { return (NZ + NTH + 63) / 64 * 64; }

// Knot blockIdx.x on NT lanes.  The per-lane z, θ and r copies are sized by the instantiation (NZ, NTH).  z: N x nz, theta: N x nth;
// r0: N x nz, rz0: N x (nz x nz), rth0: N x (nz x nth), the matrices column-major; a null output is skipped.
template <int NZ, int NTH, int NT, int GROUND>
__global__ __launch_bounds__(NT) void plant_linearize_kernel(PlantModel M, int N, const double* z, const double* theta,
                                                             const cimpc_terrain* terrain, int n_terrain, double kappa, double* r0,
                                                             double* rz0, double* rth0) {
    static_assert(NT % 64 == 0, "whole wavefronts");
    __shared__ double zs[NZ], ths[NTH];
    __shared__ cimpc_terrain ter;
    const int k = blockIdx.x, lane = threadIdx.x;
    const int nz = M.nz(), nth = M.nth();
    if (k >= N || nz > NZ || nth > NTH) return;                       // uniform over the workgroup
    for (int i = lane; i < nz; i += NT) zs[i] = z[(size_t)k * nz + i];
    for (int i = lane; i < nth; i += NT) ths[i] = theta[(size_t)k * nth + i];
    if constexpr (GROUND == GROUND_TERRAIN) {
        if (terrain) plant_stage_terrain(ter, terrain, n_terrain, k, lane);
    }
    __syncthreads();
    bool rough = false;
    if constexpr (GROUND == GROUND_TERRAIN) rough = terrain && plant_rough(M, ter);
    auto residual = [&](const auto* zz, const auto* tt, double kap, auto* rr) { plant_ground_residual<GROUND>(M, ter, rough, zz, tt, kap, rr); };
    // columns [c_lo, c_hi) of [rz0 rθ0]: only the halves asked for
    const int c_lo = rz0 ? 0 : nz, c_hi = rth0 ? nz + nth : nz;
    for (int c = c_lo + lane; c < c_hi; c += NT) {
        Dual zl[NZ], rl[NZ];
        DualTh tl[NTH];
        plant_seed_column(nz, nth, zs, ths, c, zl, tl);
        residual(zl, tl, 0.0, rl);
        double* out = c < nz ? rz0 + ((size_t)k * nz + c) * nz : rth0 + ((size_t)k * nth + (c - nz)) * nz;
        for (int i = 0; i < nz; ++i) out[i] = rl[i].d;
    }
    if (r0 && lane < 64) {                                             // the first wavefront: every lane evaluates, lane i stores r0[i], r0[i + 64]
        double zl[NZ], tl[NTH], rl[NZ];
        for (int i = 0; i < nz; ++i) zl[i] = zs[i];
        for (int i = 0; i < nth; ++i) tl[i] = ths[i];
        residual(zl, tl, kappa, rl);
        for (int i = lane; i < nz; i += 64) r0[(size_t)k * nz + i] = rl[i];
    }
}

}  // namespace cimpc

// ---- launch -------------------------------------------------------------------------------------------------------------
namespace cimpc {

// The model's linearization instance (plant_ground.h): N knots on `st`, all pointers device memory (a null output is skipped; d_ter
// null: flat ground).  No synchronization.
static bool plant_linearize_launch(const PlantModel& M, int N, const double* d_z, const double* d_th, const cimpc_terrain* d_ter,
                                   int n_terrain, double kappa, double* d_r, double* d_rz, double* d_rth, hipStream_t st) {
    return plant_visit_instance(M, d_ter != nullptr, false, [&](auto tag) {
        using I = decltype(tag);
        constexpr int NT = linearize_threads(I::NZ, I::NTH);
        auto kernel = plant_linearize_kernel<I::NZ, I::NTH, NT, I::GROUND>;
        hipLaunchKernelGGL(kernel, dim3(N), dim3(NT), 0, st, M, N, d_z, d_th, d_ter, d_ter ? n_terrain : 0, kappa, d_r, d_rz, d_rth);
        return hipGetLastError() == hipSuccess;
    });
}

// What cimpc_plant_linearize validates without a device, but for the outputs (plant_linearize.h)
static int plant_linearize_validate(int model, int N, int n_terrain, const cimpc_terrain* terrain, const double* z, const double* theta,
                                    double kappa, PlantModel* M, bool* rough) {
    if (N <= 0 || !z || !theta || !std::isfinite(kappa) || kappa < 0.0) return CIMPC_ERR_INVALID;
    if ((n_terrain != 0) != (terrain != nullptr)) return CIMPC_ERR_INVALID;
    if (!plant_model_and_ground(model, N, n_terrain, terrain, M, rough)) return CIMPC_ERR_INVALID;
    const size_t nth = (size_t)M->nth();
    for (int k = 0; k < N; ++k) if (!(theta[(size_t)k * nth + nth - 1] > 0.0)) return CIMPC_ERR_INVALID;      // h, the last entry of θ
    return CIMPC_OK;
}

int plant_linearize_check(int model, int N, int n_terrain, const cimpc_terrain* terrain, const double* z, const double* theta, double kappa,
                          PlantLinearizeDims* d) {
    PlantModel M{};
    bool rough = false;
    if (int rc = plant_linearize_validate(model, N, n_terrain, terrain, z, theta, kappa, &M, &rough); rc != CIMPC_OK) return rc;
    *d = PlantLinearizeDims{M.nq, M.nu, M.nw, M.nc, M.nb(), rough ? n_terrain : 0};
    return CIMPC_OK;
}

bool plant_stage_knots(PlantWs& W, int N, int nz, int nth, int n_terrain_up, const double* z, const double* theta, const cimpc_terrain* terrain,
                       PlantKnots* k) {
    const size_t n_z = (size_t)N * nz, n_th = (size_t)N * nth, n_ter = (size_t)n_terrain_up * TERRAIN_WORDS;
    k->host.resize(n_z + n_th + n_ter);
    std::memcpy(k->host.data(), z, n_z * sizeof(double));
    std::memcpy(k->host.data() + n_z, theta, n_th * sizeof(double));
    if (n_ter) std::memcpy(k->host.data() + n_z + n_th, terrain, n_ter * sizeof(double));
    if (!plant_grow(&W.d_lin_in, &W.cap_lin_in, k->host.size())) return false;
    k->d_z = W.d_lin_in;
    k->d_th = k->d_z + n_z;
    k->d_ter = n_ter ? reinterpret_cast<const cimpc_terrain*>(k->d_th + n_th) : nullptr;
    return hipMemcpyAsync(W.d_lin_in, k->host.data(), k->host.size() * sizeof(double), hipMemcpyHostToDevice, W.st) == hipSuccess;
}

bool plant_linearize_launch(int model, int N, const double* d_z, const double* d_th, const cimpc_terrain* d_ter, int n_terrain, double kappa,
                            double* d_r, double* d_rz, double* d_rth, hipStream_t st) {
    PlantModel M{};
    return plant_model_by_id(model, &M) && plant_linearize_launch(M, N, d_z, d_th, d_ter, n_terrain, kappa, d_r, d_rz, d_rth, st);
}

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------
// Validate (no device needed), pick the model, then on the plant workspace's private stream: one upload (z | theta | terrains),
// one launch, one read-back (the outputs asked for), one synchronize.
extern "C" int cimpc_plant_linearize(int model, int N, int n_terrain, const cimpc_terrain* terrain, const double* z, const double* theta,
                                     double kappa, double* r0, double* rz0, double* rth0) {
    using namespace cimpc;
    if (!r0 && !rz0 && !rth0) return CIMPC_ERR_INVALID;
    PlantModel M{};
    bool rough = false;
    if (int rc = plant_linearize_validate(model, N, n_terrain, terrain, z, theta, kappa, &M, &rough); rc != CIMPC_OK) return rc;
    const size_t nz = (size_t)M.nz(), nth = (size_t)M.nth();
    int dev = 0;
    if (!plant_current_device(&dev)) return CIMPC_ERR_NO_DEVICE;
    const size_t n_z = (size_t)N * nz;
    const size_t n_r = r0 ? n_z : 0, n_rz = rz0 ? n_z * nz : 0, n_rth = rth0 ? n_z * nth : 0;
    std::vector<double> out(n_r + n_rz + n_rth);
    PlantKnots in;
    std::lock_guard<std::mutex> lock(g_plant_mu);
    PlantWs* ws = plant_ws_open(dev);
    if (!ws) return CIMPC_ERR_HIP;
    PlantWs& W = *ws;
    if (!plant_grow(&W.d_lin_out, &W.cap_lin_out, out.size())) return CIMPC_ERR_HIP;
    hipStream_t st = W.st;
    double* dr = r0 ? W.d_lin_out : nullptr; double* drz = rz0 ? W.d_lin_out + n_r : nullptr; double* drth = rth0 ? W.d_lin_out + n_r + n_rz : nullptr;
    bool ok = plant_stage_knots(W, N, (int)nz, (int)nth, rough ? n_terrain : 0, z, theta, terrain, &in);
    if (ok) ok = plant_linearize_launch(M, N, in.d_z, in.d_th, in.d_ter, n_terrain, kappa, dr, drz, drth, st);
    if (ok) ok = hipMemcpyAsync(out.data(), W.d_lin_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = (hipStreamSynchronize(st) == hipSuccess) && ok;      // this stream only
    if (!ok) return CIMPC_ERR_HIP;
    if (r0) std::memcpy(r0, out.data(), n_r * sizeof(double));
    if (rz0) std::memcpy(rz0, out.data() + n_r, n_rz * sizeof(double));
    if (rth0) std::memcpy(rth0, out.data() + n_r + n_rz, n_rth * sizeof(double));
    return CIMPC_OK;
}
