// Dimension dispatch of the interior-point sweep kernel and of the single-launch solve: one instantiation per row of model_table.h, reached through one
// lookup there and one call through the row's entry here.  A further model is one row in model_table.h + an ip_model_<name>.hip (+ an async_model_<name>.hip
// if the row says so) + the file names in the Makefile's SRCS.  centroidal_quadruped_wall (ny = 48 exceeds the 32-lane group) has a 64-lane instantiation - one
// problem per wavefront, :configuration mode only (round 6); its :configurationforce mode keeps the runtime-dimension kernel.
#include "model_table.h"
#include "newton_state.h"

namespace cimpc {

// per-row entry points (ip_model_<name>.hip, async_model_<name>.hip), in table order
using IpLaunchFn = int(int mode, const IpParams& p, int waves, hipStream_t s);
using IpCallbackFn = int(int mode, const IpCallbackArgs& a, hipStream_t s);
using IpInfoFn = void(int mode, KernelInfo* info);
using AsyncLaunchFn = int(const IpParams& p, const NewtonDev& S, int waves, int grid, hipStream_t s);
struct ModelEntry { IpLaunchFn* launch; IpCallbackFn* callback; IpInfoFn* info; AsyncLaunchFn* async; };      // callback: null for a 64-lane row; async: null without a single-launch instantiation
#define CIMPC_ASYNC_ENTRY_0(f) nullptr
#define CIMPC_ASYNC_ENTRY_1(f) f
#define CIMPC_DECLARE(name, q, u, w, c, b, a) IpLaunchFn ip_launch_##name; IpCallbackFn ip_callback_##name; IpInfoFn ip_info_##name; AsyncLaunchFn async_launch_##name;
#define CIMPC_ENTRY(name, q, u, w, c, b, a) {ip_launch_##name, model_lanes(MODEL_TABLE[MODEL_##name]) <= 32 ? ip_callback_##name : nullptr, ip_info_##name, CIMPC_ASYNC_ENTRY_##a(async_launch_##name)},
CIMPC_MODEL_TABLE(CIMPC_DECLARE)
static const ModelEntry MODEL_ENTRIES[MODEL_COUNT] = {CIMPC_MODEL_TABLE(CIMPC_ENTRY)};

int ip_kernel_info(const cimpc_dims* dm, KernelInfo* info) {
    const int id = model_sweep(dm);
    if (id == MODEL_COUNT && !ip_generic_available(dm)) return CIMPC_ERR_INVALID;
    if (id < MODEL_COUNT) MODEL_ENTRIES[id].info(dm->mode, info);
    else ip_generic_info(dm, info);      // any other model with nx, ny <= 64: runtime-dimension kernel
    info->generic = id == MODEL_COUNT ? 1 : 0;
    return CIMPC_OK;
}

int launch_ip_sweep(const cimpc_dims* dm, const IpParams& p, int waves, hipStream_t s) {
    if (const int id = model_sweep(dm); id < MODEL_COUNT) return MODEL_ENTRIES[id].launch(dm->mode, p, waves, s);
    return launch_ip_generic(dm, p, s);
}

int launch_ip_callback(const cimpc_dims* dm, const IpCallbackArgs& a, hipStream_t s) {
    if (const int id = model_callback(dm); id < MODEL_COUNT) return MODEL_ENTRIES[id].callback(dm->mode, a, s);
    return CIMPC_ERR_INVALID;
}

// asynchronous single-launch Newton solve (newton_async_impl.h)
bool newton_async_available(const cimpc_dims* dm) { return model_async(dm) < MODEL_COUNT; }

int launch_newton_async(const cimpc_dims* dm, const IpParams& p, const NewtonDev& S, int waves, int grid, hipStream_t s) {
    if (const int id = model_async(dm); id < MODEL_COUNT) return MODEL_ENTRIES[id].async(p, S, waves, grid, s);
    return CIMPC_ERR_INVALID;
}

}  // namespace cimpc
