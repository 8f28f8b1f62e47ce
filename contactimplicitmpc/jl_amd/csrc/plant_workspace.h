// Per-device workspace of the plant entry points (plant_kernel.hip: step, terrain step, rollout; plant_linearize.hip: linearize):
// buffers and a private stream live across calls (a simulator step is called thousands of times in a closed loop; allocating and a
// device-wide synchronize per call stalled everything else on the GPU).  One mutex serializes the entry points; each keeps buffers
// of its own, grow-only, and all share the stream.
//   step / rollout  d_in: trajectory (T + 2) x B x nq | u schedule | w schedule | per-robot mu; d_out: gamma | b; d_st: status | iters
//                   (T x B each); d_ter: the robots' terrains
//   linearize       d_lin_in: z | theta | terrains (N x nz, N x nth, n_terrain cimpc_terrain); d_lin_out: r0 | rz0 | rth0 (those asked for)
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>

#include "../../../include/cimpc.h"

namespace cimpc {

struct PlantWs {
    int device = -1;
    hipStream_t st = nullptr;
    double *d_in = nullptr, *d_out = nullptr;
    int* d_st = nullptr;
    cimpc_terrain* d_ter = nullptr;
    size_t cap_in = 0, cap_out = 0, cap_st = 0, cap_ter = 0;
    double *d_lin_in = nullptr, *d_lin_out = nullptr;
    size_t cap_lin_in = 0, cap_lin_out = 0;
};
constexpr int PLANT_MAX_DEVICES = 16;
extern PlantWs g_plant_ws[PLANT_MAX_DEVICES];      // defined in plant_kernel.hip
extern std::mutex g_plant_mu;

template <class T>
bool plant_grow(T** p, size_t* cap, size_t need) {
    if (*cap >= need) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, need * sizeof(T)) != hipSuccess) return false;
    *cap = need;
    return true;
}

}  // namespace cimpc
