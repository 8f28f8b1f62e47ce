// The linearization of the plant models (plant_linearize.hip) for callers inside the library that bring their own device buffers
// and stream: cimpc_linearize_knots (cimpc_host.cpp) runs it on the handle's stream in front of the table build.  Models go by
// their public id (cimpc.h: CIMPC_PLANT_*), so that plant_model.h stays out of the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "../../../include/cimpc.h"

namespace cimpc {

struct PlantLinearizeDims {
    int nq, nu, nw, nc, nb;
    int n_terrain_up;      // terrains the kernel reads (0: every knot on flat ground - nothing to upload, pass a null d_ter)
};

// Everything cimpc_plant_linearize validates about its inputs, without a device: CIMPC_OK and the model's dimensions, or
// CIMPC_ERR_INVALID.
int plant_linearize_check(int model, int N, int n_terrain, const cimpc_terrain* terrain, const double* z, const double* theta, double kappa,
                          PlantLinearizeDims* d);

// The knots of a call on the device, where cimpc_plant_linearize and cimpc_plant_sensitivity stage them: z | theta | terrains packed
// into `host`, the workspace's d_lin_in grown to take them and one upload enqueued on the workspace's stream.  The caller holds
// g_plant_mu and keeps the PlantKnots until it has synchronized the stream.  n_terrain_up: PlantLinearizeDims' (0: d_ter is null).
// False: the buffer could not be grown or the copy not enqueued.
struct PlantWs;
struct PlantKnots {
    std::vector<double> host;
    const double *d_z = nullptr, *d_th = nullptr;
    const cimpc_terrain* d_ter = nullptr;
};
bool plant_stage_knots(PlantWs& W, int N, int nz, int nth, int n_terrain_up, const double* z, const double* theta, const cimpc_terrain* terrain,
                       PlantKnots* k);

// N knots on `st`, the kernel instantiation cimpc_plant_linearize takes.  Device pointers: z N x nz, theta N x nth, d_ter
// n_terrain (1 or N) terrains or null; outputs r0 N x nz, rz0 N x (nz x nz), rth0 N x (nz x nth), column-major, a null one is
// skipped.  No synchronization.  False: unknown model or a failed launch.
bool plant_linearize_launch(int model, int N, const double* d_z, const double* d_th, const cimpc_terrain* d_ter, int n_terrain, double kappa,
                            double* d_r, double* d_rz, double* d_rth, hipStream_t st);

}  // namespace cimpc
