// The step gradients of the plant models (plant_sensitivity.hip) for callers inside the library that bring their own device buffers
// and stream: cimpc_plant_rollout_grad (plant_kernel.hip) runs the kernel behind the rollout's chunks, on the rollout's stream.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/cimpc.h"
#include "plant_model.h"

namespace cimpc {

// Where the z and theta of entry e come from, all device memory.  Knots (q == nullptr): z N x nz and theta N x ntheta as they stand, entry e
// on terrain[e].  A rollout (q != nullptr) of B robots: entry e = t B + rb reads z[e], and theta = [q0; q1; u1; w1; mu; h] is put together
// from the trajectory rows t, t + 1, the schedule rows of step t (plant_rollout_plan.h), mu and h - the theta plant_step_kernel
// stepped on; robot rb stands on terrain[rb]; an entry whose step_status is 0 is not differentiated.
struct PlantSensSource {
    const double *z, *theta;
    const double *q, *u, *w, *mu;
    const int* step_status;
    double mu0, h;
    int B, K_u, n_u, hold_u, K_w, n_w, hold_w, n_mu;
};

// N entries on `st`, one workgroup each: dz N x (nr x n_cols) column-major, nr = nq + nc + nb; status N words (1: done; 0: the step
// had status 0, a pivot was zero or not finite, or a result was not finite - that entry's block is all zeros).  d_ter: n_terrain (1
// or one per knot / robot) terrains, or null (flat ground).  The caller has checked plant_sensitivity_fits(nz, n_cols).  No
// synchronization.  False: a failed launch.
bool plant_sensitivity_launch(const PlantModel& M, int N, const PlantSensSource& src, const cimpc_terrain* d_ter, int n_terrain, double reg,
                              int n_cols, double* d_dz, int* d_status, hipStream_t st);

}  // namespace cimpc
