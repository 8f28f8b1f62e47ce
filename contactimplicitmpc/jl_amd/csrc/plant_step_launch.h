// The step kernel's chunked launches (plant_kernel.hip) for callers inside the library that bring their own device buffers and stream:
// every rollout entry point, and the line search (plant_linesearch.hip), which steps n_alpha x B candidate robots in one rollout.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/cimpc.h"
#include "plant_feedback.h"
#include "plant_model.h"

namespace cimpc {

// What the steps 0 .. T-1 of a rollout of B robots read and write, all device memory; the arrays are those of PlantRollout
// (plant_kernel.hip): q (T + 2) x B x nq with rows 0 and 1 set, the u and w schedules (w null: none), mu (n_mu = B; with n_mu = 1 mu0 is
// used), per-step gamma, b, status, iters, z (null: not stored).  fb.K non-null: the closed loop of plant_feedback.h, with u_applied
// T x B x nu and fb_err T x B x 2nq; lim.u_lo non-null (with fb.K): the limited law, n_lim = 1 or B rows of nu limits.
struct PlantStepArrays {
    double* q;
    const double *u, *w, *mu;
    double *gamma, *b;
    int *status, *iters;
    double mu0, h;
    int K_u, n_u, hold_u, K_w, n_w, hold_w, n_mu;
    double* z;
    PlantFeedback fb;
    double *u_applied, *fb_err;
    PlantFeedbackLimits lim{};
};

// The rollout's chunks (plant_rollout_plan.h) back to back on `st`; the trajectory buffer carries the state, nothing is synchronized.
// rough: the terrains d_ter (n_terrain: 1 or B) are read.  False: a failed launch, and nothing more was put on the stream.
bool plant_step_chunks(const PlantModel& M, bool rough, const cimpc_ip_opts& opts, int B, int T, int steps_per_launch, const PlantStepArrays& a,
                       const cimpc_terrain* d_ter, int n_terrain, hipStream_t st);

}  // namespace cimpc
