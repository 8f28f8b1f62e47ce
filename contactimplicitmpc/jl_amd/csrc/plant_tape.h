// The device side of a rollout's tape (plant_adjoint.hip owns the rest): where cimpc_plant_rollout_tape has the sensitivity launch of a
// rollout write.  Kept apart from plant_adjoint.h, whose arithmetic is compiled without contraction: plant_kernel.hip includes this
// header and must keep contracting: the open-loop results of its step kernels depend on it bit for bit (plant_feedback.h, which that file
// does include, switches contraction off inside its own function bodies only).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/cimpc.h"
#include "plant_model.h"

namespace cimpc {

struct PlantTapeBuffers {
    double* d_dz = nullptr;      // T x B x (nr x n_cols), the blocks as plant_sensitivity_kernel writes them
    int* d_status = nullptr;     // T x B
    int device = -1;
    PlantModel M{};
    double* d_fb_K = nullptr;    // a closed-loop tape's copy of the gain rows, K_f x n_f x (nu x 2nq); null: an open-loop tape
    int K_f = 1, n_f = 1, hold_f = 1;
    double n_sample = 1.0;
};

// cimpc_plant_rollout_grad's body (plant_kernel.hip) with one change: after its validation - which also asks n_cols >= 2 nq + nu - and
// under the plant mutex it allocates d_dz and d_status on the current device, has the sensitivity launch target them DIRECTLY (no copy
// through the workspace's d_grad), reads the status back and leaves dz on the device.  On any failure both pointers are null and
// nothing stays allocated.  closed_loop: cimpc_plant_rollout_tape_feedback - the rollout runs under fb (validated with the rest; a null fb
// is refused), u_applied and fb_err come back, and the tape also gets d_fb_K and the schedule's (K_f, n_f, hold_f, n_sample).
int plant_rollout_to_tape(int model, int B, int T, int steps_per_launch, int n_terrain, const cimpc_terrain* terrain, const double* q0,
                          const double* q1, const double* u, int K_u, int n_u, int hold_u, const double* w, int K_w, int n_w, int hold_w,
                          const double* mu, int n_mu, double h, const cimpc_ip_opts* opts, double* q, double* gamma, double* b, int* status,
                          int* iters, double reg, int n_cols, double* z, int* grad_status, PlantTapeBuffers* tape, bool closed_loop = false,
                          const cimpc_feedback* fb = nullptr, double* u_applied = nullptr, double* fb_err = nullptr);

}  // namespace cimpc
