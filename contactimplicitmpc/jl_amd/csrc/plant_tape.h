// The device side of a rollout's tape (plant_adjoint.hip owns the rest): where cimpc_plant_rollout_tape has the sensitivity launch of a
// rollout write.  Kept apart from plant_adjoint.h, whose arithmetic is compiled without contraction: plant_kernel.hip includes this
// header and must keep contracting: the open-loop results of its step kernels depend on it bit for bit (plant_feedback.h, which that file
// does include, switches contraction off inside its own function bodies only).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/cimpc.h"
#include "plant_model.h"
#include "plant_rollout_call.h"

namespace cimpc {

struct PlantTapeBuffers {
    double* d_dz = nullptr;      // T x B x (nr x n_cols), the blocks as plant_sensitivity_kernel writes them
    int* d_status = nullptr;     // T x B
    int device = -1;
    PlantModel M{};
    double* d_fb_K = nullptr;    // a closed-loop tape's copy of the gain rows, K_f x n_f x (nu x 2nq); null: an open-loop tape
    int K_f = 1, n_f = 1, hold_f = 1;
    double n_sample = 1.0;
    int* d_clamped = nullptr;    // a limited closed-loop tape's mask words, T x B (plant_feedback_clamped); null: no limits

    // Frees whichever of the four allocations are set, on the current device, and nulls them.  False: a free failed.
    bool release() {
        bool ok = true;
        if (d_dz) ok = hipFree(d_dz) == hipSuccess;
        if (d_status) ok = (hipFree(d_status) == hipSuccess) && ok;
        if (d_fb_K) ok = (hipFree(d_fb_K) == hipSuccess) && ok;
        if (d_clamped) ok = (hipFree(d_clamped) == hipSuccess) && ok;
        d_dz = nullptr; d_status = nullptr; d_fb_K = nullptr; d_clamped = nullptr;
        return ok;
    }
};

// A rollout with call.grad->tape set (plant_kernel.hip): cimpc_plant_rollout_grad's body with one change - after the check and under
// the plant mutex it allocates d_dz and d_status on the current device, has the sensitivity launch target them DIRECTLY (no copy
// through the workspace's d_grad), reads the status back and leaves dz on the device.  On any failure the pointers are null and
// nothing stays allocated.  With call.loop (cimpc_plant_rollout_tape_feedback) the tape also gets d_fb_K and the schedule's
// (K_f, n_f, hold_f, n_sample).  With limits on that loop (cimpc_plant_rollout_tape_feedback_limits) it also gets d_clamped, which
// plant_clamp_mask_kernel fills behind the rollout's chunks from u_applied and the limits where they lie on the device.
int plant_rollout_to_tape(const PlantRolloutCall& call, PlantTapeBuffers* tape);

}  // namespace cimpc

// What a cimpc_plant_tape points to: plant_adjoint.hip makes and frees it, the reverse chain there, the forward chain of
// plant_tangent.hip and the LQ backward pass of plant_riccati.hip walk it.
struct cimpc_plant_tape_s {
    cimpc::PlantTapeBuffers buf;      // the device memory, its device and model; buf.d_fb_K non-null: a closed-loop tape
    int model, B, T, n_cols;
};
