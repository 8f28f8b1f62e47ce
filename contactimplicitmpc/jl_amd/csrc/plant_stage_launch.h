// The host-side launch code of the line search (plant_linesearch.hip) and of the limited backward pass (plant_riccati.hip) for callers
// inside the library whose arrays are already on the device: the two C entries themselves, and the device-resident iLQR loop
// (plant_ilqr.hip), which chains them iteration after iteration without a copy in between.
//
//   plant_linesearch_plan      everything cimpc_plant_tape_linesearch[_box] validates of its host arguments past its null pointers, and
//                              what it derives from them: the model, the cost's sizes, the candidates' rollout layout (no device needed)
//   plant_linesearch_terrains  the candidates' terrains: robot b's for every c (empty: the caller's array serves as it stands)
//   plant_linesearch_shared    the uploads that do not pass through the expansion kernel: a shared w schedule, the terrains
//   plant_linesearch_stages    the kernels of one line search back to back on `st`: expand, the step kernel's chunks, cost, gather, ONE
//                              sensitivity launch, restore.  Nothing is copied or synchronized.
//   plant_riccati_box_launch   plant_riccati_kernel<true, true> on `st`
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../../include/cimpc.h"
#include "plant_cost.h"
#include "plant_model.h"
#include "plant_riccati.h"
#include "plant_rollout_call.h"
#include "plant_tape.h"
#include "plant_workspace.h"

namespace cimpc {

// The host arguments a line search is planned from (the names of cimpc_plant_tape_linesearch_box).  q .. grad_status are the caller's
// output arrays: only that they are given is looked at.
struct PlantLsCall {
    cimpc_plant_tape tape;
    int steps_per_launch, n_terrain;
    const cimpc_terrain* terrain;
    const double *q_nom, *u_nom, *w;
    int K_w, n_w, hold_w;
    const double* mu;
    int n_mu;
    double h;
    const cimpc_ip_opts* opts;
    int n_alpha;
    const double* alpha;
    double armijo;
    const cimpc_tracking_cost* cost;
    double reg;
    double *q, *u_applied, *gamma, *b;
    int *status, *iters, *grad_status;
    int n_lim;
    const double *u_lo, *u_hi;
};

struct PlantLsPlan {
    PlantModel M{};
    bool rough = false, has_w = false, w_each = false, mu_each = false, ter_each = false, limits = false, lim_each = false;
    PlantCost C{};      // the cost with the caller's (host) pointers and the tape's T, nq, nu
    PlantRolloutLayout L{};
    int model = 0, B = 0, T = 0, NB = 0, n_alpha = 0, n_cols = 0, steps_per_launch = 0, K_w = 1, n_w = 1, hold_w = 1, n_mu = 1, n_terrain = 0, n_ter = 0,
        n_lim = 1;
    double mu0 = 0.0, h = 0.0, armijo = 0.0, reg = 0.0;
    cimpc_ip_opts opts{};
};

// One line search's arrays, all device memory.  In: the nominal's q (T + 2) x B x nq and u T x B x nu, the gains k, K (column-major
// blocks), dV, J_nom, alpha; w (K_w x B x nw) and mu (B) where they are per robot, else null; the limits (n_lim x nu) or null; C with
// device pointers; the parent tape's blocks.  Out: J and conv of the NB candidates, ok, choice, the chosen rows, the new tape's blocks.
struct PlantLsArrays {
    const double *q_nom, *u_nom, *k, *K, *w, *mu, *dV, *J_nom, *alpha, *u_lo, *u_hi;
    PlantCost C;
    double* J;
    int *ok, *choice, *conv;
    double *Cq, *Cz, *Cu, *Cg, *Cb;
    int *Cst, *Cit;
    double *lin_q, *lin_r;
    const double* parent_dz;
    const int* parent_status;
    double* dz;
    int* status;
};

// The reason of a refusal, or null with *P filled.  The caller has tested c.tape and the pointers of its own argument list.
const char* plant_linesearch_plan(const PlantLsCall& c, PlantLsPlan* P);
std::vector<cimpc_terrain> plant_linesearch_terrains(const PlantLsPlan& P, const cimpc_terrain* terrain);
// ter: plant_linesearch_terrains' (it must outlive the stream's work).  W's buffers hold P.L and P.n_ter terrains.
bool plant_linesearch_shared(const PlantLsPlan& P, const double* w, const cimpc_terrain* terrain, const std::vector<cimpc_terrain>& ter, PlantWs& W,
                             hipStream_t st);
bool plant_linesearch_stages(const PlantLsPlan& P, const PlantLsArrays& A, PlantWs& W, hipStream_t st);

// L with every pointer on the device, q and r given; sets the kernel's dynamic LDS (plant_riccati_box_lds) and launches B workgroups.
bool plant_riccati_box_launch(const PlantRiccati& L, hipStream_t st);

}  // namespace cimpc
