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
//   plant_restore_launch       the last of those stages on its own
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

constexpr int LS_THREADS = 64;
constexpr int LS_MAX_WORK = (int)plant_cost_work_doubles(PLANT_MAX_Q, PLANT_MAX_U);

// the wavefront as the team of plant_cost.h: the line search's kernels (plant_linesearch.hip) and the policy's nominal kernel (plant_mpc.hip)
struct PlantCostWave {
    __device__ int rank() const { return threadIdx.x; }
    __device__ int size() const { return LS_THREADS; }
    __device__ void sync() const { __syncthreads(); }
};

// A workgroup of THREADS as the team of a chain that fetches the next step's corner while it works a step (plant_riccati.h's Team;
// plant_shoot_forward_chain's): fetch_issue loads up to STAGE x THREADS doubles of the rows x cols corner of a column-major block with
// leading dimension ld into registers, fetch_commit leaves them packed in dst and reads what did not fit straight from src.
template <int THREADS, int STAGE>
struct PlantCornerTeam {
    double stage[STAGE];
    __device__ int rank() const { return threadIdx.x; }
    __device__ int size() const { return THREADS; }
    __device__ void sync() const { __syncthreads(); }
    __device__ void fetch_issue(const double* src, int rows, int cols, int ld) {
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = k * THREADS + (int)threadIdx.x;
            stage[k] = i < rows * cols ? src[(size_t)(i / rows) * ld + i % rows] : 0.0;
        }
    }
    __device__ void fetch_commit(double* dst, const double* src, int rows, int cols, int ld) {
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = k * THREADS + (int)threadIdx.x;
            if (i < rows * cols) dst[i] = stage[k];
        }
        for (int i = STAGE * THREADS + (int)threadIdx.x; i < rows * cols; i += THREADS) dst[i] = src[(size_t)(i / rows) * ld + i % rows];
    }
};

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
// plant_ls_cost_kernel on `st`, all device memory: J and conv (every step converged) of the NB = n B candidates (c B + b) of a rollout with
// trajectory q (T + 2) x NB x nq, applied controls u_applied T x NB x nu and status T x NB; C with device pointers and the rollout's T, nq, nu.
// The line search calls it, and so does the sampling policy (plant_sample.hip).
bool plant_candidates_cost_launch(const PlantCost& C, const double* q, const double* u_applied, const int* status, double* J, int* conv, int B, int NB,
                                  hipStream_t st);

// plant_ls_restore_kernel on `st`, all device memory: entry t B + b of the new tape (dz: blocks of `block` doubles; status) gets the parent's
// where choice[b] < 0.  The line search calls it, and so does the line search of multiple shooting (plant_shooting.hip; section 3, item 3l).
bool plant_restore_launch(const int* choice, const double* parent_dz, const int* parent_status, double* dz, int* status, int B, int T, int block,
                          hipStream_t st);

// One iteration of the device-resident iLQR loop (plant_ilqr.hip), all device memory: the rules' state
// (ladder, level, active, J; plant_ilqr.h) and rows (rho_b, J_nom), the nominal (N*), the backward pass's outputs, the limits (null: none),
// alpha, w and mu where they are per robot (else null), C with device pointers, the line search's outputs (PlantLsArrays' names), and the
// history: max_iter rows of B and max_iter words of n_active, of which iteration `it` writes its own.
struct PlantIlqrArrays {
    const double* ladder;
    int *level, *active;
    double *J, *rho_b, *J_nom;
    double *Nq, *Nu, *Ng, *Nb, *Nlq, *Nlr;
    int *Nst, *Nit;
    double *K, *k, *dV;
    int *lq_status, *n_cut, *clamped;
    const double *u_lo, *u_hi;
    const double *alpha, *w, *mu;
    PlantCost C;
    double* J_cand;
    int *ok, *choice, *conv;
    double *Cq, *Cz, *Cu, *Cg, *Cb;
    int *Cst, *Cit;
    double *Clq, *Clr;
    double *hist_J, *hist_alpha, *hist_rho;
    int *hist_accepted, *n_active;
    double rho_max, tol;
};

// The body of the loop on `st`, nothing copied or synchronized: the rho kernel, plant_riccati_box_launch about the parent tape's blocks, the
// nominal-cost kernel, plant_linesearch_stages into the fresh blocks, the commit kernel.  cimpc_plant_ilqr and cimpc_plant_mpc_control call it.
bool plant_ilqr_iteration(const PlantLsPlan& P, const PlantIlqrArrays& A, int it, const double* parent_dz, const int* parent_status, double* dz,
                          int* status, PlantWs& W, hipStream_t st);

// L with every pointer on the device, q and r given; sets the kernel's dynamic LDS (plant_riccati_box_lds) and launches B workgroups.
bool plant_riccati_box_launch(const PlantRiccati& L, hipStream_t st);

}  // namespace cimpc
