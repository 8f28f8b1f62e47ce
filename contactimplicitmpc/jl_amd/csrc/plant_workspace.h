// Per-device workspace of the plant entry points (plant_kernel.hip: step, terrain step, rollout; plant_linearize.hip: linearize; plant_sensitivity.hip: step gradients; plant_adjoint.hip: the reverse chain; plant_tangent.hip: the forward chain):
// buffers and a private stream live across calls (a simulator step is called thousands of times in a closed loop; allocating and a
// device-wide synchronize per call stalled everything else on the GPU).  One mutex serializes the entry points; each keeps buffers
// of its own, grow-only, and all share the stream.
//   step / rollout  d_in, d_out, d_st, d_z, d_grad, d_grad_st, d_fb: the regions of each, their order and sizes are plant_rollout_layout's
//                   (plant_rollout_call.h); d_ter: the robots' terrains
//   linearize       d_lin_in: z | theta | terrains (N x nz, N x nth, n_terrain cimpc_terrain); d_lin_out: r0 | rz0 | rth0 (those asked for)
//   step gradients  cimpc_plant_sensitivity: d_grad: dz (N x nr x n_cols); d_grad_st: status (N); it stages its knots in d_lin_in
//   reverse chain   d_adj_in: gq | ggamma | gb (those given); d_adj_out: g_q0 | g_q1 | g_u_step | g_w_step | g_mu | g_h; d_adj_cut: n_cut (B);
//                   d_adj_xref: g_xref_step (T x B x 2nq) of a closed-loop tape.
//   forward chain   d_tan_in: dq0 | dq1 | du_step | dw_step | dmu | dh | dxref_step (those given), each with a leading axis of n_dir;
//                   d_tan_out: dq | dgamma | db | du_applied (those asked for); d_tan_cut: n_cut (B)   (plant_tangent.hip)
//   line search     the rollout of its n_alpha x B candidates in d_in, d_out, d_st, d_z, d_fb, d_ter, laid out as a closed-loop tape call of that
//                   many robots (K in d_fb); its B-robot inputs and outputs in buffers of its own   (plant_linesearch.hip)
//   iLQR loop       the same candidates' rollout, iteration after iteration; the nominal, the gains, the rules' rows, the line search's outputs
//                   and the history in two buffers of its own   (plant_ilqr.hip)
//   MPC policy      the same candidates' rollout at every control step; everything else - the problem, the plan, its nominal, three tape
//                   buffers - belongs to the cimpc_plant_mpc handle, which copies its terrains into d_ter at every step   (plant_mpc.hip)
//   sampling policy the candidates' open-loop rollout in d_in, d_out, d_st, d_ter; the problem and the plan belong to the
//                   cimpc_plant_sampler handle   (plant_sample.hip)
//   shooting        cimpc_plant_rollout_segments: the M B virtual robots' rollout in d_in, d_out, d_st, d_z, d_ter and their blocks in d_grad,
//                   d_grad_st, laid out as a gradient call of that many robots over T / M steps; _shooting_linesearch: its n_alpha M B
//                   candidates as a closed-loop tape call (K in d_fb), the chosen segments' blocks in d_grad, d_grad_st before they are
//                   stitched into the new tape; the B-robot inputs and stitched outputs in buffers of its own   (plant_shooting.hip)
//   The stage entries' own buffers (LQ pass, line search, iLQR loop, shooting) are a PlantStageWs each, below; their regions are laid
//   out and copied by plant_staging.h
//                   A tape's dz and status are NOT here: they belong to the tape (plant_adjoint.hip) and live as long as it does
// The prologue the entry points share past their validation (plant_model_and_ground, plant_model.h; plant_rollout_check,
// plant_rollout_call.h: no device needed) is stated here once: which device a call runs on (plant_current_device), and its workspace
// with the stream open (plant_ws_open), the device a tape or a handle lives on selected for the call (PlantDeviceScope), and the
// staging copies on the workspace's stream (PlantStreamCopier).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>

#include "../../../include/cimpc.h"
#include "plant_model.h"
#include "plant_staging.h"

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
    double *d_z = nullptr, *d_grad = nullptr;
    int* d_grad_st = nullptr;
    size_t cap_z = 0, cap_grad = 0, cap_grad_st = 0;
    double *d_adj_in = nullptr, *d_adj_out = nullptr;
    int* d_adj_cut = nullptr;
    size_t cap_adj_in = 0, cap_adj_out = 0, cap_adj_cut = 0;
    double *d_fb = nullptr, *d_adj_xref = nullptr;
    size_t cap_fb = 0, cap_adj_xref = 0;
    double *d_tan_in = nullptr, *d_tan_out = nullptr;
    int* d_tan_cut = nullptr;
    size_t cap_tan_in = 0, cap_tan_out = 0, cap_tan_cut = 0;
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

// Frees *p where it is set, and clears it
template <class T>
bool plant_free(T** p) {
    const bool ok = !*p || hipFree(*p) == hipSuccess;
    *p = nullptr;
    return ok;
}

// The calling thread's CURRENT device (the caller selects it, e.g. hipSetDevice(rank) / torch.cuda.set_device), which every plant
// entry point runs on.  False: none that has a workspace, or not a gfx950.
inline bool plant_current_device(int* dev) {
    if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev >= PLANT_MAX_DEVICES) return false;
    hipDeviceProp_t prop;
    return hipGetDeviceProperties(&prop, *dev) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

// The workspace of device `dev`, its stream opened on first use; the caller holds g_plant_mu.  Null: the stream could not be created.
inline PlantWs* plant_ws_open(int dev) {
    PlantWs& W = g_plant_ws[dev];
    if (!W.st) {
        if (hipStreamCreateWithFlags(&W.st, hipStreamNonBlocking) != hipSuccess) return nullptr;
        W.device = dev;
    }
    return &W;
}

// Grow-only device buffers of one stage entry, per device, next to the plant workspace whose stream and mutex the entry uses: doubles in,
// doubles out, ints.  Each entry keeps an array of its own (g_*_ws in its file); an entry that stages everything in one buffer of doubles
// leaves d_out alone.
struct PlantStageWs {
    double *d_in = nullptr, *d_out = nullptr;
    int* d_int = nullptr;
    size_t cap_in = 0, cap_out = 0, cap_int = 0;
    bool grow(size_t in, size_t out, size_t ints) { return plant_grow(&d_in, &cap_in, in) && plant_grow(&d_out, &cap_out, out) && plant_grow(&d_int, &cap_int, ints); }
};

// g_plant_mu held and device `dev` selected, from the constructor until the object goes; rc(): CIMPC_OK, or why `dev` could not be
// selected (nothing to undo then).  leave(ok) selects the caller's device again and folds a failure to do so into ok; the mutex stays
// held, so an entry whose new tape must not outlive a failed restore can still release it.
class PlantDeviceScope {
public:
    explicit PlantDeviceScope(int dev) : dev_(dev) {
        if (hipGetDevice(&cur_) != hipSuccess) rc_ = CIMPC_ERR_NO_DEVICE;
        else if (cur_ != dev_ && hipSetDevice(dev_) != hipSuccess) rc_ = CIMPC_ERR_HIP;
        entered_ = rc_ == CIMPC_OK;
    }
    ~PlantDeviceScope() { (void)leave(true); }
    int rc() const { return rc_; }
    bool leave(bool ok) {
        if (entered_ && cur_ != dev_) ok = (hipSetDevice(cur_) == hipSuccess) && ok;
        entered_ = false;
        return ok;
    }

private:
    std::lock_guard<std::mutex> lock_{g_plant_mu};
    int dev_, cur_ = -1, rc_ = CIMPC_OK;
    bool entered_ = false;
};

// `body` on the device of a handle (cimpc_plant_mpc, cimpc_plant_sampler: `device`, `failed`) under the plant mutex; a HIP error latches
// the handle.
template <class Handle, class Body>
int plant_handle_on_device(Handle* h, Body&& body) {
    PlantDeviceScope scope(h->device);
    if (scope.rc() != CIMPC_OK) return scope.rc();
    const bool ok = scope.leave(body());
    if (!ok) h->failed = true;
    return ok ? CIMPC_OK : CIMPC_ERR_HIP;
}

// plant_staging.h's copier on a stream: PlantStreamCopier copy{{st}, ok};
struct PlantStreamCopy {
    hipStream_t st;
    bool operator()(void* d, const void* s, size_t bytes, bool up) const { return hipMemcpyAsync(d, s, bytes, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st) == hipSuccess; }
};
using PlantStreamCopier = PlantCopier<PlantStreamCopy>;

}  // namespace cimpc
