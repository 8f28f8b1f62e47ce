// One call of the device rollout, stated once (plain C++, host only: tests/native/plant_rollout_call_check.cpp builds it with g++):
// what the call is given (PlantRolloutCall), every test made on it before a device is touched (plant_rollout_check), and where each
// of its arrays lives in the plant workspace's grow-only buffers (plant_rollout_layout).  The eight entry points - cimpc_plant_step,
// _step_terrain, _rollout, _rollout_grad, _rollout_tape and the three _feedback ones - fill a PlantRolloutCall from their C parameter
// lists and hand it to plant_rollout_impl (plant_kernel.hip), which reads its pointers off the layout; so do the three _feedback_limits
// entries, whose limits plant_limits_refusal tests by reason.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <optional>

#include "../../../include/cimpc.h"
#include "plant_model.h"
#include "plant_sensitivity_plan.h"
#include "plant_staging.h"

namespace cimpc {

// K x n x width doubles on the host, row k held for `hold` steps (rollout_row); n = 1: one schedule for every robot, B: one per robot
struct PlantSchedule { const double* rows; int K, n, hold; };

// The step gradients of every step (the _grad and _tape entry points): dz T x B x (nr x n_cols), its status T x B and, when asked for,
// z T x B x nz.  tape: dz stays on the device in memory the tape owns (plant_tape.h), dz is not read, and n_cols >= 2 nq + nu.
struct PlantRolloutGrad {
    double reg;
    int n_cols;
    double *z, *dz;      // z may be null
    int* status;
    bool tape;
};

// A closed loop (the _feedback entry points): the host schedule and where u_applied (T x B x nu) and fb_err (T x B x 2nq) go
// u_lo, u_hi (both or neither): the limited law of plant_feedback.h, n_lim x nu host rows, n_lim 1 or B.  With grad the blocks are taken
// with the applied control as theta's column, so they do not see the clamp; with a tape the tape also owns the mask of clamped controls
// (DESIGN.md section 3, item 3i), and clamped (T x B words) is where it comes back: limits on a tape without it are refused.
struct PlantRolloutLoop {
    const cimpc_feedback* fb;
    double *u_applied, *fb_err;
    const double *u_lo = nullptr, *u_hi = nullptr;
    int n_lim = 1;
    int* clamped = nullptr;
};

// Everything a rollout call is given.  A simulator step is T = 1, steps_per_launch = 1, one u and one w row per robot, n_mu = 1 and
// q_row0 = 2 (trajectory row 2 alone comes back).
struct PlantRolloutCall {
    int model, B, T, steps_per_launch;
    int n_terrain;
    const cimpc_terrain* terrain;
    bool needs_terrain = false;      // cimpc_plant_step_terrain: a null terrain is refused; every other entry pairs terrain with its count
    const double *q0, *q1;
    PlantSchedule u, w;      // w.rows may be null: no disturbance
    const double* mu;
    int n_mu;
    double h;
    const cimpc_ip_opts* opts;
    double* q;
    int q_row0 = 0;          // the first trajectory row that is read back into q
    double *gamma, *b;
    int *status, *iters;
    std::optional<PlantRolloutGrad> grad;
    std::optional<PlantRolloutLoop> loop;
};

// The fields the six rollout entry points fill from the 25 parameters they share (cimpc_plant_rollout, include/cimpc.h), by the
// parameters' names and stated once, so that no entry can transpose two of them: {PLANT_ROLLOUT_CALL_BASE, .grad = ..., .loop = ...}.
#define PLANT_ROLLOUT_CALL_BASE                                                                                                             \
    .model = model, .B = B, .T = T, .steps_per_launch = steps_per_launch, .n_terrain = n_terrain, .terrain = terrain, .q0 = q0, .q1 = q1, \
    .u = {u, K_u, n_u, hold_u}, .w = {w, K_w, n_w, hold_w}, .mu = mu, .n_mu = n_mu, .h = h, .opts = opts, .q = q, .gamma = gamma, .b = b,  \
    .status = status, .iters = iters

// Where a call's arrays live, in elements of each buffer of PlantWs (plant_workspace.h), and what plant_grow is asked for (need_*; 0:
// the call does not use the buffer).  The regions of a buffer follow each other in the order they are listed, without gaps; one that
// the call does not have takes no room.
struct PlantRolloutLayout {
    size_t row = 0, TB = 0;                        // B x nq doubles of one trajectory row; T x B steps
    PlantSpan q, u, w, mu;                         // d_in: trajectory (T + 2) x B x nq | u schedule | w schedule | per-robot mu (n_mu = B)
    PlantSpan gamma, b;                            // d_out: T x B x nc | T x B x nb
    PlantSpan status, iters;                       // d_st: T x B each
    PlantSpan z;                                   // d_z: T x B x nz, with grad
    PlantSpan dz, grad_status;                     // d_grad, d_grad_st - or, with a tape, the tape's d_dz and d_status, and need_grad* = 0
    PlantSpan fb_K, x_ref, u_applied, fb_err;      // d_fb, with loop; with a tape K is read from the tape's d_fb_K and the K region stays unused
    PlantSpan u_lo, u_hi;                          // d_fb, behind them, with limits: n_lim x nu each
    size_t need_in = 0, need_out = 0, need_st = 0, need_z = 0, need_grad = 0, need_grad_st = 0, need_fb = 0;
};

inline PlantRolloutLayout plant_rollout_layout(const PlantModel& M, const PlantRolloutCall& c) {
    PlantRolloutLayout L;
    const size_t nq = M.nq, nu = M.nu, nr = nq + (size_t)M.nc + (size_t)M.nb();
    L.row = (size_t)c.B * nq;
    L.TB = (size_t)c.T * c.B;
    PlantCursor at;
    L.q = at.take((size_t)(c.T + 2) * L.row);
    L.u = at.take((size_t)c.u.K * c.u.n * nu);
    L.w = at.take(c.w.rows ? (size_t)c.w.K * c.w.n * M.nw : 0);
    L.mu = at.take(c.n_mu == 1 ? 0 : (size_t)c.B);
    L.need_in = at.end();
    L.gamma = at.take(L.TB * M.nc);
    L.b = at.take(L.TB * M.nb());
    L.need_out = at.end();
    L.status = at.take(L.TB);
    L.iters = at.take(L.TB);
    L.need_st = at.end();
    if (c.grad) {
        L.z = at.take(L.TB * M.nz());
        L.need_z = at.end();
        L.dz = at.take(L.TB * nr * (size_t)c.grad->n_cols);
        L.need_grad = at.end();
        L.grad_status = at.take(L.TB);
        L.need_grad_st = at.end();
        if (c.grad->tape) L.need_grad = L.need_grad_st = 0;
    }
    if (c.loop) {
        const size_t n_x = (size_t)c.loop->fb->K_f * c.loop->fb->n_f * 2 * nq;
        L.fb_K = at.take(n_x * nu);
        L.x_ref = at.take(n_x);
        L.u_applied = at.take(L.TB * nu);
        L.fb_err = at.take(L.TB * 2 * nq);
        if (c.loop->u_lo) {
            L.u_lo = at.take((size_t)c.loop->n_lim * nu);
            L.u_hi = at.take((size_t)c.loop->n_lim * nu);
        }
        L.need_fb = at.end();
    }
    return L;
}

// Why the limits of a closed loop are refused, or null when they stand: what the three _feedback_limits entries leave for
// cimpc_last_error(NULL), in the order cimpc_plant_rollout_feedback_limits has tested them since it exists.  tape: the call records a tape.
inline const char* plant_limits_refusal(int model, int B, const PlantRolloutLoop& l, bool tape) {
    if (!l.u_lo || !l.u_hi) return "a null u_lo or u_hi";
    if (l.n_lim != 1 && l.n_lim != B) return "n_lim neither 1 nor B";
    PlantModel named{};
    if (!plant_model_by_id(model, &named) || named.nu < 1) return "a model without controls";
    const size_t n = l.n_lim > 0 ? (size_t)l.n_lim * named.nu : 0;
    for (size_t e = 0; e < n; ++e) {
        if (l.u_lo[e] != l.u_lo[e] || l.u_hi[e] != l.u_hi[e]) return "a NaN limit";
        if (l.u_lo[e] > l.u_hi[e]) return "u_lo above u_hi";
    }
    if (tape && !l.clamped) return "limits on a tape without clamped";
    return nullptr;
}

// Every test of a call that needs no device.  CIMPC_OK: *M is the call's model and *rough says whether its terrains have to reach the
// device; CIMPC_ERR_INVALID: the call is refused.  K and x_ref are read (they must be finite) only after every test on the schedule
// that owns them.
inline int plant_rollout_check(const PlantRolloutCall& c, PlantModel* M, bool* rough) {
    const int B = c.B;
    if (c.needs_terrain ? !c.terrain : (c.n_terrain != 0) != (c.terrain != nullptr)) return CIMPC_ERR_INVALID;
    if (B <= 0 || !c.q0 || !c.q1 || !c.u.rows || !c.opts || !c.q || !c.gamma || !c.b || !c.status || !c.iters || c.h <= 0.0) return CIMPC_ERR_INVALID;
    if (c.T < 1 || c.steps_per_launch < 0 || c.u.K < 1 || c.u.hold < 1 || (c.u.n != 1 && c.u.n != B) || !c.mu || (c.n_mu != 1 && c.n_mu != B))
        return CIMPC_ERR_INVALID;
    if (c.w.rows && (c.w.K < 1 || c.w.hold < 1 || (c.w.n != 1 && c.w.n != B))) return CIMPC_ERR_INVALID;
    if (!plant_model_and_ground(c.model, B, c.n_terrain, c.terrain, M, rough)) return CIMPC_ERR_INVALID;
    const cimpc_ip_opts& o = *c.opts;
    if (o.max_iter <= 0 || o.max_ls < 0 || !(o.r_tol > 0.0) || !(o.kappa_tol > 0.0) || !(o.ls_scale > 0.0 && o.ls_scale < 1.0)) return CIMPC_ERR_INVALID;
    if (c.grad) {
        const PlantRolloutGrad& g = *c.grad;
        if ((!g.dz && !g.tape) || !g.status || !std::isfinite(g.reg) || g.reg < 0.0 || g.n_cols < 1 || g.n_cols > M->nth() ||
            !plant_sensitivity_fits(M->nz(), g.n_cols) || (long long)c.T * B > INT_MAX)
            return CIMPC_ERR_INVALID;
        if (g.tape && g.n_cols < 2 * M->nq + M->nu) return CIMPC_ERR_INVALID;
    }
    if (c.loop) {
        const cimpc_feedback* f = c.loop->fb;
        if (!f || !f->K || !f->x_ref || !c.loop->u_applied || !c.loop->fb_err || f->K_f < 1 || f->hold_f < 1 || (f->n_f != 1 && f->n_f != B) ||
            !std::isfinite(f->n_sample) || !(f->n_sample > 0.0) || 2 * M->nq > M->nz())
            return CIMPC_ERR_INVALID;
        const PlantRolloutLayout L = plant_rollout_layout(*M, c);
        for (size_t i = 0; i < L.fb_K.n; ++i) if (!std::isfinite(f->K[i])) return CIMPC_ERR_INVALID;
        for (size_t i = 0; i < L.x_ref.n; ++i) if (!std::isfinite(f->x_ref[i])) return CIMPC_ERR_INVALID;
        // limits: both arrays, n_lim 1 or B, no NaN, u_lo <= u_hi, and on a tape somewhere for the mask to go
        if ((c.loop->u_lo || c.loop->u_hi) && plant_limits_refusal(c.model, B, *c.loop, c.grad && c.grad->tape)) return CIMPC_ERR_INVALID;
    }
    return CIMPC_OK;
}

}  // namespace cimpc
