// How a plant entry stages its arrays, stated once (plain C++, host only: tests/native/plant_staging_check.cpp builds it with g++).  An
// array's extent is stated ONCE, where its region is taken from the layout cursor; the copies up and down and the device pointers handed
// to the kernels all read it from the region:
//
//   PlantSpan      elements [at, at + n) of a buffer: on(base) is its pointer, or_null(base) null where the call does not have the array
//   PlantCursor    take(n) lays the next region behind the last one (n = 0 takes no room); end() is the buffer's need, and starts over
//   PlantCopier    up(base, region, host) / down(host, base, region) through a copy primitive - hipMemcpyAsync on the plant stream in the
//                  library (plant_workspace.h), memcpy in the host check and for cimpc_plant_tape_lqr's packed upload - folding failures
//                  into the entry's running ok; a region of zero elements or a null host pointer copies nothing
//   the cost       plant_cost_spans takes Q | Qf | R | x_goal | u_goal of a PlantCost, plant_cost_up copies them and returns the cost on
//                  the device's pointers
//   refusals       plant_refuse, plant_first_null, plant_all_finite: what every entry says before it touches a device
//   layouts        of the entries whose staging the host check walks: plant_linesearch_layout, plant_segments_layout
#pragma once
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "../../../include/cimpc.h"
#include "plant_cost.h"
#include "plant_model.h"

namespace cimpc {

void set_global_error(const std::string& msg);      // cimpc_host.cpp: what cimpc_last_error(NULL) returns

// Elements [at, at + n) of a buffer
struct PlantSpan {
    size_t at = 0, n = 0;
    template <class T> T* on(T* base) const { return base + at; }
    template <class T> T* or_null(T* base) const { return n ? base + at : nullptr; }      // an optional array whose kernel takes null
    // elements [from, from + cnt) of the region: a row of it, or the rows written so far
    PlantSpan part(size_t from, size_t cnt) const { assert(from + cnt <= n); return PlantSpan{at + from, cnt}; }
};

// The regions of a buffer follow each other in the order they are taken, without gaps
struct PlantCursor {
    size_t at = 0;
    PlantSpan take(size_t n) { const PlantSpan s{at, n}; at += n; return s; }
    size_t end() { const size_t need = at; at = 0; return need; }
};

// Copy: bool(void* dst, const void* src, size_t bytes, bool to_device).  ok: the entry's running flag; nothing is copied once it is false.
template <class Copy>
struct PlantCopier {
    Copy copy;
    bool& ok;
    template <class T> void up(T* base, const PlantSpan& r, const T* host) { if (r.n && host) ok = ok && copy(base + r.at, host, r.n * sizeof(T), true); }
    template <class T> void down(T* host, const T* base, const PlantSpan& r) { if (r.n && host) ok = ok && copy(host, base + r.at, r.n * sizeof(T), false); }
};
struct PlantHostCopy { bool operator()(void* dst, const void* src, size_t bytes, bool) const { std::memcpy(dst, src, bytes); return true; } };

// ---- the tracking cost ------------------------------------------------------------------------------------------------------------------
struct PlantCostSpans { PlantSpan Q, Qf, R, x_goal, u_goal; };

// Q | Qf | R | x_goal | u_goal of a cost with C's n_Q, n_R, n_x, T, nq, nu; present = false: a call without a cost, which takes no room
inline PlantCostSpans plant_cost_spans(PlantCursor& at, const PlantCost& C, bool present = true) {
    const size_t n = (size_t)2 * C.nq, m = (size_t)C.nu, on = present ? 1 : 0;
    PlantCostSpans s;
    s.Q = at.take(on * C.n_Q * n * n); s.Qf = at.take(on * n * n); s.R = at.take(on * C.n_R * m * m);
    s.x_goal = at.take(on * (size_t)(C.T + 1) * C.n_x * n); s.u_goal = at.take(on * (size_t)C.T * C.n_x * m);
    return s;
}

// C on the pointers of its regions in `base`
inline PlantCost plant_cost_on(PlantCost C, double* base, const PlantCostSpans& s) {
    C.Q = s.Q.on(base); C.Qf = s.Qf.on(base); C.R = s.R.on(base); C.x_goal = s.x_goal.on(base); C.u_goal = s.u_goal.on(base);
    return C;
}

// The five arrays of `host` up into their regions; returns plant_cost_on
template <class Copier>
PlantCost plant_cost_up(Copier& copy, double* base, const PlantCostSpans& s, const PlantCost& host) {
    copy.up(base, s.Q, host.Q); copy.up(base, s.Qf, host.Qf); copy.up(base, s.R, host.R);
    copy.up(base, s.x_goal, host.x_goal); copy.up(base, s.u_goal, host.u_goal);
    return plant_cost_on(host, base, s);
}

// ---- refusals ---------------------------------------------------------------------------------------------------------------------------
inline bool plant_all_finite(const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
    return true;
}

// Leaves "<entry>: <why>" for cimpc_last_error(NULL)
inline int plant_refuse(const char* entry, const std::string& why) {
    set_global_error(std::string(entry) + ": " + why);
    return CIMPC_ERR_INVALID;
}

// The name of the first null pointer among an entry's required arguments, in the order they are listed; null: every one is given
struct PlantRequired { const char* name; const void* ptr; };
template <size_t N>
const char* plant_first_null(const PlantRequired (&required)[N]) {
    for (const PlantRequired& r : required) if (!r.ptr) return r.name;
    return nullptr;
}

// ---- cimpc_plant_tape_linesearch[_box] --------------------------------------------------------------------------------------------------
// w_each, mu_each: w (K_w x B x nw) and mu (B) are per robot and pass through the expansion kernel; limits: n_lim x nu rows each
struct PlantLsShape { int B, T, n_alpha, K_w, n_lim; bool w_each, mu_each, limits; };

struct PlantLsLayout {
    PlantSpan q_nom, u_nom, k, K, w, mu, dV, J_nom, alpha;      // d_in: the B-robot inputs in the order they go up,
    PlantCostSpans cost;                                        //       the cost
    PlantSpan u_lo, u_hi;                                       //       and the limits
    PlantSpan J, q, u_applied, gamma, b, lin_q, lin_r, z;       // d_out: J of the candidates and the chosen rows in the order they come back
    PlantSpan ok, choice, status, iters, conv;                  // d_int
    size_t need_in = 0, need_out = 0, need_int = 0;
};

inline PlantLsLayout plant_linesearch_layout(const PlantModel& M, const PlantCost& C, const PlantLsShape& s) {
    const size_t B = (size_t)s.B, TB = (size_t)s.T * B, NB = (size_t)s.n_alpha * B, nq = M.nq, nu = M.nu, n = 2 * nq, traj = (size_t)(s.T + 2) * B * nq;
    PlantLsLayout L;
    PlantCursor at;
    L.q_nom = at.take(traj); L.u_nom = at.take(TB * nu); L.k = at.take(TB * nu); L.K = at.take(TB * nu * n);
    L.w = at.take(s.w_each ? (size_t)s.K_w * B * M.nw : 0); L.mu = at.take(s.mu_each ? B : 0);
    L.dV = at.take(2 * B); L.J_nom = at.take(B); L.alpha = at.take((size_t)s.n_alpha);
    L.cost = plant_cost_spans(at, C);
    L.u_lo = at.take(s.limits ? (size_t)s.n_lim * nu : 0); L.u_hi = at.take(s.limits ? (size_t)s.n_lim * nu : 0);
    L.need_in = at.end();
    L.J = at.take(NB); L.q = at.take(traj); L.u_applied = at.take(TB * nu); L.gamma = at.take(TB * M.nc); L.b = at.take(TB * M.nb());
    L.lin_q = at.take((size_t)(s.T + 1) * B * n); L.lin_r = at.take(TB * nu); L.z = at.take(TB * M.nz());
    L.need_out = at.end();
    L.ok = at.take(NB); L.choice = at.take(B); L.status = at.take(TB); L.iters = at.take(TB); L.conv = at.take(NB);
    L.need_int = at.end();
    return L;
}

// ---- cimpc_plant_rollout_segments -------------------------------------------------------------------------------------------------------
// segments: M of T / M steps; w as given (K_w x n_w x nw) where has_w; mu (B) where mu_each; cost: the call has one
struct PlantSegmentsShape { int B, T, segments, K_w, n_w; bool has_w, mu_each, cost; };

struct PlantSegmentsLayout {
    PlantSpan nodes, u, w, mu;                                  // d_in: the B-robot inputs in the order they go up,
    PlantCostSpans cost;                                        //       and the cost where there is one
    PlantSpan gamma, b, defects, D, J, lt, lin_q, lin_r;        // d_out: the stitched outputs
    PlantSpan status, iters;                                    // d_int
    size_t need_in = 0, need_out = 0, need_int = 0;
};

inline PlantSegmentsLayout plant_segments_layout(const PlantModel& M, const PlantCost& C, const PlantSegmentsShape& s) {
    const size_t B = (size_t)s.B, TB = (size_t)s.T * B, nq = M.nq, nu = M.nu, n = 2 * nq;
    PlantSegmentsLayout L;
    PlantCursor at;
    L.nodes = at.take((size_t)s.segments * B * n); L.u = at.take(TB * nu);
    L.w = at.take(s.has_w ? (size_t)s.K_w * s.n_w * M.nw : 0); L.mu = at.take(s.mu_each ? B : 0);
    L.cost = plant_cost_spans(at, C, s.cost);
    L.need_in = at.end();
    L.gamma = at.take(TB * M.nc); L.b = at.take(TB * M.nb()); L.defects = at.take((size_t)(s.segments - 1) * B * n); L.D = at.take(B); L.J = at.take(B);
    L.lt = at.take((size_t)(s.T + 1) * B); L.lin_q = at.take((size_t)(s.T + 1) * B * n); L.lin_r = at.take(TB * nu);
    L.need_out = at.end();
    L.status = at.take(TB); L.iters = at.take(TB);
    L.need_int = at.end();
    return L;
}

}  // namespace cimpc
