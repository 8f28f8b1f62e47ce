// What a solver handle knows about its window, its reference and its gain latch, stated once: the flags, the questions the entry
// points ask of them, the transitions the entry points make, the one order in which the window moves, the check of a caller's
// window and the sizes of the horizon arrays.  Plain C++17, no HIP: cimpc_host.cpp holds one HandleState and goes through these
// names only; tests/native/handle_state_check.cpp runs every failure point on the CPU (DESIGN.md section 5.4b has the table).
#pragma once

#include <cstddef>
#include <vector>

#include "../../../include/cimpc.h"

namespace cimpc {

struct Refusal {       // code CIMPC_OK: not refused (msg is null)
    int code;
    const char* msg;
};

// who wrote the per-step sensitivity memory last
enum : int { DZ_NOBODY = 0, DZ_NEWTON = 1 /* newton_solve: dz_good */, DZ_IMPLICIT = 2 /* implicit_dynamics: slot 0 of dz */ };

struct HandleState {
    bool objective_set = false, window_set = false, reference_set = false, alt_set = false;
    bool gait_set = false;            // window and reference are generated on the device from the resident gait (cimpc_set_gait)
    bool gains_set = false, gains_latched = false;
    bool latch_ready = false;         // a Newton solve has run and nothing has moved the window or the reference since
    bool advance_pending = false;     // a cimpc_mpc_advance is queued on the handle's stream and not waited for
    int dz_producer = DZ_NOBODY;
    std::vector<int> win_mirror;      // 0-based window as the HOST last uploaded it; empty: unknown (moved on the device, or a move failed).
                                      // Not empty implies window_set and not gait_set: window_move is the only writer

    // ---- questions ---------------------------------------------------------------------------------------------------------
    Refusal solve_refusal(bool every_knot_set, bool need_newton) const {      // check_ready
        if (!every_knot_set) return {CIMPC_ERR_STATE, "set_linearization has not been called for every knot"};
        if (!window_set) return {CIMPC_ERR_STATE, "set_window has not been called"};
        if (need_newton && !objective_set) return {CIMPC_ERR_STATE, "set_objective has not been called"};
        if (need_newton && !reference_set) return {CIMPC_ERR_STATE, "set_reference has not been called"};
        return {CIMPC_OK, nullptr};
    }
    Refusal advance_refusal() const {
        if (!window_set || !reference_set) return {CIMPC_ERR_STATE, "set_window / set_reference have not been called"};
        return {CIMPC_OK, nullptr};
    }
    Refusal latch_refusal() const {
        if (!gains_set) return {CIMPC_ERR_STATE, "cimpc_set_gains has not been called"};
        if (!latch_ready)
            return {CIMPC_ERR_STATE, "cimpc_gain_latch belongs between a newton solve and cimpc_mpc_advance: no solve has run, or the window or the reference moved since"};
        return {CIMPC_OK, nullptr};
    }
    Refusal feedback_refusal() const {
        if (!gains_set || !gains_latched) return {CIMPC_ERR_STATE, "cimpc_gain_latch has not been called since cimpc_set_gains"};
        return {CIMPC_OK, nullptr};
    }
    bool drain_needed() const { return advance_pending; }
    bool has_altitude() const { return alt_set; }
    bool advances_by_gait() const { return gait_set; }
    // the sensitivity memory follows the reference knots around a window move: archive with the old window, restore with the new one
    bool rekey_out_needed() const { return dz_producer != DZ_NOBODY && window_set; }
    int rekey_out_store() const { return dz_producer == DZ_NEWTON ? 0 : 1; }      // the store that holds the live blocks: 0 dz_good, 1 slot 0
    bool rekey_in_needed(bool archive_exists) const { return dz_producer != DZ_NOBODY && archive_exists; }
    bool dz_sync_needed(int next_producer) const { return dz_producer != DZ_NOBODY && dz_producer != next_producer; }
    bool mirror_equals(const int* w0, size_t n) const {
        if (win_mirror.size() != n) return false;
        for (size_t k = 0; k < n; ++k)
            if (win_mirror[k] != w0[k]) return false;
        return true;
    }

    // ---- transitions (the window's are window_move's) ---------------------------------------------------------------------------
    void objective_replaced() { objective_set = true; }
    void objective_refused() { objective_set = false; }      // a refused objective leaves NO objective
    void altitude_set() { alt_set = true; }
    void altitude_cleared() { alt_set = false; }
    void unlatch() { latch_ready = false; }                  // the window or the reference is about to move
    void reference_replaced() { reference_set = true; gait_set = false; }      // an explicit reference replaces the gait-generated one
    void gait_installed() { gait_set = reference_set = true; }                 // (behind a window_move with WindowHome::Device)
    void advance_queued() { advance_pending = true; }
    void advance_drained() { advance_pending = false; }
    void solve_started() { dz_producer = DZ_NEWTON; latch_ready = true; }
    void implicit_dynamics_started() { dz_producer = DZ_IMPLICIT; }
    void gains_changing() { gains_latched = false; }
    void gains_replaced() { gains_set = true; }
    void gains_cleared() { gains_set = false; }
    void latched() { gains_latched = true; }
};

enum class WindowHome { Host, Device };      // who wrote the new window: the host (it keeps a mirror) or a kernel

// The only place the order of a window move is written.  out() archives the sensitivity memory under the window still in force,
// change() rewrites the device window, in() restores under the new one; each returns a CIMPC_* code.  From the first step on the
// mirror is unknown and no latch may run; the move is committed only when all three succeeded, and a failure's code comes back as
// it is, with the state left at "mirror unknown, no latch" (window_set, reference_set and gait_set as they were).
template <class Out, class Change, class In>
int window_move(HandleState& s, WindowHome home, const int* w0, size_t n, Out&& out, Change&& change, In&& in) {
    s.latch_ready = false;
    s.win_mirror.clear();
    if (int rc = out(); rc != CIMPC_OK) return rc;
    if (int rc = change(); rc != CIMPC_OK) return rc;
    if (int rc = in(); rc != CIMPC_OK) return rc;
    s.window_set = true;
    if (home == WindowHome::Host) {
        s.win_mirror.assign(w0, w0 + n);
        s.gait_set = false;               // an explicit window replaces the gait-generated one
    }
    return CIMPC_OK;
}

// A caller's window (1-based knots, 1 .. K) as the device buckets it (0-based); refused at the first entry out of range
inline Refusal window_to_knots(const int* window, size_t n, int K, int* out) {
    for (size_t k = 0; k < n; ++k) {
        const int t = window[k];
        if (t < 1 || t > K) return {CIMPC_ERR_INVALID, "window entry out of range (1-based knot index)"};
        out[k] = t - 1;
    }
    return {CIMPC_OK, nullptr};
}

// Elements of the horizon arrays of all B rollouts: window, q, u, w, gamma, b, theta, the duals nu, the altitudes
struct HorizonSizes {
    size_t win, q, u, w, g, b, th, nu, alt;
};
inline HorizonSizes horizon_sizes(const cimpc_dims& d, int nth, int nd) {
    const size_t B = d.B, H = d.H;
    return {B * (H + 2), B * (H + 2) * d.nq, B * H * d.nu, B * H * d.nw, B * H * d.nc, B * H * d.nb, B * H * nth, B * H * nd, B * d.nc};
}
inline HorizonSizes horizon_rows(cimpc_dims d, int nth, int nd) {      // ... of one rollout
    d.B = 1;
    return horizon_sizes(d, nth, nd);
}

}  // namespace cimpc
