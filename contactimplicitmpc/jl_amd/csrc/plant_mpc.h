// The rules of the receding-horizon iLQR policy, stated ONCE for the kernels of plant_mpc.hip, the entries
// of the cimpc_plant_mpc handle and a host program (tests/native/plant_mpc_check.cpp).  Integers and copies only: nothing here does
// floating-point arithmetic, so the device's rows are the host's bit for bit.
//
// THE GOAL WINDOW.  The reference has L stages: x_ref (L + 1) x n_x x 2nq and u_ref L x n_x x nu, n_x 1 or B.  The cost of control step s
// over a horizon of H stages reads
//     x goal of stage t (0 .. H):      row min(s + t, L)          (plant_mpc_x_row)
//     u goal of stage t (0 .. H - 1):  row min(s + t, L - 1)      (plant_mpc_u_row)
// so the last goal is held.  Q, R and Qf are indexed by stage, not by time: they are not shifted.
//
// THE WARM START.  The plan advanced by shift >= 0 control steps:  u_warm[t] = u_plan[min(t + shift, H - 1)]  (plant_mpc_warm_row): the last
// row repeats, shift = 0 leaves the plan as it is, and a plan inside the box stays inside it - nothing is clipped again.
//
// THE START ROWS.  q[0] = q0 and q[1] = q1 as uploaded; the host forms q0 = q1 - h v1 as `rollout` does.
//
// THE PER-STEP RESET.  Every robot starts every control step at level 0 of the ladder and active (plant_mpc_reset_robot); the ladder is the
// one uploaded at creation (plant_ilqr.h).
//
// THE REFUSALS, each a reason string, made before any device is touched: plant_mpc_problem_refusal (creation), plant_mpc_step_refusal and
// plant_mpc_state_refusal (a control step), plant_mpc_plan_refusal (a plan that is loaded); the loop's own are plant_ilqr_refusal's.
#pragma once
#include <cmath>
#include <cstddef>

#include "plant_ilqr.h"

#ifdef __HIPCC__
#define PMPC_HD __host__ __device__
#else
#define PMPC_HD
#endif

namespace cimpc {

PMPC_HD inline int plant_mpc_x_row(int s, int t, int L) {
    const long long r = (long long)s + t;
    return r < L ? (int)r : L;
}

PMPC_HD inline int plant_mpc_u_row(int s, int t, int L) {
    const long long r = (long long)s + t;
    return r < L - 1 ? (int)r : L - 1;
}

PMPC_HD inline int plant_mpc_warm_row(int t, int shift, int H) {
    const long long r = (long long)t + shift;
    return r < H - 1 ? (int)r : H - 1;
}

// n doubles from src to dst by member `rank` of a team of `size`
PMPC_HD inline void plant_mpc_copy(double* dst, const double* src, int n, int rank, int size) {
    for (int i = rank; i < n; i += size) dst[i] = src[i];
}

PMPC_HD inline void plant_mpc_reset_robot(int* level, int* active) {
    *level = 0;
    *active = 1;
}

// Row t (0 .. H - 1) of robot b of the warm start: u_plan and u_warm H x B x nu
PMPC_HD inline void plant_mpc_warm_start(double* u_warm, const double* u_plan, int t, int b, int shift, int H, int B, int nu, int rank, int size) {
    plant_mpc_copy(u_warm + ((size_t)t * B + b) * nu, u_plan + ((size_t)plant_mpc_warm_row(t, shift, H) * B + b) * nu, nu, rank, size);
}

// Row t (0 .. H) of goal column g (0 .. n_x - 1) of control step s: x_goal (H + 1) x n_x x n and, for t < H, u_goal H x n_x x m
PMPC_HD inline void plant_mpc_window(double* x_goal, double* u_goal, const double* x_ref, const double* u_ref, int s, int t, int g, int H, int L, int n_x,
                                     int n, int m, int rank, int size) {
    plant_mpc_copy(x_goal + ((size_t)t * n_x + g) * n, x_ref + ((size_t)plant_mpc_x_row(s, t, L) * n_x + g) * n, n, rank, size);
    if (t < H) plant_mpc_copy(u_goal + ((size_t)t * n_x + g) * m, u_ref + ((size_t)plant_mpc_u_row(s, t, L) * n_x + g) * m, m, rank, size);
}

inline const char* plant_mpc_problem_refusal(int H, int L, int n_iter) {
    if (H < 1 || L < 1) return "H or L below 1";
    if (n_iter < 1) return "n_iter below 1";
    return nullptr;
}

inline const char* plant_mpc_step_refusal(int s, int shift, bool has_plan) {
    if (shift < 0 || s < 0) return "shift or s negative";
    if (!has_plan) return "a shift with no plan loaded";
    return nullptr;
}

inline bool plant_mpc_finite(const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// q0, q1: n = B nq entries each
inline const char* plant_mpc_state_refusal(const double* q0, const double* q1, size_t n) {
    if (!plant_mpc_finite(q0, n)) return "a non-finite entry of q0";
    if (!plant_mpc_finite(q1, n)) return "a non-finite entry of q1";
    return nullptr;
}

// u0 H x B x nu; with limits (n_lim x nu rows, n_lim 1 or B; both null: none) every entry lies in its box
inline const char* plant_mpc_plan_refusal(const double* u0, int H, int B, int nu, const double* u_lo, const double* u_hi, int n_lim) {
    const size_t n = (size_t)H * B * nu;
    if (!plant_mpc_finite(u0, n)) return "a non-finite entry of u0";
    if (u_lo && u_hi)
        for (size_t e = 0; e < n; ++e) {
            const size_t i = e % nu, b = (e / nu) % B, row = (n_lim == 1 ? 0 : b) * nu + i;
            if (u0[e] < u_lo[row] || u0[e] > u_hi[row]) return "an entry of u0 outside the limits";
        }
    return nullptr;
}

}  // namespace cimpc
