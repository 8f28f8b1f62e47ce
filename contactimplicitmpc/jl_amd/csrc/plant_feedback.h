// Linear state feedback inside a device rollout (DESIGN.md sections 3, item 3c, and 5.5): u = ubar + K (x_ref - x), stated ONCE for
// the step kernel (plant_kernel.hip), the reverse chain (plant_adjoint.h) and a host program (tests/native/plant_feedback_check.cpp).
//
// A feedback schedule has K_f rows, every row held for hold_f steps and the last from there on (rollout_row): K, K_f x n_f x
// (nu x 2nq), each block COLUMN-major - one knot of cimpc_reference_gains' output -, and x_ref, K_f x n_f x 2nq; n_f = 1 (one schedule
// for every robot) or B.  Step t of a robot, row k = rollout_row(t, hold_f, K_f), q0 = q[t], q1 = q[t + 1], ubar_t the open-loop row:
//
//   x[j]   = j < nq ? q1[j] - n_sample (q1[j] - q0[j]) : q1[j - nq]      the expression of gains.hip's feedback kernel, also for n_sample = 1
//   e[j]   = x_ref[k][j] - x[j]                                          j = 0 .. 2nq-1
//   s[i]   = sum_j K[k][i, j] e[j]                                       ascending j from 0.0, one rounded product and one rounded sum per term
//   u_t[i] = ubar_t[i] + s[i]
//
// Nothing is divided by N_sample here: the host passes K / N_sample beside u / N_sample.  The reverse statements, after v = D_t' a of
// step t, with gu = v[2nq : 2nq+nu]:
//
//   gx[j] = sum_i K[k][i, j] gu[i]                                       ascending i from 0.0
//   lambda[t][i]   = lambda[t][i] - n_sample gx[i]                       i < nq
//   lambda[t+1][i] = (lambda[t+1][i] - (1 - n_sample) gx[i]) - gx[nq + i]
//
// No contraction in these functions (a * b + c rounds twice).  The pragma stands inside each body, not at file scope: the step kernel
// includes this header and must keep contracting everywhere else.
#pragma once
#include <cstddef>

#include "plant_rollout_plan.h"

#ifdef __HIPCC__
#define PFB_HD __host__ __device__
#else
#define PFB_HD
#endif

namespace cimpc {

// A feedback schedule in the memory its reader reads (device memory for the kernels).  K == nullptr: open loop.
// The struct does not grow with the clamp's derivative: the mask of clamped controls that the two chains
// read is appended to PlantAdjoint and PlantTangent instead.  This struct also lies in the arguments of the step kernel, whose
// instantiations a word more in it would compile differently (see PlantFeedbackLimits below), and the step kernel has no use for the mask.
struct PlantFeedback {
    const double* K = nullptr;      // K_f x n_f x (nu x 2nq), blocks column-major
    const double* x_ref = nullptr;  // K_f x n_f x 2nq
    int K_f = 1, n_f = 1, hold_f = 1;
    double n_sample = 1.0;
};

// The limits of the limited law: u_t[i] = plant_feedback_limit(ubar_t[i] + s[i], u_lo[i], u_hi[i]) with
// n_lim x nu limits, n_lim = 1 (one row for every robot) or B; u_applied stores the limited value, fb_err is unchanged.  u_lo == nullptr:
// no limits.  Kept beside PlantFeedback, not inside it: that struct lies in the arguments of the step, adjoint and tangent kernels, and
// three more words in it changed the register allocation of the six closed-loop step instantiations.
struct PlantFeedbackLimits {
    const double *u_lo = nullptr, *u_hi = nullptr;      // n_lim x nu each, or both null
    int n_lim = 1;
};

// the K block and the x_ref row step t of robot rb reads
PFB_HD inline const double* plant_feedback_gain(const PlantFeedback& F, int t, int rb, int nu, int nq) {
    return rollout_schedule(F.K, t, F.hold_f, F.K_f, F.n_f, rb, nu * 2 * nq);
}
PFB_HD inline const double* plant_feedback_target(const PlantFeedback& F, int t, int rb, int nq) {
    return rollout_schedule(F.x_ref, t, F.hold_f, F.K_f, F.n_f, rb, 2 * nq);
}

// e[j] of the law: q0, q1 the step's two trajectory rows, target its x_ref row
PFB_HD inline double plant_feedback_error(const double* target, const double* q0, const double* q1, int nq, double n_sample, int j) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double x = j < nq ? q1[j] - n_sample * (q1[j] - q0[j]) : q1[j - nq];
    return target[j] - x;
}

// u_t[i] of the law: Kk the step's block, e its 2nq errors, ubar the open-loop control i
PFB_HD inline double plant_feedback_control(const double* Kk, const double* e, int nu, int nq, int i, double ubar) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int j = 0; j < 2 * nq; ++j) s = s + Kk[(size_t)j * nu + i] * e[j];
    return ubar + s;
}

// The limiter of a control with limits, stated once: lo where u < lo, hi where u > hi, u otherwise.  A
// NaN u passes through (both comparisons are false); -inf and +inf bounds never bind; lo == hi gives that value.
PFB_HD inline double plant_feedback_limit(double u, double lo, double hi) { return u < lo ? lo : (u > hi ? hi : u); }

// robot rb's row of a limit array
PFB_HD inline const double* plant_feedback_limits(const double* lim, int n_lim, int rb, int nu) { return lim + (size_t)(n_lim == 1 ? 0 : rb) * nu; }

// The derivative of the limited law, stated once.  Control i of step t is FREE when its APPLIED value
// u = u_applied[t, b, i] lies strictly inside its limits, and CLAMPED otherwise: on a bound, whether the limiter moved it there or the law
// landed there; with lo == hi; and when u is NaN (every comparison is false; such a step fails and is cut anyway).  Infinite bounds never
// clamp.  The limited law's derivative is the unlimited law's where the control is free and exactly 0.0 where it is clamped: an element of
// the generalized derivative everywhere, the classical derivative off the bounds.
PFB_HD inline bool plant_feedback_free(double u, double lo, double hi) { return (lo < u) && (u < hi); }

// The mask word of one (step, robot): bit i set where control i is clamped; u the nu applied controls, lo and hi the robot's limit rows.
// nu <= 12 (PLANT_MAX_U), so an int holds it.
PFB_HD inline int plant_feedback_clamped(const double* u, const double* lo, const double* hi, int nu) {
    int word = 0;
    for (int i = 0; i < nu; ++i) if (!plant_feedback_free(u[i], lo[i], hi[i])) word |= 1 << i;
    return word;
}
// whether control i is free by a mask word
PFB_HD inline bool plant_feedback_word_free(int word, int i) { return ((word >> i) & 1) == 0; }

// gx[j] of the reverse statements: gu the step's nu control cotangents
PFB_HD inline double plant_feedback_pull(const double* Kk, const double* gu, int nu, int j) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int i = 0; i < nu; ++i) s = s + Kk[(size_t)j * nu + i] * gu[i];
    return s;
}

// lambda[t][i] and lambda[t+1][i] after the feedback path of step t (i < nq)
PFB_HD inline double plant_feedback_lambda0(double l0, const double* gx, double n_sample, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return l0 - n_sample * gx[i];
}
PFB_HD inline double plant_feedback_lambda1(double l1, const double* gx, double n_sample, int nq, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return (l1 - (1.0 - n_sample) * gx[i]) - gx[nq + i];
}

}  // namespace cimpc
