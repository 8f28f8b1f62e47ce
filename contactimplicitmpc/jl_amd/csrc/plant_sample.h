// The rules of the sampling policy - predictive sampling and the MPPI mean -, stated ONCE for the kernels of
// plant_sample.hip, the entries of the cimpc_plant_sampler handle, the host entry cimpc_plant_sample_noise and a host program
// (tests/native/plant_sample_check.cpp).  Plain C++: no builtins, no inline assembly; the Philox products are (uint64_t)a * b.
//
// RANDOM BITS.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds).  The key is
// (seed & 0xffffffff, seed >> 32) of a 64-bit seed; the counter is (draw, b, c, e): draw = (uint32)(s n_iter + it) with the product formed in
// 64 bits (plant_sample_draw), b the robot, c the sample, e = j nu + i for noise row j and control i.  A robot's noise therefore does not
// depend on B, on N, on the launch geometry or on what rides along, and it is the same every time control step s is asked for.
//
// THE DEVIATE (plant_sample_deviate) is this project's definition, chosen so that device and host agree to the bit: the four output words
// give eight 16-bit fields f_0 .. f_7 (word 0 low half, word 0 high half, word 1 low half, ...);  s = sum_k ((f_k + 0.5) 2^-16 - 0.5), every
// term and every partial sum exact in a double;  eps = s * 0x1.3988e1409212ep+0 (sqrt(1.5) rounded), ONE rounded product.  That is a centred
// Irwin-Hall deviate of order 8: unit variance, excess kurtosis -0.15, support +-4.9.  It is NOT a Gaussian.  No log or cos runs on the device.
//
// THE CANDIDATE LAW.  Candidate c of robot b is rollout robot c B + b, as in the line search (plant_cost.h): it starts from the robot's q[0],
// q[1] and runs open loop on robot b's mu and terrain.  The noise row of step t is j = t / noise_hold: plant_sample_noise_rows(H, noise_hold)
// rows, the last may be partial.  Candidate 0 is a copy of the plan to the bit (nothing is added: -0.0 stays -0.0); for c >= 1
//     u_c[t, b, i] = limit(u_nom[t, b, i] + sigma[i] * eps)      one rounded product, one rounded sum, plant_feedback_limit where limits are given
// (plant_sample_candidate).
//
// ELIGIBILITY AND CHOICE.  A candidate is eligible when its H steps all converged and its J is finite (plant_sample_eligible); choice[b] is
// the eligible candidate of least J, the lower index on a tie, -1 if there is none: plant_linesearch_choice (plant_cost.h).
//
// THE UPDATE (plant_sample_update), temperature lam >= 0.  With choice -1 the plan is kept and every weight is 0.0.  lam == 0, predictive
// sampling: the new plan is the chosen candidate's rows bit for bit; the weights are 1.0 at the choice and 0.0 elsewhere.  lam > 0, the MPPI
// mean:  w_c = eligible ? exp(-((J_c - J_choice) / lam)) : 0.0 (plant_sample_weight);  S = sum of w_c over ascending c from 0.0;
//     u_new[t, b, i] = limit(u_nom + (sum_c w_c * (u_c - u_nom)) / S)      ascending c from 0.0, one rounded difference, product and sum per term
// (plant_sample_mean); the normalised weights w_c / S are an output.  J_nom is candidate 0's J, J_best the choice's (J_nom with choice -1).
//
// THE REFUSALS (plant_sample_refusal), each a reason string, made before a device is touched.  The shared arguments are refused by
// plant_mpc_problem_refusal, _step_refusal, _state_refusal and _plan_refusal; the index rules of the goal window and the warm start are
// plant_mpc.h's.
//
// No contraction in these functions; the pragma stands inside each body, as in plant_cost.h.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "plant_cost.h"
#include "plant_feedback.h"
#include "plant_mpc.h"

#ifdef __HIPCC__
#define PSMP_HD __host__ __device__
#else
#define PSMP_HD
#endif

namespace cimpc {

// Philox4x32-10: out = the ten-round bijection of ctr under key
PSMP_HD inline void plant_sample_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the first counter word of iteration `it` of control step s
PSMP_HD inline uint32_t plant_sample_draw(int s, int n_iter, int it) { return (uint32_t)((uint64_t)s * (uint64_t)n_iter + (uint64_t)it); }

PSMP_HD inline int plant_sample_noise_rows(int H, int noise_hold) { return (int)(((long long)H + noise_hold - 1) / noise_hold); }

// eps of four output words
PSMP_HD inline double plant_sample_deviate(const uint32_t w[4]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int k = 0; k < 8; ++k) {
        const uint32_t f = (k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu);
        s = s + (((double)f + 0.5) * 0x1p-16 - 0.5);
    }
    return s * 0x1.3988e1409212ep+0;
}

// eps of (seed; draw, b, c, e)
PSMP_HD inline double plant_sample_eps(uint64_t seed, uint32_t draw, uint32_t b, uint32_t c, uint32_t e) {
    const uint32_t ctr[4] = {draw, b, c, e}, key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    uint32_t out[4];
    plant_sample_philox(ctr, key, out);
    return plant_sample_deviate(out);
}

// control i of candidate c: lo, hi the robot's limit rows, or both null
PSMP_HD inline double plant_sample_candidate(double u_nom, double sigma, double eps, int c, const double* lo, const double* hi, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (c == 0) return u_nom;
    const double step = sigma * eps;
    const double u = u_nom + step;
    return lo ? plant_feedback_limit(u, lo[i], hi[i]) : u;
}

PSMP_HD inline bool plant_sample_eligible(bool converged, double J) { return converged && std::isfinite(J); }

PSMP_HD inline double plant_sample_weight(bool eligible, double J, double J_choice, double lam) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return eligible ? std::exp(-((J - J_choice) / lam)) : 0.0;
}

// One entry of the MPPI mean: candidate c's entry at cand[c * stride], its unnormalised weight at w[c * w_stride]
PSMP_HD inline double plant_sample_mean(double u_nom, const double* cand, size_t stride, const double* w, size_t w_stride, int N, double S, const double* lo,
                                        const double* hi, int i) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double acc = 0.0;
    for (int c = 0; c < N; ++c) {
        const double d = cand[c * stride] - u_nom;
        const double p = w[c * w_stride] * d;
        acc = acc + p;
    }
    const double shift = acc / S;
    const double u = u_nom + shift;
    return lo ? plant_feedback_limit(u, lo[i], hi[i]) : u;
}

// One iteration's update, every pointer in the memory the team reads.  In: J and conv of the N B candidates (c B + b), their controls cand
// H x (N B) x nu, the limits (n_lim x nu, or both null).  In and out: the plan u_plan H x B x nu, updated in place.  Scratch: ok, w_raw (N B).
// Out: weights (N B, normalised), and robot b's entries of J_nom, J_best, choice, n_eligible (B each).
struct PlantSampleUpdate {
    const double* J;
    const int* conv;
    const double* cand;
    double* u_plan;
    const double *u_lo, *u_hi;
    int n_lim;
    int* ok;
    double *w_raw, *weights;
    double *J_nom, *J_best;
    int *choice, *n_eligible;
    int B, N, H, nu;
    double lam;
};

// Robot b's update by a team (rank, size, sync as in plant_cost.h); every member gets the choice, and the team is synchronized on return.
// Every output element is one ordered chain, so the result does not depend on the team.
template <class Team>
PSMP_HD inline int plant_sample_update(const PlantSampleUpdate& P, int b, Team& team) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const int B = P.B, N = P.N, nu = P.nu, rank = team.rank(), size = team.size();
    const size_t NB = (size_t)N * B;
    for (int c = rank; c < N; c += size) P.ok[(size_t)c * B + b] = plant_sample_eligible(P.conv[(size_t)c * B + b] != 0, P.J[(size_t)c * B + b]) ? 1 : 0;
    team.sync();
    const int choice = plant_linesearch_choice(P.J + b, (size_t)B, P.ok + b, (size_t)B, N);
    const double J_choice = choice < 0 ? 0.0 : P.J[(size_t)choice * B + b];
    for (int c = rank; c < N; c += size) {
        const size_t at = (size_t)c * B + b;
        P.w_raw[at] = choice < 0 ? 0.0 : P.lam == 0.0 ? (c == choice ? 1.0 : 0.0) : plant_sample_weight(P.ok[at] != 0, P.J[at], J_choice, P.lam);
    }
    team.sync();
    double S = 0.0;
    int n_eligible = 0;
    for (int c = 0; c < N; ++c) {
        S = S + P.w_raw[(size_t)c * B + b];
        n_eligible += P.ok[(size_t)c * B + b];
    }
    for (int c = rank; c < N; c += size) P.weights[(size_t)c * B + b] = choice < 0 ? 0.0 : P.w_raw[(size_t)c * B + b] / S;
    if (rank == 0) {
        P.choice[b] = choice;
        P.n_eligible[b] = n_eligible;
        P.J_nom[b] = P.J[b];
        P.J_best[b] = choice < 0 ? P.J[b] : J_choice;
    }
    if (choice >= 0) {
        const double *lo = P.u_lo ? plant_feedback_limits(P.u_lo, P.n_lim, b, nu) : nullptr, *hi = P.u_lo ? plant_feedback_limits(P.u_hi, P.n_lim, b, nu) : nullptr;
        const long long n = (long long)P.H * nu;
        for (long long e = rank; e < n; e += size) {
            const int t = (int)(e / nu), i = (int)(e % nu);
            const size_t to = ((size_t)t * B + b) * nu + i, from = ((size_t)t * NB + b) * nu + i;      // candidate 0's entry; candidate c's lies c B nu further
            if (P.lam == 0.0) P.u_plan[to] = P.cand[from + (size_t)choice * B * nu];
            else P.u_plan[to] = plant_sample_mean(P.u_plan[to], P.cand + from, (size_t)B * nu, P.w_raw + b, (size_t)B, N, S, lo, hi, i);
        }
    }
    team.sync();
    return choice;
}

// sigma: nu entries
inline const char* plant_sample_refusal(int N, int B, int H, int nu, const double* sigma, int noise_hold, double lam, int n_iter) {
    if (N < 1) return "N below 1";
    if (!plant_linesearch_fits(N, B, H)) return "N B H beyond an int";
    if (!sigma) return "null sigma";
    for (int i = 0; i < nu; ++i)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return "a sigma entry that is negative or not finite";
    if (noise_hold < 1) return "noise_hold below 1";
    if (!(lam >= 0.0)) return "lam negative or not a number";
    if (n_iter < 1) return "n_iter below 1";
    return nullptr;
}

}  // namespace cimpc
