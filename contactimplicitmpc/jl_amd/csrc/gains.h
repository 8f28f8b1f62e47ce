// Time-varying LQR feedback gains along the reference (gains.hip) for callers inside the library: the handle's policy calls of
// cimpc_host.cpp (cimpc_set_gains, cimpc_gain_latch, cimpc_gain_feedback) launch the two policy kernels through these, and the
// stateless entries of gains.hip leave their message where cimpc_last_error(NULL) finds it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace cimpc {

// Sizes the Riccati kernel serves: n = 2 nq states, m = nu controls (model_table.h needs 36 and 12)
constexpr int GAINS_MAX_N = 48;
constexpr int GAINS_MAX_M = 16;

// What cimpc_gain_latch keeps per rollout, in this order: u1 (nu) | K[window[1]] (nu x 2nq, column-major) | target = [q_ref[1]; q_ref[2]] (2nq)
inline size_t gain_latch_doubles(int nq, int nu) { return (size_t)nu + (size_t)nu * 2 * nq + 2 * (size_t)nq; }

// One workgroup per rollout: latch[b] = (traj_u[b][0], K[window[b][0]], ref_q[b][0..1]).  window: B x (H + 2) 0-based knots; traj_u: B x H x nu;
// ref_q: B x (H + 2) x nq; K: H_ref x (nu x 2nq).  No synchronization.  False: a failed launch.
bool gain_latch_launch(int B, int H, int nq, int nu, const int* window, const double* traj_u, const double* ref_q, const double* K,
                       double* latch, hipStream_t st);

// One workgroup per rollout: u[b] = (u1 + K ([q_ref1; q_ref2] - [q_cur - n_sample (q_cur - q_prev); q_cur])) / n_sample from latch[b].
// q_prev, q_cur: B x nq; u: B x nu; all device memory.  No synchronization.  False: a failed launch.
bool gain_feedback_launch(int B, int nq, int nu, const double* latch, const double* q_prev, const double* q_cur, double n_sample, double* u,
                          hipStream_t st);

// The message of a call without a handle (cimpc_last_error(NULL)); defined in cimpc_host.cpp
void set_global_error(const std::string& msg);

}  // namespace cimpc
