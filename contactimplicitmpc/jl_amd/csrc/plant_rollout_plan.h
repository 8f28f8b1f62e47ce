// How an open-loop rollout of the device plant is cut into launches and which schedule row a step reads, in one place (plain C++, host
// and device: tests/native/plant_rollout_plan_check.cpp builds it with g++).  A rollout of T simulator steps runs as chained launches of
// at most `steps_per_launch` steps on one stream; the trajectory buffer carries the state from one launch to the next.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define ROLLOUT_HD __host__ __device__
#else
#define ROLLOUT_HD
#endif

namespace cimpc {

// Steps per launch when the caller passes 0.  With the kernel times of DESIGN.md section 5.5 (0.72 ms per hopper step at B = 512, 5.4 ms
// for the box and 9.15 ms for the wall at B = 256) a launch stays under about 0.6 s.
constexpr int PLANT_ROLLOUT_STEPS_PER_LAUNCH = 64;

// Row of a K-row schedule that simulator step t (0-based) reads: every row is held for `hold` steps (the reference's N_sample:
// open_loop_policy, src/simulator/policy.jl:4-34; open_loop_disturbances, disturbances.jl:4-36), the last one from there on.
ROLLOUT_HD constexpr int rollout_row(int t, int hold, int K) { return t / hold < K - 1 ? t / hold : K - 1; }

// What robot rb reads at step t from a schedule s of K x n x width doubles (n = 1: one schedule for every robot, else one per robot):
// the u1 or the w1 of the step, as the step kernel and the sensitivity kernel put them into theta.
ROLLOUT_HD constexpr const double* rollout_schedule(const double* s, int t, int hold, int K, int n, int rb, int width) {
    return s + ((size_t)rollout_row(t, hold, K) * n + (n == 1 ? 0 : rb)) * width;
}

// Launch k of a rollout runs steps t0 .. t0 + n - 1.
struct RolloutChunk { int t0, n; };
ROLLOUT_HD constexpr int rollout_chunk_steps(int steps_per_launch) { return steps_per_launch > 0 ? steps_per_launch : PLANT_ROLLOUT_STEPS_PER_LAUNCH; }
ROLLOUT_HD constexpr int rollout_chunk_count(int T, int steps_per_launch) { return T <= 0 ? 0 : (T - 1) / rollout_chunk_steps(steps_per_launch) + 1; }
ROLLOUT_HD constexpr RolloutChunk rollout_chunk(int T, int steps_per_launch, int k) {
    const int c = rollout_chunk_steps(steps_per_launch);
    const long long t0 = (long long)k * c;
    return {(int)t0, (int)(T - t0 < c ? T - t0 : c)};
}

static_assert(rollout_row(0, 3, 4) == 0 && rollout_row(2, 3, 4) == 0 && rollout_row(3, 3, 4) == 1 && rollout_row(11, 3, 4) == 3 && rollout_row(100, 3, 4) == 3,
              "a row is held for `hold` steps, the last one for good");
static_assert(rollout_chunk_count(65, 0) == 2 && rollout_chunk(65, 0, 1).t0 == 64 && rollout_chunk(65, 0, 1).n == 1, "65 steps: 64 + 1");

}  // namespace cimpc
