// The words the host and the kernels exchange during a solve, in one place (plain C++, no HIP header:
// tests/native/round_protocol_check.cpp builds it with g++).  Names and layout arithmetic only - which kernel runs, and when, is
// decided in kkt_plan.h and schedule_plan.h.  Every value here is part of the protocol between cimpc_host.cpp and the kernels
// (newton_impl.h, newton_async_impl.h, newton_kernels.hip, kkt_dense.hip): a change is a change of both sides.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define ROUND_HD __host__ __device__ __forceinline__
#else
#define ROUND_HD inline
#endif

namespace cimpc {

constexpr int QPAD = 32;   // ints between two queue counters
constexpr int CPAD = 32;   // ints between two ROUND counters: every counter on its own 128-byte line - same-line atomics serialise
                           // in the L2 at ~50 ns each, and the decision kernel issues several per workgroup

// ---- Round counters (NewtonDev::counters / counters_next): one block per round parity, zeroed for the next round by the
// residual kernel of the running one.
enum RoundCounter : int {
    RC_SWEEP = 0,       // rollouts that need a sweep in the next round
    RC_KKT = 1,         // rollouts that entered STAGE_KKT (length of kkt_list)
    RC_PARKED = 2,      // interior-point solves the sweep parked (IpParams::pending_count)
    RC_DRAINED = 3,     // workgroups of the sweep that ran out of work (IpParams::drain_count)
    RC_SLOTS = 4,       // evaluation slots requested of the next round (length of slot_list)
    RC_NEW_SLOTS = 5,   // ... of which newly requested: slots re-listed while a solve is parked are not in it (a deterministic count)
    RC_TICKET = 7,      // decision blocks that have finished: the last one publishes the round
};
constexpr int ROUND_COUNTERS = 8;                          // counters per block (6 is unused)
constexpr int ROUND_COUNTER_INTS = ROUND_COUNTERS * CPAD;
ROUND_HD constexpr int* round_counter(int* block, int k) { return block + k * CPAD; }
// the two blocks follow each other (d_ring of the host): round r counts in block r & 1
ROUND_HD constexpr int* round_counter_block(int* blocks, int parity) { return blocks + ROUND_COUNTER_INTS * parity; }

// ---- Host ring: host-mapped pinned memory, one slot per round parity.  The last decision block of a round stores the counts
// and then the stamp (NewtonDev::round_stamp = round + 1); the host spins on the stamp.
enum RingWord : int {
    RING_N_SWEEP = 0,
    RING_N_KKT = 1,
    RING_STAMP = 2,
    RING_ABORT = 3,     // of slot 0 only: abort flag of the persistent kernel, host -> device.  The decision kernel never writes
                        // word 3 of a slot, which is why the flag can live in the ring.
    RING_PARKED = 4,
    RING_FINISHED = 5,  // rollouts whose solve has ended (hybrid schedule; else 0)
    RING_SLOTS = 6,
    RING_NEW_SLOTS = 7,
};
constexpr int RING_SLOT_INTS = 8, RING_SLOTS_COUNT = 2, RING_ALLOC_INTS = 32;
// the words the decision kernel publishes, in the order of its stores (the stamp last)
constexpr RingWord RING_PUBLISHED[] = {RING_N_SWEEP, RING_N_KKT, RING_PARKED, RING_SLOTS, RING_NEW_SLOTS, RING_FINISHED, RING_STAMP};
template <class T> ROUND_HD constexpr T* ring_slot(T* ring, long long round) { return ring + RING_SLOT_INTS * (round & 1); }
template <class T> ROUND_HD constexpr T* ring_abort_word(T* ring) { return ring + RING_ABORT; }

// ---- Queue control block of the lock-step rounds: queue counters, queue heads and the two round-counter blocks in ONE
// allocation, cleared by one memset at the start of a solve.
struct QueueCtl { size_t count, head, counters, ints; };      // offsets of count[2][K], head[K], the counter blocks; total
constexpr QueueCtl queue_ctl(size_t K) { return {0, 2 * K * QPAD, 3 * K * QPAD, 3 * K * QPAD + 2 * (size_t)ROUND_COUNTER_INTS}; }

// ---- Control block of the persistent solve: its own queue counters and heads (one parity), the job words of AsyncQ and the
// wake-up words.
constexpr int EPOCH_STRIDE = 16, EPOCH_BUCKETS = 16, EPOCH_WORDS = 2 * EPOCH_BUCKETS + 1;
constexpr int ASYNC_JOB_INTS = 64;      // the job words: what a hybrid solve clears again before its rounds (no epoch word)
struct AsyncCtl { size_t count, head, jobs, rq_head, n_done, rq_tail, kq_head, kq_tail, epoch, ints; };
constexpr AsyncCtl async_ctl(size_t K) {
    const size_t j = 2 * K * QPAD;      // (the counters keep the room of two parities)
    return {0, K * QPAD, j, j + 0, j + 8, j + 16, j + 32, j + 48, j + ASYNC_JOB_INTS, j + ASYNC_JOB_INTS + EPOCH_WORDS * EPOCH_STRIDE};
}
// Wake-up words (offsets from AsyncQ::epoch), 64 B apart: one per bucket for interior-point work, one per bucket for jobs, one
// for any job.  bucket = rollout % 16 for a producer, blockIdx % 16 for an idle workgroup, which polls only its own two words.
ROUND_HD constexpr int epoch_bucket(int i) { return i & (EPOCH_BUCKETS - 1); }
ROUND_HD constexpr int epoch_ip(int bucket) { return bucket * EPOCH_STRIDE; }
ROUND_HD constexpr int epoch_job(int bucket) { return (EPOCH_BUCKETS + bucket) * EPOCH_STRIDE; }
ROUND_HD constexpr int epoch_any_job() { return 2 * EPOCH_BUCKETS * EPOCH_STRIDE; }

// KKT job words of the persistent solve: rollout index in the low 24 bits, kind above
constexpr int KJOB_SHIFT = 24, KJOB_MASK = (1 << KJOB_SHIFT) - 1;
enum KktJobKind : int {
    KJOB_ONE_ENDED = 0,
    KJOB_TOP = 1,       // top chain of the twisted solve
    KJOB_BOTTOM = 2,    // bottom chain
    KJOB_RETRY = 3,     // one-ended recursion of a rollout whose twisted hand-over timed out
};

// ---- Twisted hand-over: per rollout one line of flags (NewtonDev::kkt_tw_flags) and one exchange block (kkt_tw_xch).  The flags
// are epoch-valued: a producer stores the launch's stamp, a consumer waits for equality, nothing is reset.
enum TwFlag : int {
    TW_TRACES = 0,      // traces ready
    TW_MIDDLE = 1,      // middle dnu (banded: middle x) ready
    TW_FINISHED = 2,    // chains finished (a counter; the last chain zeroes it)
    TW_TIMED_OUT = 3,   // a hand-over of this launch timed out: poisoned numbers
};
constexpr int KKT_BAND_TW_FLAG0 = 4;      // the same four words of the banded twisted kernel (kkt_dense.hip) start here
constexpr int KKT_TW_FLAGS = 32;          // ints per rollout (one 128-byte line)
constexpr int KKT_TW_SPINS = 1 << 21;     // default bound of a wait (NewtonDev::kkt_tw_spins; cimpc_debug_set_tw_spins for the tests)
// exchange block of the two chains: [S00 | S11 | S10^T] (nd x nd each), c0, c1, dnu_{m+1}, dnu_m
ROUND_HD constexpr int kkt_tw_xch_doubles(int nd) { return 3 * nd * nd + 4 * nd; }

// ---- End-of-solve result block (solve_finish_kernel -> one device-to-host copy).  Counts travel as doubles (exact below 2^53).
//   [0..3] sums over the rollouts of NewtonDev::stats, [4] sum of the Newton iteration counts, [5..7] reserved,
//   then per rollout [u_1 (nu) | Newton iterations | r_norm]
enum ResultWord : int { RESULT_SWEEPS = 0, RESULT_IP_SOLVES = 1, RESULT_IP_ITERS = 2, RESULT_IP_FAILURES = 3, RESULT_NEWTON_SUM = 4 };
constexpr int RESULT_STATS = 4, RESULT_SUMS = 5, RESULT_HEADER = 8;
ROUND_HD constexpr int result_record(int nu) { return nu + 2; }
ROUND_HD constexpr size_t result_doubles(size_t B, int nu) { return RESULT_HEADER + B * (size_t)result_record(nu); }
ROUND_HD constexpr size_t result_u1(size_t b, int nu) { return RESULT_HEADER + b * (size_t)result_record(nu); }
// ... and within the rollout's record
ROUND_HD constexpr int record_iters(int nu) { return nu; }
ROUND_HD constexpr int record_r_norm(int nu) { return nu + 1; }

}  // namespace cimpc
