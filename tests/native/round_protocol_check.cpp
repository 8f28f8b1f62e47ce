// Host-only driver of contactimplicitmpc/jl_amd/csrc/round_protocol.h (tests/test_round_protocol.py): no input; one output line per
// block of the protocol, "<block> name=value ...".  Offsets of pointer accessors are measured on a dummy array.
#include "../../contactimplicitmpc/jl_amd/csrc/round_protocol.h"

#include <cstdio>
#include <initializer_list>

using namespace cimpc;

int main() {
    static int mem[4096];
    printf("counters sweep=%d kkt=%d parked=%d drained=%d slots=%d new_slots=%d ticket=%d count=%d pad=%d ints=%d", RC_SWEEP, RC_KKT, RC_PARKED,
           RC_DRAINED, RC_SLOTS, RC_NEW_SLOTS, RC_TICKET, ROUND_COUNTERS, CPAD, ROUND_COUNTER_INTS);
    for (int k = 0; k < ROUND_COUNTERS; ++k) printf(" at%d=%d", k, (int)(round_counter(mem, k) - mem));
    printf(" block0=%d block1=%d\n", (int)(round_counter_block(mem, 0) - mem), (int)(round_counter_block(mem, 1) - mem));

    printf("ring n_sweep=%d n_kkt=%d stamp=%d abort=%d parked=%d finished=%d slots=%d new_slots=%d stride=%d nslots=%d alloc=%d", RING_N_SWEEP,
           RING_N_KKT, RING_STAMP, RING_ABORT, RING_PARKED, RING_FINISHED, RING_SLOTS, RING_NEW_SLOTS, RING_SLOT_INTS, RING_SLOTS_COUNT, RING_ALLOC_INTS);
    for (int r = 0; r < 4; ++r) printf(" round%d=%d", r, (int)(ring_slot(mem, r) - mem));
    printf(" abort_word=%d published=", (int)(ring_abort_word(mem) - mem));
    for (size_t k = 0; k < sizeof(RING_PUBLISHED) / sizeof(RING_PUBLISHED[0]); ++k) printf("%s%d", k ? "," : "", (int)RING_PUBLISHED[k]);
    printf("\n");

    for (size_t K : {(size_t)1, (size_t)40, (size_t)256}) {
        const QueueCtl q = queue_ctl(K);
        printf("queue_ctl K=%zu qpad=%d count=%zu head=%zu counters=%zu ints=%zu\n", K, QPAD, q.count, q.head, q.counters, q.ints);
        const AsyncCtl a = async_ctl(K);
        printf("async_ctl K=%zu count=%zu head=%zu jobs=%zu rq_head=%zu n_done=%zu rq_tail=%zu kq_head=%zu kq_tail=%zu epoch=%zu ints=%zu clear=%d\n", K,
               a.count, a.head, a.jobs, a.rq_head, a.n_done, a.rq_tail, a.kq_head, a.kq_tail, a.epoch, a.ints, ASYNC_JOB_INTS);
    }

    printf("epoch stride=%d buckets=%d words=%d any=%d", EPOCH_STRIDE, EPOCH_BUCKETS, EPOCH_WORDS, epoch_any_job());
    for (int b = 0; b < EPOCH_BUCKETS; ++b) printf(" ip%d=%d job%d=%d", b, epoch_ip(b), b, epoch_job(b));
    printf(" bucket_of_17=%d bucket_of_511=%d\n", epoch_bucket(17), epoch_bucket(511));

    printf("kjob shift=%d mask=%d one_ended=%d top=%d bottom=%d retry=%d\n", KJOB_SHIFT, KJOB_MASK, KJOB_ONE_ENDED, KJOB_TOP, KJOB_BOTTOM, KJOB_RETRY);

    printf("twisted traces=%d middle=%d finished=%d timed_out=%d band0=%d line=%d spins=%d", TW_TRACES, TW_MIDDLE, TW_FINISHED, TW_TIMED_OUT,
           KKT_BAND_TW_FLAG0, KKT_TW_FLAGS, KKT_TW_SPINS);
    for (int nd : {1, 7, 18, 30}) printf(" xch%d=%d", nd, kkt_tw_xch_doubles(nd));
    printf("\n");

    printf("result sweeps=%d ip_solves=%d ip_iters=%d ip_failures=%d newton_sum=%d stats=%d sums=%d header=%d", RESULT_SWEEPS, RESULT_IP_SOLVES,
           RESULT_IP_ITERS, RESULT_IP_FAILURES, RESULT_NEWTON_SUM, RESULT_STATS, RESULT_SUMS, RESULT_HEADER);
    const int shapes[3][2] = {{1, 8}, {512, 8}, {64, 12}};
    for (const auto& s : shapes) {
        const int B = s[0], nu = s[1];
        printf(" doubles_%d_%d=%zu record_%d=%d iters_%d=%d r_norm_%d=%d u1_last_%d_%d=%zu", B, nu, result_doubles(B, nu), nu, result_record(nu), nu,
               record_iters(nu), nu, record_r_norm(nu), B, nu, result_u1(B - 1, nu));
    }
    printf("\n");
    return 0;
}
