// How a solve is scheduled, in one place (plain C++: tests/native/schedule_plan_check.cpp builds it with g++): plan_schedule fixes the handle's
// launch shapes in cimpc_create, choose_solve_path the path of each solve, plan_round / plan_sweep each lock-step round and sweep launch.
#pragma once
#include <algorithm>
#include <cstddef>
#include "kkt_plan.h"

namespace cimpc {

// Schedule knobs with an environment override for the A/B scripts under scripts/ (Knobs::read_environment in cimpc_host.cpp).
struct SchedulePolicy {
    int async_mode = 2;          // CIMPC_ASYNC: 0 lock-step rounds only, 1 always the single launch, 2 auto
    int async_tail = -1;         // CIMPC_ASYNC_TAIL: hybrid hand-over threshold (-1: by batch size)
    int async_full_max = 32;     // CIMPC_ASYNC_FULL_MAX: largest batch solved by the single persistent launch alone (larger: hybrid).
                                 // Measured 128 -> 64 (round 3): B = 96 8.88 -> 8.11 ms, B = 128 9.72 -> 9.48 ms, B = 64 unchanged (6.9 ms); 64 -> 32 (round 6,
                                 // after the rounds' sweep and KKT stage got faster): B = 64 5.0-5.7 -> 4.35-4.4 ms, B = 48 4.54 -> 4.07 ms with the hand-over at 32
    int spec_first = -1;         // CIMPC_SPEC_FIRST: step lengths of the first line-search round of a solve's first Newton iteration (-1: by batch size)
    int iter_cap = 28;           // CIMPC_ITER_CAP (B = 512: 20 / 24 / 28 / 32 -> 8.73 / 8.65 / 8.74 / 8.56 ms, inside the spread: profiles/r03/knobs3.log)
                                 // (measured B = 512: 16 / 20 / 24 / 32 / 48 -> 13.57 / 12.73 / 12.85 / 12.97 / 14.41 ms per batch step)
    int tail_div = 8;            // CIMPC_TAIL_DIV
    int drain_pct = 95;          // CIMPC_DRAIN_PCT: drain parking once this percentage of the sweep's workgroups has left (0 = off; B = 512: 0 / 75 / 90 / 95 / 97 -> 10.68 / 10.97 / 10.48 / 10.45 / 10.47 ms)
    int drain_min = 4;           // CIMPC_DRAIN_MIN: ... for solves that have had at least this many iterations in the launch
    int sweep_wgs = 0;           // CIMPC_SWEEP_WGS: persistent sweep workgroups (0: computed from the resident set) - sub-batch experiments
    int waves32 = 0;             // CIMPC_WAVES32: waves per sweep workgroup of the 32-lane models (0: by batch size; 4 = latency build, 8 = throughput build)
};
struct ScheduleFacts {             // what the host knows of the handle
    int B = 1, H = 1, H_ref = 1, G = 16;   // G: lanes per problem (KernelInfo::G), 16, 32 or 64
    bool async_available = false;  // the persistent kernel serves the handle (newton_async_available, H_ref <= 256, queues within 1 GiB)
};
struct SchedulePlan {         // the handle's schedule (cimpc_create)
    ScheduleFacts f;
    bool async_on = false, single_launch = false, hybrid = false;   // persistent kernel allocated; a condensed solve is its ONE launch / rounds + its tail
    int async_tail = 96;         // hybrid: hand over to the asynchronous kernel when at most this many rollouts are active
    int waves = 4, wpk = 1;      // waves per sweep workgroup, persistent workgroups of a sweep launch
    long long adapt32 = 0;       // 32-lane models: problems per sweep launch from which the throughput build is taken (0: the handle's one build)
    int async_grid = 0, async_service = 0;   // workgroups of the persistent kernel launched from reset, job-only ones among them
    int tail_grid = 0, tail_service = 0;     // ... of the one that takes over the hybrid's tail
    int spec_all = 3, spec_first = 3, spec_mid = 8, spec_tail = 3;   // line-search speculation (NewtonDev)
    bool kkt_overlap = false;    // the rounds' KKT stage on its own stream next to the sweep
};
constexpr int async_idle_sleep = 2, async_idle_spins = 48, async_wake_fan = 1;   // idle back-off of the asynchronous kernel (AsyncQ; ~2 us units), polls before looking around, wake-up fan

inline SchedulePlan plan_schedule(const SchedulePolicy& p, const ScheduleFacts& f) {
    SchedulePlan s;
    const int B = (s.f = f).B;
    // asynchronous single-launch solve? CIMPC_ASYNC: 0 = lock-step rounds only, 1 = always the single launch, unset / 2 = auto. Measured on MI355X (quadruped, H =
    // 40): the single launch wins for 4 <= B <= 128 rollouts (B = 64: 8.1 vs 11.2 ms), the rounds win for large batches (B = 512: 16.5 vs
    // 21.7 ms) - except for their sparse tail, which auto mode hands over to the asynchronous kernel.
    s.async_on = p.async_mode != 0 && f.async_available;
    s.single_launch = s.async_on && (p.async_mode == 1 || (p.async_mode == 2 && B >= 4 && B <= p.async_full_max));
    s.hybrid = s.async_on && p.async_mode == 2 && !s.single_launch && B > p.async_full_max;
    // measured: B = 512 -> 48 .. 96 flat; B = 1024 / 2048 -> 96 (11.1 / 18.85 ms against 11.4 / 19.5 at 170 / 256:
    // the persistent kernel's chains do not get shorter with more rollouts handed over, the rounds do)
    // (round 6, mid-size batches: B = 48 / 64 / 96 best at 32 - 4.07 / 4.35 / 4.41 ms -, B = 128 at 32-48 - 4.91 -, B = 192 at 48 - 4.76 ms against 5.30
    //  with the rule above: scripts/dbg/headline_b.sh)
    // 32-lane models (centroidal: one workgroup per CU, 512-register waves): the persistent kernel wins up to 32 rollouts only and the
    // rounds keep their lead far into the tail - measured on BASELINE configs[4] (H = 60): B = 8 / 16 / 32 / 64 / 128 -> single launch
    // 10.7 / 14.1 / 19.3 / 29.5 / - ms, lock-step rounds 12.1 / 17.7 / 20.5 / 22.4 / 34.9 ms, hand-over at 16 active rollouts 22.3 / 35.7 ms
    s.async_tail = p.async_tail >= 0 ? p.async_tail : f.G == 32 ? 16 : B < 256 ? std::max(32, B / 4) : std::min(96, std::max(64, B / 6));
    // all-seven-step-lengths speculation: shortens the chain of rollouts that exhaust their line search; pays
    // when the solve is latency-bound (small batches), costs throughput otherwise (B = 2048: -8 %)
    s.spec_all = B <= 128 ? 3 : 8;
    // first line search of a solve (no history yet): 1, 1/2, 1/4 evaluated together up to mid-size batches (B = 512: 9.65 -> 9.50 ms,
    // B = 128: 8.14 -> 8.03 ms for 0.3 more evaluated sweeps per step; B = 2048: 25.4 -> 25.6 ms, throughput-bound: one candidate there)
    s.spec_first = p.spec_first >= 0 ? p.spec_first : (B <= 1024 ? 3 : 1);
    // large batches: a rollout whose previous search needed a back-off starts the next one with 1, 1/2, 1/4 together (one round less per Newton iteration for 0.9
    // more evaluated sweeps per step: B = 512 11.4 -> 10.9 ms); small batches already evaluate all seven step lengths from depth 3 on
    s.spec_mid = B > 128 ? 1 : 8;
    s.kkt_overlap = B >= 64;
    // 4 waves share one staged table (throughput); measured for single rollouts too (one problem per knot anyway): B = 1 quadruped H = 40 cold 0.945 -> 0.926 ms,
    // warm MPC loop 3.19 -> 3.03 ms, hopper H = 20 1.02 -> 0.97 ms against 1 wave
    // 32-lane models (round 4): from about three problems per lane group and sweep on, the throughput build of the sweep - eight waves per
    // workgroup, two per SIMD (ip_kernel_impl.h: ip_queue_kernel<M, WIDE>; centroidal H = 60: 64 rollouts 7.9 -> 11.6 ms of sweeps per
    // step, 128 rollouts 14.0 -> 12.2 ms, 256 rollouts 26.0 -> 22.4 ms - profiles/r04/cent_w8b.log).  CIMPC_WAVES32 = 4 / 8 forces one.
    // (A first form that ALSO read the MGS column twice instead of keeping it in registers was LDS-bound: cent_8wave_experiment.log.)
    if (f.G == 32) {
        if (p.waves32 > 0 && p.waves32 < 1000) s.waves = p.waves32;
        else if ((size_t)B * f.H >= 6000) s.waves = 8;
        // Round 5: the build is chosen PER LAUNCH (plan_sweep) from the problems queued for it - a step of 64 rollouts has launches of
        // 3.8 k (one candidate per rollout) to 11.5 k problems (three): centroidal H = 60, 64 rollouts 7.87 -> 6.7 ms of sweeps per
        // step (10.7 -> 9.6 ms per batch step), 128 rollouts 12.0 -> 11.5 ms; thresholds 5 / 7 / 9 / 11 k are equivalent at 64,
        // 5 - 7 k best at 128 (profiles/r05/cent_adapt32.log).  CIMPC_WAVES32 >= 1000 sets the threshold, 4 / 8 force one build.
        s.adapt32 = p.waves32 >= 1000 ? p.waves32 : (p.waves32 == 4 || p.waves32 == 8) ? 0 : 7000;
    }
    // the single-launch solve runs its residual jobs on the whole workgroup: 4 waves also for small batches
    // (measured B = 8: 5.2 -> 4.4 ms, B = 64: 8.5 -> 7.5 ms)
    // (quirk kept from the measurements: decided at create, whatever KKT backend the solves later take)
    if (s.single_launch) s.waves = 4;
    // persistent workgroups of a sweep launch: all resident (256 VGPRs -> 8 waves per CU), about two problems per lane group in a full round, and never fewer
    // workgroups than busy knots (a workgroup serves one knot at a time)
    const size_t groups_per_wg = (64 / f.G) * s.waves;
    const size_t nprob = (size_t)B * f.H;
    size_t w = (nprob + 2 * groups_per_wg - 1) / (2 * groups_per_wg);
    w = std::max<size_t>(w, std::min<size_t>(f.H_ref, nprob));
    // (32-lane models run one wave per SIMD - 512 registers - i.e. 4 waves per CU; the asynchronous launcher
    //  clamps its grid to the occupancy the runtime reports in any case)
    const size_t resident = (size_t)256 * std::max(1, (f.G == 16 ? (s.waves > 4 ? 2 * s.waves : 8) : 4) / s.waves);
    s.wpk = p.sweep_wgs > 0 ? p.sweep_wgs : (int)std::max<size_t>(1, std::min<size_t>(w, resident));
    // asynchronous solve: the same resident set plus dedicated residual/KKT workgroups
    // (a line-search burst is up to 7 evaluations x H knots per rollout and every knot needs a workgroup of its own: small batches get at least 240 - measured B =
    //  8: 6.4 -> 5.1 ms, B = 128: 11.1 -> 10.3 ms)
    const int a_wgs = p.sweep_wgs > 0 ? s.wpk : std::max(s.wpk, 240);
    s.async_service = std::max(1, a_wgs / 8);
    s.async_grid = std::max((int)std::min<size_t>(resident, (size_t)a_wgs + s.async_service), s.async_service + 1);
    // hybrid tail: few rollouts left - a smaller resident set means fewer idle workgroups polling next to the working ones: 3 per
    // rollout handed over (B = 512: 512 / 320 / 256 / 192 / 96 workgroups -> 10.85 / 10.42 / 10.35 / 10.38 / 10.6 ms)
    // (256 = one workgroup per CU: the tail is latency bound, co-resident workgroups slow each other)
    const int tail = std::max(256, 3 * s.async_tail);
    s.tail_grid = std::min(tail, s.async_grid);
    s.tail_service = tail < s.async_grid ? std::max(1, tail / 8) : s.async_service;
    return s;
}

// The persistent kernel solves the condensed KKT only; the backend can change after cimpc_create (cimpc_set_objective).
enum class SolvePath { Rounds, Persistent, Hybrid };
inline SolvePath choose_solve_path(const SchedulePlan& s, KktBackend be) {
    return be != KktBackend::Condensed ? SolvePath::Rounds : s.single_launch ? SolvePath::Persistent : s.hybrid ? SolvePath::Hybrid : SolvePath::Rounds;
}
// Lock-step rounds: safety net only: every Newton iteration needs at most 3 (speculative) rounds, each evaluation at most ceil(max_iter / iter_cap) launches of the
// resumable interior-point sweep
// (drain parking guarantees drain_min iterations of progress per launch, iter_cap parking iter_cap)
inline int max_rounds(const SchedulePolicy& p, int newton_max_iter, int ip_max_iter) {
    const int min_progress = p.drain_pct > 0 ? std::min(p.iter_cap, p.drain_min) : p.iter_cap;
    return (newton_max_iter * 8 + 2) * ((ip_max_iter + min_progress - 1) / min_progress + 1);
}

// Single rollouts (B < 4: below the persistent kernel's range) keep ONE round queued ahead of the one the host waits for: such a round is launched BLIND - KKT
// kernel on the full list range with its count read on the device, everything else is device-driven anyway - and costs three empty launches if the solve turns out
// to be over; in exchange no round waits for the host to see the previous one's stamp and launch (about 10 us per round of a 0.7 ms solve). Warm-started solves only
// - the cadence of an MPC loop, five Newton iterations over eight to ten rounds: hopper H = 20 0.652 -> 0.614 ms per MPC step; the four rounds of a cold start lose
// more to the empty launches than they gain (0.685 -> 0.706 ms).
// (not with a wall-clock budget: the round queued ahead would still run - and step the trajectory - after the host has stopped waiting, newton.jl:187-277 ends
//  silently at the check)
inline bool round_ahead(const SchedulePlan& s, KktBackend be, bool warm_start, bool budget) { return s.f.B < 4 && be != KktBackend::CondensedMixed && warm_start && !budget; }
// A lock-step round: its sweep's parking cap, the residual launch over n_slots listed slots or every (rollout, slot) pair (-1; -2: B < 4),
// split_join: the slot kernel ahead of the join with the overlapped KKT stage.  blind: launched ahead of the host's view of the last round.
struct RoundPlan { int cap, n_slots; bool split_join; };
inline RoundPlan plan_round(const SchedulePolicy& p, const SchedulePlan& s, int ip_max_iter, bool kkt, bool blind, int last_sweep, int last_slots) {
    // parking (iter_cap) protects a busy round from one long solve; in the sparse tail of a solve it only adds rounds, so a round that serves few rollouts lets
    // every solve run to the end
    // (batches below tail_div rollouts never park: a round there is as long as its longest solve whichever way it is cut)
    // (in a blind round `last_sweep` is one round stale: the cap is then chosen without it)
    const bool sparse = p.tail_div > 0 && (s.f.B < p.tail_div || (!blind && (long long)last_sweep * p.tail_div <= s.f.B));
    const int cap = sparse ? ip_max_iter : p.iter_cap;
    // the evaluation slots of this round: the compact list its requesters built (small batches run the KKT stage in the same
    // round as the evaluation of its candidates - not known to the host at launch: every (rollout, slot) pair gets a block there)
    const int n_slots = s.kkt_overlap ? last_slots : (s.f.B < 4 ? -2 : -1);
    // round 4: the per-slot residual kernel goes in FRONT of the join with the overlapped KKT kernel (it reads the sweep's results only; the rollouts the KKT kernel
    // works on have no slot on this round's list), the decision kernel behind it - in the rounds whose KKT recursion outlasts the sweep (about six per step of the
    // headline batch) the 26 us of the slot kernel leave the critical path
    return {cap, n_slots, kkt && s.kkt_overlap && n_slots >= 0};
}

// hybrid: sparse tail: few rollouts left, every round pays its fixed latency for them -> the persistent kernel finishes them along their own chains
inline bool hand_over(const SchedulePlan& s, int active) { return active > 0 && active <= s.async_tail; }
// A sweep launch (IpParams: drain_thresh 0 = no drain parking).  hint: problems of the launch as far as the host knows them (<= 0:
// unknown); iter_cap: the launch's parking cap; drain: the launch has a drain counter (lock-step rounds)
struct SweepLaunch { int waves, wpk; bool direct; int drain_thresh; };
inline SweepLaunch plan_sweep(const SchedulePolicy& p, const SchedulePlan& s, long long hint, int iter_cap, int ip_max_iter, bool drain) {
    SweepLaunch l{s.waves, s.wpk, false, 0};
    // 32-lane models: the build of the sweep is chosen PER LAUNCH from the problems the host knows to be queued (round 5; the choice
    // used to be made once per handle from B H): the latency build (4 waves per workgroup) below `adapt32` problems, the throughput
    // build (8 waves, two per SIMD) from there on.  Parked iterates are the model's, not the build's: a solve may change builds.
    // (only where the host's count is complete: with the KKT stage in the same round as the evaluation of its candidates - small
    //  batches - the requests of that round are not known at launch; a first version sized a B = 1 sweep for ONE workgroup: 1.1 -> 20 ms)
    // (adapt32 > 0: a 32-lane model without a forced build; an explicit CIMPC_SWEEP_WGS keeps its grid)
    if (s.adapt32 > 0 && hint > 0 && s.kkt_overlap && p.sweep_wgs <= 0) {
        l.waves = hint >= s.adapt32 ? 8 : 4;
        const size_t groups_per_wg = 2 * (size_t)l.waves;
        size_t w = ((size_t)hint + 2 * groups_per_wg - 1) / (2 * groups_per_wg);
        w = std::max<size_t>(w, std::min<size_t>((size_t)s.f.H_ref, (size_t)std::max<long long>(hint, 1)));
        l.wpk = (int)std::max<size_t>(1, std::min<size_t>(w, 256));
    }
    // (round 4, measured and removed: one sweep workgroup per CU in rounds with few problems - <= 4 k / 8 k / 16 k - so that every
    //  wave has its SIMD to itself: 7.97 -> 7.96 / 7.99 / 8.01 ms per step, no effect: profiles/r04/knob_small_round.log)
    // single rollouts (B < 4: at most 7 B problems per knot): one workgroup per knot, no remaining-work scans (IpParams::direct)
    if (s.f.B < 4 && p.sweep_wgs <= 0) { l.direct = true; l.wpk = s.f.H_ref; }
    if (drain && p.drain_pct > 0 && iter_cap < ip_max_iter) l.drain_thresh = std::max(1, (int)((long long)l.wpk * p.drain_pct / 100));
    return l;
}

}  // namespace cimpc
