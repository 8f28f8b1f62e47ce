// Which kernel serves a KKT stage, in one place (plain C++: tests/native/kkt_plan_check.cpp builds it with g++).  select_kkt_backend
// picks the solver family per handle, choose_kkt_form the kernel per launch, from facts (KktCaps) the *_available functions test
// once per problem; launch_kkt_stage (newton_kernels.hip) launches the form it is given and re-tests nothing.
#pragma once
#include "../../../include/cimpc.h"

namespace cimpc {

enum class KktBackend {
    Condensed,        // dual Schur complement + block Cholesky on the fp64 MFMA (newton_impl.h: kkt_body)
    CondensedMixed,   // ... block products on the fp32 MFMA, fp64 refinement and fallback (CIMPC_KKT_CONDENSED_MIXED)
    Banded,           // banded LDL^T (kkt_dense.hip): :configuration mode with a velocity objective, or on request
    DenseLu,          // the reference default: dense jacobian! + LU with partial pivoting, any mode / objective
    CfCondensed,      // :configurationforce with negligible impulse weights, reduced onto the condensed solve ...
    CfBanded,         // ... or, with a velocity objective, onto the banded LDL^T
};

enum class KktForm {
    PerRollout,       // kkt_kernel: one one-wave workgroup per rollout
    Scalar,           // kkt_kernel_scalar: tiles beyond 24 or horizons beyond kkt_max_h
    Packed,           // kkt_kernel_packed: compact list, kkt_pack rollouts per workgroup
    Pipelined,        // kkt_kernel_pipe: three wavefronts per rollout
    Twisted,          // kkt_kernel_twisted: two workgroups of three wavefronts per rollout, one chain from either end
    Duo,              // kkt_kernel_duo: the two chains as two one-wave bodies in one workgroup
    BandedOneEnded,   // kkt_banded_kernel
    BandedTwisted,    // kkt_banded_twisted_kernel: two workgroups per rollout
    Dense,            // kkt_dense_kernel
    AsyncOneEnded,    // KKT job of the persistent kernel (newton_async_impl.h)
    AsyncTwoJob,      // ... as two cooperating jobs, the chains of the twisted solve (AsyncQ::kkt_tw)
};

// two chains per system that hand over through global memory with bounded waits (counted by cimpc_get_kkt_twisted)
inline bool two_ended(KktForm f) { return f == KktForm::Twisted || f == KktForm::Duo || f == KktForm::BandedTwisted || f == KktForm::AsyncTwoJob; }

// What the compiled kernels can do for the handle's problem.
struct KktCaps {
    bool cfg = false;             // :configuration mode
    bool velocity = false;        // TrackingVelocityObjective
    bool cf_tiny = false;         // :configurationforce impulse weights below fp64 resolution (max <= 1e-30)
    bool wide_tiles = false;      // nq or nu in 17 .. 24 (24-wide tiles)
    bool condensed = false;       // kkt_condensed_available: a compiled condensed solve for (nq, nu)
    bool mfma = false;            // kkt_mfma_available: ... whose per-rollout kernel is kkt_kernel (else kkt_kernel_scalar)
    bool packed = false;          // kkt_packed_available: the compact-list kernels apply (packed, pipelined, twisted, duo)
    bool twisted = false;         // kkt_twisted_available
    bool duo = false;             // kkt_duo_available
    bool mixed = false;           // kkt_mixed_available
    bool banded = false;          // kkt_banded_available in the form NewtonDev::band_reduce
    bool cf_reduce = false;       // kkt_cf_reduce_available (a velocity objective: in the form NewtonDev::band_reduce)
    bool banded_twisted = false;  // kkt_banded_twisted_available, on the problem the banded kernel solves (cf mode: cf_shadow)
};

// Schedule knobs that take part (Knobs::read_environment in cimpc_host.cpp reads the overrides).
struct KktPolicy {
    int kkt_pipe = -1;            // CIMPC_KKT_PIPE: three-wave pipelined kernel 0 never, >= 1 always, < 0 where the solve is on the critical path
    int kkt_twisted = -1;         // CIMPC_KKT_TWISTED: two-ended condensed solve 0 never, else by the rules; >= 2: the overlapped rounds' bound
    int kkt_duo = 1;              // CIMPC_KKT_DUO: 0 packed one-wave kernel next to the sweep, 1 the duo kernel where it applies, 2 also at the B1 seam
    int kkt_duo_hint = 20000;     // CIMPC_KKT_DUO_HINT: ... in rounds whose sweep has at most this many problems newly requested
    int kkt_duo_max = 256;        // ... for at most this many systems per launch (one workgroup per CU at a time)
    int kkt_tw_max = 120;         // twisted kernel for at most this many rollouts per launch (two workgroups each must be resident together)
    int kkt_pipe_max = 128;       // pipelined kernel for at most this many rollouts per round (it takes three times the waves)
    int async_kkt_tw = 1;         // CIMPC_ASYNC_KKT_TW: the persistent kernel's KKT stage as two jobs 0 never, 1 by size, 2 always
    bool lazy_dz = true;          // CIMPC_LAZY_DZ: 0 = the decision kernel copies the accepted sensitivities itself
    bool kkt_overlap = true;      // the handle's: the rounds' KKT stage on its own stream next to the sweep (from 64 rollouts on)
};

// Pair bound of the twisted kernel: two workgroups per rollout must be resident together, 120 rollouts per launch.
// Overlapped rounds take it where EVERY round's KKT set fits, i.e. batches of up to 120 rollouts - B = 96: 5.56 -> 4.8-5.1 ms
// per batch step; with a bound below the batch size the rounds mix kernels and lose (B = 128: 6.04 -> 6.8 ms at 48 / 96;
// B = 256 and 512 within the noise: profiles/r05/ab_tw_overlap.log).  CIMPC_KKT_TWISTED >= 2 is the bound itself (A/B lines).
inline int kkt_tw_overlap_max(const KktPolicy& p, int B) { return p.kkt_twisted >= 2 ? p.kkt_twisted : p.kkt_twisted != 0 && B <= p.kkt_tw_max ? p.kkt_tw_max : 0; }

// kkt_backend as requested (cimpc_newton_opts), narrowed to what the problem and the compiled kernels allow.
inline KktBackend select_kkt_backend(const KktCaps& c, int want) {
    if (!c.cfg) return want != CIMPC_KKT_DENSE_LU && c.cf_tiny && c.cf_reduce ? (c.velocity ? KktBackend::CfBanded : KktBackend::CfCondensed) : KktBackend::DenseLu;
    if (want == CIMPC_KKT_DENSE_LU) return KktBackend::DenseLu;
    // (dimension sets without a compiled condensed solve - the runtime-dimension path - take the banded LDL^T / dense LU)
    if (want == CIMPC_KKT_BANDED_LDL || c.velocity || !c.condensed) return c.banded ? KktBackend::Banded : KktBackend::DenseLu;
    if (want == CIMPC_KKT_CONDENSED_MIXED && c.mixed) return KktBackend::CondensedMixed;
    return KktBackend::Condensed;
}

// Lazy commit of the accepted sensitivities (NewtonDev::good_src): correct only where EVERY Newton-loop KKT stage is a kkt_body kernel on
// fp64 tiles, which reads through the index - for the condensed backend with `packed` and `mfma` choose_kkt_form returns no other.
inline bool kkt_lazy_commit(const KktPolicy& p, const KktCaps& c, KktBackend be) {
    return be == KktBackend::Condensed && p.lazy_dz && c.packed && c.mfma;
}

// Where the stage runs: the B1 seam (cimpc_kkt_solve, one solve over every rollout), a lock-step round with the KKT stage on the
// sweep's stream ahead of it (kkt_overlap off) or on its own stream next to it, the persistent kernel launched from reset (the
// whole solve) or taking over the rounds' last rollouts (hybrid tail).
struct KktSite {
    enum Kind { Seam, Round, Overlapped, Persistent, HybridTail } kind = Seam;
    int attempt = 0;               // Seam: 1 = repeat after a twisted hand-over timed out
    int n_kkt = 0;                 // rounds: systems to solve (blind: the batch size)
    bool blind = false;            // rounds: launched ahead of the host's knowledge of the previous round
    long long sweep_problems = 0;  // rounds: interior-point problems newly requested of this round's sweep (unknown when blind)
    bool tw_off = false;           // a twisted hand-over timed out earlier in this solve
    int B = 0;                     // rollouts of the handle
    int async_tail = 0;            // HybridTail: hand-over threshold of the hybrid schedule
    int waves = 4;                 // Persistent / HybridTail: waves per workgroup of the persistent kernel
};

inline KktForm choose_kkt_form(const KktPolicy& p, const KktCaps& c, KktBackend be, const KktSite& s) {
    const bool seam = s.kind == KktSite::Seam;
    // the banded LDL^T is launched over all rollouts of the handle: the twisted kernel's pair bound applies to the batch
    // (CIMPC_KKT_DUO=2 waives it, as at the seam below)
    const bool tw_batch = p.kkt_twisted != 0 && (s.B <= p.kkt_tw_max || p.kkt_duo == 2);
    const bool tw_now = seam ? s.attempt == 0 : !s.tw_off;
    const KktForm per_rollout = c.mfma ? KktForm::PerRollout : KktForm::Scalar;
    switch (be) {
    case KktBackend::DenseLu: return KktForm::Dense;
    case KktBackend::Banded:
    case KktBackend::CfBanded: return c.banded_twisted && tw_batch && tw_now ? KktForm::BandedTwisted : KktForm::BandedOneEnded;
    // fixed by the backend, per rollout: the mixed sequence, and the cf reduction's inner solve (its kernel fits the reduced problem)
    case KktBackend::CondensedMixed:
    case KktBackend::CfCondensed: return KktForm::PerRollout;
    case KktBackend::Condensed: break;
    }
    switch (s.kind) {
    case KktSite::Seam:
        // a lone solve is latency-bound: two chains from either end (CIMPC_KKT_DUO=2: the duo kernel, which the tests reach here)
        if (tw_batch && tw_now && p.kkt_duo == 2 && c.duo) return KktForm::Duo;
        if (tw_batch && tw_now && c.twisted) return KktForm::Twisted;
        return per_rollout;
    case KktSite::Round:
    case KktSite::Overlapped: {
        if (!c.packed) return per_rollout;
        const bool overlap = s.kind == KktSite::Overlapped, tw = tw_now && p.kkt_twisted != 0;
        const int n = s.n_kkt;
        // The three-wave pipelined kernel where the solve is on the critical path (not overlapped): next to a busy sweep it takes twice
        // the CUs for half the time - measured neutral - and the packed one-wave kernel stays.  Wide tiles hold one rollout per CU in
        // either kernel (105 KB / 128 KB of LDS): always taken there (BASELINE configs[4] at 64 rollouts: KKT 6.1 -> 3.2 ms per step,
        // 16.3 -> 13.3 ms; at 128 rollouts 24.2 -> 21.2 ms: profiles/r04/cent_kkt_pipe.log)
        const bool pipelined = p.kkt_pipe >= 0 ? p.kkt_pipe != 0 : (!overlap && n <= p.kkt_pipe_max) || c.wide_tiles;
        // Where the pipelined kernel runs, the twisted solve takes its place: two workgroups per rollout factor the block
        // penta-diagonal matrix from both ends (two chains of about H / 2 steps), as long as every pair is resident at once
        if (pipelined) return tw && n <= p.kkt_tw_max && c.twisted ? KktForm::Twisted : KktForm::Pipelined;
        if (!overlap || !tw || n <= 0) return KktForm::Packed;
        // ... and in the overlapped rounds of batches within the pair bound (kkt_tw_overlap_max): the packed one-wave recursion
        // (266 us) outlasts the thinning sweep next to it in the late rounds, the twisted pair does not
        if (!s.blind && n <= kkt_tw_overlap_max(p, s.B) && c.twisted) return KktForm::Twisted;
        // Next to the sweep the duo kernel (both chains as one-wave bodies in one workgroup, the packed workgroup's LDS) while every
        // system gets a workgroup at once: the packed recursion, 0.27 - 0.33 ms whatever the number of systems, outlasted the sweep in
        // 11 of the 16 rounds of the headline step.  Only next to sweeps SHORTER than that (80 us + 1 us per 112 problems): next to a
        // long one the packed kernel is off the critical path and takes half the CUs (duo everywhere: B = 1024 11.7 -> 12.5 ms; here:
        // B = 256 6.46 -> 5.89 ms, B = 512 unchanged).  NEWLY requested problems only: the parked ones depend on timing, and a choice
        // that followed them would make the iterates differ from run to run (the kernels agree to 1e-12, not to the bit).
        if (p.kkt_duo != 0 && n <= p.kkt_duo_max && !s.blind && s.sweep_problems <= p.kkt_duo_hint && c.duo) return KktForm::Duo;
        return KktForm::Packed;
    }
    case KktSite::Persistent:
    case KktSite::HybridTail: {
        // Two cooperating jobs where it was measured a gain: single launches of at most 32 rollouts (quadruped H = 40, B = 4 / 16 /
        // 32: 2.08 -> 1.85, 2.43 -> 2.27, 3.55 -> 3.41 ms; B = 64: 4.4 -> 4.9 ms - twice the jobs when every rollout reaches its KKT
        // stage at once; hybrid tail of B = 512: no difference in six alternating pairs) and hybrid tails of at most 32 rollouts
        // (B = 48 / 64 / 96 / 128: -1.5 / -3 / -1 / 0 % in alternating pairs).  16-wide tiles and four-wave workgroups.
        const int size = s.kind == KktSite::Persistent ? s.B : s.async_tail;
        const bool want = p.async_kkt_tw == 2 || (p.async_kkt_tw == 1 && size <= 32);
        return want && p.kkt_twisted != 0 && !s.tw_off && c.duo && s.waves >= 4 ? KktForm::AsyncTwoJob : KktForm::AsyncOneEnded;
    }
    }
    return per_rollout;
}

}  // namespace cimpc
