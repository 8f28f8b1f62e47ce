// Host runtime behind the C ABI of include/cimpc.h: handle, HBM residency, the per-knot
// linearization tables (A1; built by lin_table_build.h), window bucketing, and the lock-step driver of newton_solve!
// (/root/reference/src/controller/newton.jl:169-288).  HIP runtime only - no torch, no BLAS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cimpc_internal.h"
#include "lin_table.h"
#include "lin_table_build.h"
#include "model_table.h"
#include "newton_state.h"
#include "gains.h"
#include "handle_state.h"
#include "plant_linearize.h"
#include "schedule_plan.h"

using namespace cimpc;

namespace {

thread_local std::string g_create_error;

enum ProfClass { PC_IP = 0, PC_KKT = 1, PC_RESID = 2, PC_OTHER = 3, PC_ASYNC = 4, PC_COUNT = 5 };

struct ProfRec {
    hipEvent_t a, b;
    int cls;
};

}  // namespace

// Streams of the lock-step rounds: the sweep / residual chain runs on `st`, the KKT recursion of the
// rollouts that start a Newton iteration on `st_kkt` next to it (joined by an event before the residual).
struct RoundStreams {
    hipStream_t st = nullptr;
    hipStream_t st_kkt = nullptr;
    hipEvent_t ev_join = nullptr;   // end of the round's KKT kernel
    hipEvent_t ev_start = nullptr;  // the caller's stream at the start of a solve (uploads of q0 / q1 precede the reset kernel)
};

// Settings with an environment override for the A/B scripts under scripts/, read ONCE in cimpc_create (no solve-path call touches the
// environment).  The defaults are the measured optima; the rules that use them are in schedule_plan.h and kkt_plan.h.
struct Knobs {
    SchedulePolicy sched{};      // CIMPC_ASYNC, _ASYNC_TAIL, _ASYNC_FULL_MAX, _SPEC_FIRST, _ITER_CAP, _TAIL_DIV, _DRAIN_PCT, _DRAIN_MIN, _SWEEP_WGS, _WAVES32
    bool async_debug = false;    // CIMPC_ASYNC_DEBUG
    double watchdog_s = 30.0;    // CIMPC_ASYNC_WATCHDOG_S
    bool debug_rounds = false;   // CIMPC_DEBUG_ROUNDS
    bool generic_static = false; // CIMPC_GENERIC_STATIC: runtime-dimension sweep with the static queue partition of rounds 2-3 instead of the dynamic pull
    KktPolicy kkt{};             // CIMPC_KKT_PIPE, _TWISTED, _DUO, _DUO_HINT, CIMPC_LAZY_DZ, CIMPC_ASYNC_KKT_TW and the KKT kernels' bounds (kkt_plan.h)
    int kkt_tw_nb = 0;           // CIMPC_KKT_TW_NB: rows eliminated from the bottom (0: the default split)
    int kkt_tw_spins = 0;        // bound of a chain's wait for its partner, in polls (0: 2^21); the tests force the time-out path through cimpc_debug_set_tw_spins
    int banded_form = 0;         // CIMPC_BANDED_FORM: banded LDL^T variants the sizes in the tree never reach - bit 0: four pivots per block, bit 1: window
                                 // of w + RB slots instead of the next power of two, bit 2: controls not eliminated (the form a singular R_t
                                 // falls back to) - tests/test_gpu_round4.py runs every form against form 0

    static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
    void read_environment() {
        sched.async_mode = env_int("CIMPC_ASYNC", sched.async_mode);
        sched.async_tail = env_int("CIMPC_ASYNC_TAIL", sched.async_tail);
        sched.spec_first = env_int("CIMPC_SPEC_FIRST", sched.spec_first);
        sched.iter_cap = std::max(1, env_int("CIMPC_ITER_CAP", sched.iter_cap));
        async_debug = getenv("CIMPC_ASYNC_DEBUG") != nullptr;
        if (const char* v = getenv("CIMPC_ASYNC_WATCHDOG_S")) watchdog_s = atof(v);
        debug_rounds = getenv("CIMPC_DEBUG_ROUNDS") != nullptr;
        sched.tail_div = env_int("CIMPC_TAIL_DIV", sched.tail_div);
        sched.async_full_max = env_int("CIMPC_ASYNC_FULL_MAX", sched.async_full_max);
        sched.drain_pct = env_int("CIMPC_DRAIN_PCT", sched.drain_pct);
        sched.drain_min = std::max(1, env_int("CIMPC_DRAIN_MIN", sched.drain_min));
        kkt.kkt_pipe = env_int("CIMPC_KKT_PIPE", kkt.kkt_pipe);
        kkt.kkt_twisted = env_int("CIMPC_KKT_TWISTED", kkt.kkt_twisted);
        kkt_tw_nb = env_int("CIMPC_KKT_TW_NB", kkt_tw_nb);
        kkt.lazy_dz = env_int("CIMPC_LAZY_DZ", 1) != 0;
        kkt.kkt_duo = env_int("CIMPC_KKT_DUO", kkt.kkt_duo);
        kkt.kkt_duo_hint = env_int("CIMPC_KKT_DUO_HINT", kkt.kkt_duo_hint);
        kkt.async_kkt_tw = env_int("CIMPC_ASYNC_KKT_TW", kkt.async_kkt_tw);
        generic_static = env_int("CIMPC_GENERIC_STATIC", generic_static ? 1 : 0) != 0;
        sched.sweep_wgs = env_int("CIMPC_SWEEP_WGS", sched.sweep_wgs);
        sched.waves32 = env_int("CIMPC_WAVES32", sched.waves32);
        banded_form = env_int("CIMPC_BANDED_FORM", banded_form);
    }
};

struct cimpc_ctx {
    cimpc_dims dm{};
    Knobs kn{};
    cimpc_ip_opts ip{};
    cimpc_newton_opts nt{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    KernelInfo ki{};
    int nz = 0, nth = 0, nths = 0, nd = 0, nr = 0, nx = 0, ny = 0, N = 0;
    // device memory
    std::vector<void*> allocs;
    double* d_tab = nullptr;
    IpQueues Q{};                // device work queues (par is set per launch)
    int* d_window = nullptr;
    // cimpc_set_gait: the controller's full reference trajectory + per-rollout step counters
    double *g_q = nullptr, *g_u = nullptr, *g_w = nullptr, *g_g = nullptr, *g_b = nullptr, *g_th = nullptr, *g_stride = nullptr;
    int* g_phase = nullptr;
    int* d_good_src = nullptr;      // [B][H] NewtonDev::good_src (in use where kkt_lazy_commit holds: set_kkt_backend)
    double* d_dz_knot = nullptr;    // [B][H_ref][nths*nd] per-knot archive, allocated at the first window change that needs it
    double* d_alt = nullptr;
    double* d_zout = nullptr;
    double *d_Q = nullptr, *d_R = nullptr, *d_Qinv = nullptr, *d_Rinv = nullptr, *d_Cg = nullptr,
           *d_Cb = nullptr;
    double *d_q0 = nullptr, *d_q1 = nullptr;      // one allocation: d_q1 = d_q0 + B nq (uploaded by one copy)
    double* h_qin = nullptr;     // pinned staging of [q0 | q1], then nq doubles for the stride of cimpc_mpc_advance
    double* h_stage = nullptr;   // pinned staging of cimpc_mpc_solve (window, reference, altitude in; trajectory out), allocated at its first call
    size_t h_stage_doubles = 0;
    double* d_result = nullptr;  // end-of-solve result block (solve_finish_kernel): result_doubles(B, nu)
    double* h_result = nullptr;  // ... its pinned host copy, valid from the end of a solve to the next call that touches the state
    double* d_rhs = nullptr;   // B1 seam staging
    double* d_pstate = nullptr;   // parked interior-point iterates
    long long ip_budget_ticks = 0;  // cimpc_ip_opts::max_time in ticks of the device's constant-rate clock (0 = unlimited)
    NewtonDev S{};
    int* h_counters = nullptr;   // pinned
    // bookkeeping
    std::vector<char> knot_set;
    int n_knots_set = 0;
    HandleState st;              // what is set, where the window lives, who may latch (handle_state.h): read and changed through its names only
    // KKT stage (kkt_plan.h): the knobs that take part, what the kernels can do for the problem, the solver family
    KktPolicy kp{};
    KktCaps kc{};
    KktBackend kb = KktBackend::Condensed;
    long long n_kkt_twisted = 0;   // KKT launches that took the twisted kernel (cimpc_get_kkt_twisted)
    int* h_twfail = nullptr;       // host-mapped: hand-overs of the twisted kernels that timed out (NewtonDev::kkt_tw_fail), never reset
    int twfail_seen = 0;           // ... its value when the host last looked
    long long n_kkt_tw_fallbacks = 0;   // KKT stages repeated on the one-ended kernels after such a time-out (cimpc_get_kkt_twisted_fallbacks)
    bool band_reduce_ok = false;   // every R_t could be inverted: the banded LDL^T may eliminate the controls first (NewtonDev::band_reduce)
    double* d_mix_ws = nullptr;
    int* d_mix_nfb = nullptr;
    size_t dense_ws_doubles = 0;
    // :configurationforce with negligible gamma / b weights: eliminated onto the :configuration solvers (newton_kernels.hip)
    bool cf_tiny = true;
    double* d_cf_ws = nullptr;
    double* d_dense_ws = nullptr;  // [B][N*N + 2N], allocated on first use
    double *d_V = nullptr, *d_qt = nullptr, *d_vt = nullptr;
    int* d_ring = nullptr;       // the two round-counter blocks (behind the queue counters: queue_ctl, Q.count .. +ctl_ints)
    size_t ctl_ints = 0;
    int* h_ring = nullptr;       // pinned, host-mapped ring (round_protocol.h: RingWord)
    int* h_ring_dev = nullptr;   // device pointer of h_ring
    // asynchronous single-launch solve (newton_async_impl.h)
    SchedulePlan sched{};        // launch shapes and paths of the solves (schedule_plan.h)
    bool async_dirty = true;     // the persistent kernel's queues may hold entries an aborted solve left behind
    int* a_items = nullptr;      // [K][a_cap] live interior-point queues
    int* a_jobs = nullptr;       // residual job entries, then KKT job entries
    int* a_ctrl = nullptr;       // control block of the persistent solve (round_protocol.h: async_ctl)
    int* a_evals = nullptr;      // [B]
    long long* a_dbg = nullptr;  // [16] diagnostics (CIMPC_ASYNC_DEBUG)
    size_t a_cap = 0, a_rq_cap = 0, a_kq_cap = 0;
    RoundStreams rs;
    bool external_stream = false;
    std::vector<double> h_tab;       // one knot staging
    std::vector<double> h_tab_work;  // the host build's workspace (lin_table_build.h)
    // device table build (cimpc_set_linearization_batch, cimpc_linearize_knots), grow-only: z0 | th0 | terrains | r0 | rz0 | rth0 of
    // the call's knots, their tables as built (committed to d_tab only when every knot's Dx could be inverted), one status word each
    double* d_tb = nullptr;
    size_t tb_cap = 0;
    // feedback gains (cimpc_set_gains, cimpc_gain_latch, cimpc_gain_feedback): K of every reference knot, what the last latch kept
    // per rollout (gains.h: gain_latch_doubles) and the staging of a feedback call [q_prev | q_cur | u]; allocated at the first cimpc_set_gains
    double *d_gK = nullptr, *d_glatch = nullptr, *d_gio = nullptr;
    cimpc_stats last_stats{};
    // profiling
    int prof_on = 0;             // 0 off, 1 every launch, 2 the interior-point sweep launches only (cimpc_profile_enable)
    bool prof_open = false;      // the last prof_begin recorded an event pair (prof_end closes it)
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[PC_COUNT] = {0, 0, 0, 0, 0};
    long long prof_n[PC_COUNT] = {0, 0, 0, 0, 0};
    long long prof_async_problems = 0;
    long long prof_ip_problems = 0, prof_kkt_systems = 0;
};

namespace {

int fail(cimpc_ctx* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    else g_create_error = msg;
    return code;
}
int refuse(cimpc_ctx* h, const Refusal& r) { return r.code == CIMPC_OK ? CIMPC_OK : fail(h, r.code, r.msg); }

}  // namespace

void cimpc::set_global_error(const std::string& msg) { g_create_error = msg; }

namespace {

#define HIP_TRY(h, call)                                                                     \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail(h, CIMPC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

template <class T>
int dev_alloc(cimpc_ctx* h, T** p, size_t count) {
    void* v = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&v, count * sizeof(T));
    if (e != hipSuccess) return fail(h, CIMPC_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    e = hipMemset(v, 0, count * sizeof(T));
    // the fill runs on the NULL stream, which the library's non-blocking streams do not wait for: a buffer
    // allocated lazily right before a launch (dense KKT workspace) must be clean before anything touches it
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(h, CIMPC_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    h->allocs.push_back(v);
    *p = static_cast<T*>(v);
    return CIMPC_OK;
}

// The handle's table layout, the one its kernels read (ki.tab_size doubles per knot)
int table_layout(cimpc_ctx* h, LinLayout* L) {
    *L = LinLayout(h->nx, h->ny, h->nth, h->ki.G, h->ki.generic ? 0 : h->nths, h->ki.generic ? 0 : h->ki.adj);
    if (L->size != h->ki.tab_size) return fail(h, CIMPC_ERR_STATE, "table layout of the library and of the kernel differ");
    return CIMPC_OK;
}

void prof_begin(cimpc_ctx* h, int cls, hipStream_t st = nullptr) {
    h->prof_open = false;
    if (!h->prof_on || (h->prof_on == 2 && cls != PC_IP)) return;
    h->prof_open = true;
    if (!st) st = h->stream;
    ProfRec r;
    auto get = [&]() {
        if (!h->ev_pool.empty()) {
            hipEvent_t e = h->ev_pool.back();
            h->ev_pool.pop_back();
            return e;
        }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    };
    r.a = get();
    r.b = get();
    r.cls = cls;
    (void)hipEventRecord(r.a, st);
    h->prof_recs.push_back(r);
}
void prof_end(cimpc_ctx* h, hipStream_t st = nullptr) {
    if (!h->prof_on || !h->prof_open) return;
    h->prof_open = false;
    (void)hipEventRecord(h->prof_recs.back().b, st ? st : h->stream);
}
void prof_collect(cimpc_ctx* h) {
    if (h->prof_recs.empty()) return;
    (void)hipStreamSynchronize(h->stream);
    if (h->rs.st) (void)hipStreamSynchronize(h->rs.st);
    if (h->rs.st_kkt) (void)hipStreamSynchronize(h->rs.st_kkt);
    for (auto& r : h->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            h->prof_ms[r.cls] += ms;
            h->prof_n[r.cls] += 1;
        }
        h->ev_pool.push_back(r.a);
        h->ev_pool.push_back(r.b);
    }
    h->prof_recs.clear();
}

IpParams make_ip_params(cimpc_ctx* h, const TrajDev& T, int par, int* pending_counter, double* zout) {
    IpParams p{};
    p.tab = h->d_tab;
    p.Q = h->Q;
    p.Q.par = par;
    p.wpk = h->sched.wpk;
    p.q = T.q;
    p.theta = T.th;
    p.gam = T.g;
    p.bfr = T.b;
    p.alt = h->st.has_altitude() ? h->d_alt : nullptr;
    p.d = h->S.d;
    p.dz = h->S.dz;
    p.nu = nullptr; p.dtn = nullptr; p.dtn_ld = h->S.dtn_ld;      // (the Newton loop switches the products on, see cimpc_newton_solve_dev)
    p.status = h->S.ip_status;
    p.iters = h->S.ip_iters;
    p.zout = zout;
    p.pflag = h->S.pflag;
    p.pstate = h->d_pstate;
    p.pending_count = pending_counter;
    p.iter_cap = h->kn.sched.iter_cap;
    p.slots = CS;
    p.H = h->dm.H;
    p.o = h->ip;
    p.kc_floor = h->ip.kappa_tol / h->ip.undercut;
    p.tau_floor = 1.0 - h->ip.eps_min;
    p.reg_floor = h->ip.kappa_tol * h->ip.gamma_reg;
    p.budget_ticks = h->ip_budget_ticks;
    p.generic_static = h->kn.generic_static ? 1 : 0;
    return p;
}

// queue kernel + sensitivity kernel of one round
int run_sweep(cimpc_ctx* h, int par, int* pending_counter, double* zout, hipStream_t st, int iter_cap = 0, int* drain_counter = nullptr,
              bool with_products = false, long long hint = -1) {
    IpParams p = make_ip_params(h, h->S.cand, par, pending_counter, zout);
    if (with_products && h->S.dtn != nullptr) { p.nu = h->S.nu_cand; p.dtn = h->S.dtn; }
    if (iter_cap > 0) p.iter_cap = iter_cap;
    const SweepLaunch l = plan_sweep(h->kn.sched, h->sched, hint, p.iter_cap, h->ip.max_iter, drain_counter != nullptr);
    p.wpk = l.wpk; p.direct = l.direct;
    if (l.drain_thresh > 0) { p.drain_count = drain_counter; p.drain_thresh = l.drain_thresh; p.drain_min = h->kn.sched.drain_min; }
    prof_begin(h, PC_IP, st);
    int rc = launch_ip_sweep(&h->dm, p, l.waves, st);
    prof_end(h, st);
    if (rc != CIMPC_OK) return fail(h, rc, "ip sweep launch failed");
    return CIMPC_OK;
}

// KktCaps of the handle's problem, the backend they allow for the requested kkt_backend, and what follows from it
static void set_kkt_backend(cimpc_ctx* h) {
    NewtonDev& S = h->S;
    KktCaps& c = h->kc;
    c.cfg = h->dm.mode == CIMPC_MODE_CONFIGURATION;
    c.velocity = S.V != nullptr;
    c.cf_tiny = h->cf_tiny;
    c.wide_tiles = (h->dm.nq > 16 || h->dm.nu > 16) && h->dm.nq <= 24 && h->dm.nu <= 24;
    c.condensed = kkt_condensed_available(S);
    c.mfma = kkt_mfma_available(S);
    c.packed = kkt_packed_available(S);
    c.twisted = kkt_twisted_available(S);
    c.duo = kkt_duo_available(S);
    c.mixed = kkt_mixed_available(S);
    // Form of the banded LDL^T.  The reduced form (controls eliminated first) needs LDS for its pre-pass as well as the
    // window: where that does not fit (long horizons of wide models) the full interleaved form is tried, and the dense LU
    // serves what neither fits.  avail() = the availability test of whoever would run the banded kernel on S.
    auto pick_band_form = [&](auto avail) {
        for (int r = h->band_reduce_ok ? 1 : 0; r >= 0; --r) { S.band_reduce = r; if (avail()) return true; }
        S.band_reduce = h->band_reduce_ok ? 1 : 0;
        return false;
    };
    S.band_reduce = h->band_reduce_ok ? 1 : 0;
    c.banded = c.cfg && pick_band_form([&] { return kkt_banded_available(S); });
    c.cf_reduce = !c.cfg && (c.velocity ? pick_band_form([&] { return kkt_cf_reduce_available(S); }) : kkt_cf_reduce_available(S));
    c.banded_twisted = kkt_banded_twisted_available(c.cfg ? S : cf_shadow(S));
    h->kb = select_kkt_backend(c, h->nt.kkt_backend);
    S.good_src = kkt_lazy_commit(h->kp, c, h->kb) ? h->d_good_src : nullptr;
}

// workspaces of the handle's KKT backend, allocated on first use
int ensure_kkt_ws(cimpc_ctx* h) {
    if (h->kb == KktBackend::Condensed) return CIMPC_OK;
    if (h->kb == KktBackend::CondensedMixed) {
        if (h->d_mix_ws) return CIMPC_OK;
        if (dev_alloc(h, &h->d_mix_ws, kkt_mixed_workspace_doubles(h->S)) != CIMPC_OK) return CIMPC_ERR_HIP;
        return dev_alloc(h, &h->d_mix_nfb, 1);
    }
    const bool cf = h->kb == KktBackend::CfCondensed || h->kb == KktBackend::CfBanded;
    if (cf && !h->d_cf_ws && dev_alloc(h, &h->d_cf_ws, cf_reduce_doubles(h->S)) != CIMPC_OK) return CIMPC_ERR_HIP;
    if (h->kb == KktBackend::CfCondensed) return CIMPC_OK;            // reduced problem goes to the condensed MFMA solve
    const size_t need = cf ? kkt_dense_workspace_doubles(cf_shadow(h->S), true) : kkt_dense_workspace_doubles(h->S, h->kb == KktBackend::Banded);
    if (h->d_dense_ws && h->dense_ws_doubles >= need) return CIMPC_OK;
    h->d_dense_ws = nullptr;                      // (an earlier, smaller workspace stays in h->allocs until destroy)
    h->dense_ws_doubles = need;
    return dev_alloc(h, &h->d_dense_ws, need);
}

// the form of a KKT stage at `site`, counted: the only place n_kkt_twisted moves
static KktForm plan_kkt_stage(cimpc_ctx* h, const KktSite& site) {
    const KktForm f = choose_kkt_form(h->kp, h->kc, h->kb, site);
    if (two_ended(f)) h->n_kkt_twisted++;
    return f;
}
static int run_kkt_stage(cimpc_ctx* h, const NewtonDev& Sk, const KktArgs& K, const KktSite& site, const int* list, int n, const int* n_dev, hipStream_t st) {
    return launch_kkt_stage(Sk, K, h->kb, plan_kkt_stage(h, site), list, n, n_dev, KktWorkspace{h->d_dense_ws, h->d_cf_ws, h->d_mix_ws, h->d_mix_nfb}, st);
}

// statistics of the running / last solve: the per-rollout records of the decision stage, summed (NewtonDev::stats)
int read_stats(cimpc_ctx* h, long long out[4]) {
    std::vector<long long> v((size_t)h->dm.B * 4);
    HIP_TRY(h, hipMemcpy(v.data(), h->S.stats, v.size() * sizeof(long long), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = out[3] = 0;
    for (size_t b = 0; b < (size_t)h->dm.B; ++b)
        for (int k = 0; k < 4; ++k) out[k] += v[b * 4 + k];
    return CIMPC_OK;
}

// cimpc_mpc_advance returns with its copy / kernels still queued on h->stream (a private NON-blocking stream): every entry point that
// rewrites reference / gait / window / objective state with blocking NULL-stream copies must first let that work finish, or the
// pending gait_window / rekey kernels race with the rewrite
int drain_pending(cimpc_ctx* h) {
    if (!h->st.drain_needed()) return CIMPC_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->st.advance_drained();
    return CIMPC_OK;
}

int check_ready(cimpc_ctx* h, bool need_newton) {
    if (!h) return CIMPC_ERR_INVALID;
    return refuse(h, h->st.solve_refusal(h->n_knots_set == h->dm.H_ref, need_newton));
}

}  // namespace

extern "C" {

int cimpc_version(void) { return 108; }      // 1.08: + cimpc_tvlqr, cimpc_reference_gains(_lin), cimpc_set_gains, cimpc_gain_latch, cimpc_gain_feedback (no struct changed).  1.07: + cimpc_set_linearization_batch, cimpc_linearize_knots, cimpc_get_table (no struct changed).  1.06: round 6 (+ cimpc_mpc_solve; no struct changed).  1.05: round 5 (+ cimpc_get_kkt_twisted; no struct changed).  1.04: round 4 (cimpc_ip_opts::max_time - the struct grew by one double at its end)

void cimpc_default_ip_opts(cimpc_ip_opts* o) {
    if (!o) return;
    o->r_tol = 1.0e-8;
    o->kappa_tol = 2.0e-4;
    o->undercut = 5.0;
    o->gamma_reg = 0.1;
    o->kappa_reg = 1.0e-3;
    o->eps_min = 0.05;
    o->ls_scale = 0.5;
    o->max_iter = 100;
    o->max_ls = 3;
    o->stall_alpha = 1.0e-13;
    o->max_time = 0.0;       // unlimited (the reference's default, 1e5 s, is treated as unlimited too)
}

void cimpc_default_newton_opts(cimpc_newton_opts* o) {
    if (!o) return;
    o->r_tol = 3.0e-4;
    o->beta_init = 1.0e-5;
    o->max_time = 0.0;
    o->kappa = 2.0e-4;
    o->max_iter = 5;
    o->kkt_backend = CIMPC_KKT_CONDENSED;
}

const char* cimpc_last_error(cimpc_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int cimpc_create(const cimpc_dims* dims, const cimpc_ip_opts* ip, const cimpc_newton_opts* nt,
                 int device, cimpc_handle* out) {
    if (!dims || !out) return fail(nullptr, CIMPC_ERR_INVALID, "null argument");
    *out = nullptr;
    const cimpc_dims& d = *dims;
    if (d.nq <= 0 || d.nu < 0 || d.nw < 0 || d.nc <= 0 || d.nb < 0 || d.H <= 0 || d.H_ref <= 0 ||
        d.B <= 0 || (d.mode != 0 && d.mode != 1))
        return fail(nullptr, CIMPC_ERR_INVALID, "invalid dimensions");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, CIMPC_ERR_NO_DEVICE,
                    "no HIP device visible: this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, CIMPC_ERR_NO_DEVICE, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(nullptr, CIMPC_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, CIMPC_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, CIMPC_ERR_NO_DEVICE, "hipSetDevice failed");

    cimpc_ctx* h = new cimpc_ctx();
    h->dm = d;
    if (ip) h->ip = *ip; else cimpc_default_ip_opts(&h->ip);
    if (nt) h->nt = *nt; else cimpc_default_newton_opts(&h->nt);
    h->device = device;
    if (h->ip.max_time > 0.0 && h->ip.max_time < 1000.0) {      // per-solve budget of the interior point (policy.jl:9,61)
        if (h->ip.max_iter >= 128) { delete h; return fail(nullptr, CIMPC_ERR_INVALID, "ip max_time needs max_iter < 128 (the parked state packs both into one word)"); }
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
            delete h;      // no guessing: a budget in ticks of an unknown clock would silently be the wrong budget
            return fail(nullptr, CIMPC_ERR_HIP, "ip max_time: the device does not report hipDeviceAttributeWallClockRate");
        }
        h->ip_budget_ticks = std::max<long long>(1, (long long)std::llround(h->ip.max_time * 1.0e3 * (double)khz));
    }
    h->kn.read_environment();       // the only place the environment is consulted
    if (ip_kernel_info(&h->dm, &h->ki) != CIMPC_OK) {
        delete h;
        std::string built;
        for (const ModelRow& r : MODEL_TABLE) (built += built.empty() ? "" : ", ") += r.name;
        return fail(nullptr, CIMPC_ERR_INVALID, "model dimensions outside the runtime-dimension kernel (nx, ny <= 64) and without a compiled set (built: " + built + ")");
    }
    h->nx = d.nq;
    h->ny = 2 * d.nc + d.nb;
    h->nz = d.nq + 4 * d.nc + 2 * d.nb;
    h->nth = 2 * d.nq + d.nu + d.nw + 2;
    h->nths = 2 * d.nq + d.nu;
    h->nd = d.mode ? d.nq + d.nc + d.nb : d.nq;
    h->nr = d.mode ? d.nq + d.nu + d.nc + d.nb : d.nq + d.nu;
    h->N = d.H * (h->nr + h->nd);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(nullptr, CIMPC_ERR_HIP, "hipStreamCreate failed");
    }
    h->own_stream = true;
    h->knot_set.assign(d.H_ref, 0);
    h->h_tab.assign(h->ki.tab_size, 0.0);
    h->h_tab_work.assign(lin_table_work_doubles(h->nx, h->ny), 0.0);

    const size_t B = d.B, H = d.H;
    int rc = CIMPC_OK;
    {   // the handle's schedule (schedule_plan.h); the persistent kernel's queues are sized for every push of one solve: they never wrap
        const size_t K = d.H_ref;
        const size_t evals = 1 + 7 * (size_t)std::max(1, h->nt.max_iter);       // per rollout and solve
        h->a_cap = B * evals * ((H + K - 1) / K + 1);
        h->a_rq_cap = B * (2 + 3 * (size_t)std::max(1, h->nt.max_iter));
        h->a_kq_cap = B * (2 + 3 * (size_t)std::max(1, h->nt.max_iter));      // (twisted KKT jobs: two entries per stage, one more after a timed-out hand-over)
        const size_t bytes = (K * h->a_cap + h->a_rq_cap + h->a_kq_cap) * sizeof(int);
        h->sched = plan_schedule(h->kn.sched, ScheduleFacts{d.B, d.H, d.H_ref, h->ki.G, newton_async_available(&d) && K <= 256 && bytes <= ((size_t)1 << 30)});
    }
    auto A = [&](auto** p, size_t n) { if (rc == CIMPC_OK) rc = dev_alloc(h, p, n); };
    A(&h->d_tab, (size_t)d.H_ref * h->ki.tab_size);
    {   // work queues: a knot can appear ceil(H / H_ref) times in one window
        const size_t K = d.H_ref;
        const size_t cap = B * CS * ((H + K - 1) / K + 1);
        h->Q.K = (int)K; h->Q.cap = (int)cap; h->Q.par = 0;
        A(&h->Q.items, 2 * K * cap);
        // queue counters, queue heads and the round counters: ONE block, cleared by one memset at the start of a solve
        const QueueCtl L = queue_ctl(K);
        h->ctl_ints = L.ints;
        A(&h->Q.count, h->ctl_ints);
        if (rc == CIMPC_OK) { h->Q.head = h->Q.count + L.head; h->d_ring = h->Q.count + L.counters; }
        A(&h->Q.done_count, B * CS);
        A(&h->d_window, B * (H + 2));
        h->Q.window = h->d_window;
    }
    A(&h->d_alt, B * d.nc);
    A(&h->d_zout, B * CS * H * h->nz);
    A(&h->d_Q, H * d.nq * d.nq);
    A(&h->d_R, H * d.nu * d.nu);
    A(&h->d_Qinv, H * d.nq * d.nq);
    A(&h->d_Rinv, H * d.nu * d.nu);
    A(&h->d_Cg, H * d.nc * d.nc);
    A(&h->d_Cb, H * d.nb * d.nb);
    A(&h->d_V, H * d.nq * d.nq);
    A(&h->d_qt, H * d.nq);
    A(&h->d_vt, H * d.nq);
    A(&h->d_q0, 2 * B * d.nq);
    if (rc == CIMPC_OK) h->d_q1 = h->d_q0 + B * d.nq;
    A(&h->d_result, result_doubles(B, d.nu));
    if (rc == CIMPC_OK && (hipHostMalloc((void**)&h->h_qin, (2 * B + 1) * d.nq * sizeof(double), hipHostMallocDefault) != hipSuccess ||
                           hipHostMalloc((void**)&h->h_result, result_doubles(B, d.nu) * sizeof(double), hipHostMallocDefault) != hipSuccess))
        rc = CIMPC_ERR_HIP;
    A(&h->d_rhs, B * h->N);
    NewtonDev& S = h->S;
    S.dm = d;
    S.b0 = 0;
    S.nb_launch = d.B;
    S.nd = h->nd; S.nr = h->nr; S.nth = h->nth; S.nths = h->nths; S.N = h->N;
    const size_t BS = B * CS;     // evaluation slots (speculative line search)
    for (TrajDev* T : {&S.traj, &S.cand, &S.ref}) {
        const size_t n = (T == &S.cand) ? BS : B;      // (S.ref: read-only during a solve)
        A(&T->q, n * (H + 2) * d.nq); A(&T->u, n * H * d.nu); A(&T->w, n * H * d.nw);
        A(&T->g, n * H * d.nc); A(&T->b, n * H * d.nb); A(&T->th, n * H * h->nth);
    }
    A(&S.nu, B * H * h->nd); A(&S.nu_cand, BS * H * h->nd); A(&S.d, BS * H * h->nd);
    A(&S.dz, BS * H * h->nths * h->nd); A(&S.dz_good, B * H * h->nths * h->nd); A(&h->d_good_src, B * H);
    S.dtn_ld = h->ki.generic ? 0 : h->ki.dtn_ld;
    if (S.dtn_ld > 0) A(&S.dtn, BS * H * (size_t)S.dtn_ld);
    A(&S.ip_status, BS * H); A(&S.ip_iters, BS * H); A(&S.pflag, BS * H); A(&S.cur_slot, B);
    A(&h->d_pstate, BS * H * (2 * (size_t)h->nx + 4 * (size_t)h->ny + 4));
    A(&S.res, B * h->N); A(&S.res_cand, BS * h->N); A(&S.delta, B * h->N);
    A(&S.r_norm, B); A(&S.r_cand, BS); A(&S.alpha, B); A(&S.beta, B);
    A(&S.ls_iter, B); A(&S.newton_l, B); A(&S.stage, B); A(&S.need_sweep, BS);
    A(&S.kkt_list, 2 * B);
    A(&S.slot_list, 2 * BS);
    A(&S.counters, ROUND_COUNTER_INTS);
    A(&S.stats, std::max<size_t>(B * 4, 64));      // (>= 32 entries: diagnostic builds with -DCIMPC_KKT_PROF park their phase clocks at [8..23])
    A(&S.ro_sweeps, B); A(&S.ro_ip_iters, B); A(&S.ro_ip_fail, B); A(&S.nlog, B * NLOG * 4);
    A(&S.kkt_ws, B * H * (3 * (size_t)h->nd * h->nd + h->nd));
    A(&S.kkt_tw_xch, B * kkt_tw_xch_doubles(h->nd));
    A(&S.kkt_tw_flags, B * KKT_TW_FLAGS);
    if (rc == CIMPC_OK && hipHostMalloc((void**)&h->h_counters, ROUND_COUNTER_INTS * sizeof(int)) != hipSuccess)
        rc = fail(h, CIMPC_ERR_HIP, "hipHostMalloc failed");
    if (rc != CIMPC_OK) {
        g_create_error = h->err;
        cimpc_destroy(h);
        return rc;
    }
    S.Q = h->d_Q; S.R = h->d_R; S.Qinv = h->d_Qinv; S.Rinv = h->d_Rinv; S.Cg = h->d_Cg; S.Cb = h->d_Cb;
    if (hipMemset(h->d_good_src, 0xFF, B * H * sizeof(int)) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {      // -1: every block is in dz_good
        g_create_error = "hipMemset failed"; cimpc_destroy(h); return CIMPC_ERR_HIP;
    }
    S.band_form = h->kn.banded_form;
    S.r_tol = h->nt.r_tol; S.beta_init = h->nt.beta_init; S.kappa = h->nt.kappa; S.max_iter = h->nt.max_iter;
    h->kp = h->kn.kkt;
    h->kp.kkt_overlap = h->sched.kkt_overlap;
    set_kkt_backend(h);
    S.spec_all = h->sched.spec_all; S.spec_first = h->sched.spec_first; S.spec_mid = h->sched.spec_mid;
    S.kkt_tw_nb = h->kn.kkt_tw_nb;
    S.kkt_tw_epoch = 0;
    S.kkt_tw_spins = h->kn.kkt_tw_spins > 0 ? h->kn.kkt_tw_spins : KKT_TW_SPINS;
    {
        int* dv = nullptr;
        if (hipHostMalloc((void**)&h->h_twfail, 4 * sizeof(int), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&dv, h->h_twfail, 0) != hipSuccess) {
            g_create_error = "mapped counter allocation failed"; cimpc_destroy(h); return CIMPC_ERR_HIP;
        }
        h->h_twfail[0] = 0;
        S.kkt_tw_fail = dv;
    }
    if (hipHostMalloc((void**)&h->h_ring, RING_ALLOC_INTS * sizeof(int), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->h_ring_dev, h->h_ring, 0) != hipSuccess) {
        g_create_error = "ring allocation failed"; cimpc_destroy(h); return CIMPC_ERR_HIP;
    }
    if (h->sched.async_on) {
        const size_t K = d.H_ref;
        if (dev_alloc(h, &h->a_items, K * h->a_cap) != CIMPC_OK || dev_alloc(h, &h->a_jobs, h->a_rq_cap + h->a_kq_cap) != CIMPC_OK ||
            dev_alloc(h, &h->a_ctrl, async_ctl(K).ints) != CIMPC_OK || dev_alloc(h, &h->a_evals, B) != CIMPC_OK) {
            g_create_error = h->err; cimpc_destroy(h); return CIMPC_ERR_HIP;
        }
        if (h->kn.async_debug && dev_alloc(h, &h->a_dbg, 16) != CIMPC_OK) { g_create_error = h->err; cimpc_destroy(h); return CIMPC_ERR_HIP; }
        h->async_dirty = true;
    }
    {   // streams of the rounds (one batch: sub-batch streams were measured and only multiply the per-launch
        // latency floor - 4 sub-batches 34.8 ms/step vs 28.2 ms single batch at B = 512)
        RoundStreams& r = h->rs;
        if (hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&r.st_kkt, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&r.ev_join, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&r.ev_start, hipEventDisableTiming) != hipSuccess) {
            g_create_error = "stream creation failed"; cimpc_destroy(h); return CIMPC_ERR_HIP;
        }
    }
    *out = h;
    return CIMPC_OK;
}

int cimpc_destroy(cimpc_handle h) {
    if (!h) return CIMPC_ERR_INVALID;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& r : h->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : h->ev_pool) (void)hipEventDestroy(e);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->d_tb) (void)hipFree(h->d_tb);
    if (h->h_counters) (void)hipHostFree(h->h_counters);
    if (h->h_ring) (void)hipHostFree(h->h_ring);
    if (h->h_qin) (void)hipHostFree(h->h_qin);
    if (h->h_result) (void)hipHostFree(h->h_result);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_twfail) (void)hipHostFree(h->h_twfail);
    {
        RoundStreams& r = h->rs;
        if (r.st) { (void)hipStreamSynchronize(r.st); (void)hipStreamDestroy(r.st); }
        if (r.st_kkt) { (void)hipStreamSynchronize(r.st_kkt); (void)hipStreamDestroy(r.st_kkt); }
        if (r.ev_join) (void)hipEventDestroy(r.ev_join);
        if (r.ev_start) (void)hipEventDestroy(r.ev_start);
    }
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CIMPC_OK;
}

int cimpc_set_stream(cimpc_handle h, void* hip_stream) {
    if (!h) return CIMPC_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    h->st.advance_drained();
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = static_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
    h->external_stream = true;   // caller-ordered stream: the solve runs as ONE batch on it
    return CIMPC_OK;
}

int cimpc_synchronize(cimpc_handle h) {
    if (!h) return CIMPC_ERR_INVALID;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CIMPC_OK;
}

int cimpc_set_linearization(cimpc_handle h, int t, const double* z0, const double* th0,
                            const double* r0, const double* rz0, const double* rth0) {
    if (!h || !z0 || !th0 || !r0 || !rz0 || !rth0) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (t < 1 || t > h->dm.H_ref) return fail(h, CIMPC_ERR_INVALID, "knot index out of range (1-based)");
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    LinLayout L(0, 0, 0, 0);
    if (int rc = table_layout(h, &L); rc != CIMPC_OK) return rc;
    // the build the device runs (lin_table_build.h), here by a team of one
    if (!lin_table_build_knot(L, z0, th0, r0, rz0, rth0, h->h_tab_work.data(), h->h_tab.data(), SoloTeam{}))
        return fail(h, CIMPC_ERR_INVALID, "Dx = rz0[idyn, ix] is singular");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(h->d_tab + (size_t)(t - 1) * L.size, h->h_tab.data(), (size_t)L.size * sizeof(double),
                         hipMemcpyHostToDevice));
    if (!h->knot_set[t - 1]) { h->knot_set[t - 1] = 1; h->n_knots_set++; }
    return CIMPC_OK;
}

namespace {

// The device table build behind cimpc_set_linearization_batch (model < 0: r0, rz0, rth0 come from the host) and
// cimpc_linearize_knots (model >= 0: they are linearized on the device from z0, th0): one upload, the kernels on the handle's stream,
// N status words back, then - only if no knot was refused - one device-to-device copy into the handle's tables.
int build_tables_on_device(cimpc_ctx* h, int t0, int N, const double* z0, const double* th0, const double* r0, const double* rz0,
                           const double* rth0, int model, int n_ter_up, int n_terrain, const cimpc_terrain* terrain, double kappa) {
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    const size_t nz = h->nz, nth = h->nth;
    LinLayout L(0, 0, 0, 0);
    if (int rc = table_layout(h, &L); rc != CIMPC_OK) return rc;
    constexpr size_t TW = sizeof(cimpc_terrain) / sizeof(double);
    const size_t n_z = (size_t)N * nz, n_th = (size_t)N * nth, n_ter = (size_t)n_ter_up * TW;
    const size_t o_th = n_z, o_ter = o_th + n_th, o_r = o_ter + n_ter, o_rz = o_r + n_z, o_rth = o_rz + n_z * nz;
    const size_t o_tab = o_rth + n_z * nth, o_st = o_tab + (size_t)N * L.size, total = o_st + ((size_t)N + 1) / 2;
    const size_t n_up = model >= 0 ? o_r : o_tab;                  // what goes up: the inputs alone, or the triple too
    std::vector<double> up(n_up);
    std::memcpy(up.data(), z0, n_z * sizeof(double));
    std::memcpy(up.data() + o_th, th0, n_th * sizeof(double));
    if (n_ter) std::memcpy(up.data() + o_ter, terrain, n_ter * sizeof(double));
    if (model < 0) {
        std::memcpy(up.data() + o_r, r0, n_z * sizeof(double));
        std::memcpy(up.data() + o_rz, rz0, n_z * nz * sizeof(double));
        std::memcpy(up.data() + o_rth, rth0, n_z * nth * sizeof(double));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->tb_cap < total) {
        if (h->d_tb) (void)hipFree(h->d_tb);
        h->d_tb = nullptr; h->tb_cap = 0;
        HIP_TRY(h, hipMalloc((void**)&h->d_tb, total * sizeof(double)));
        h->tb_cap = total;
    }
    double* D = h->d_tb;
    int* d_status = reinterpret_cast<int*>(D + o_st);
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(D, up.data(), n_up * sizeof(double), hipMemcpyHostToDevice, st));
    bool launched = true;
    if (model >= 0)
        launched = plant_linearize_launch(model, N, D, D + o_th, n_ter ? reinterpret_cast<const cimpc_terrain*>(D + o_ter) : nullptr, n_terrain,
                                          kappa, D + o_r, D + o_rz, D + o_rth, st);
    launched = launched && lin_table_build_launch(L, N, D, D + o_th, D + o_r, D + o_rz, D + o_rth, D + o_tab, d_status, st);
    if (!launched) {
        (void)hipStreamSynchronize(st);
        return fail(h, CIMPC_ERR_HIP, "the table build could not be launched");
    }
    std::vector<int> status(N);
    HIP_TRY(h, hipMemcpyAsync(status.data(), d_status, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    for (int k = 0; k < N; ++k)
        if (status[k] != 0) return fail(h, CIMPC_ERR_INVALID, "Dx = rz0[idyn, ix] is singular at knot " + std::to_string(t0 + k) + "; no knot was changed");
    HIP_TRY(h, hipMemcpyAsync(h->d_tab + (size_t)(t0 - 1) * L.size, D + o_tab, (size_t)N * L.size * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    for (int t = t0; t < t0 + N; ++t)
        if (!h->knot_set[t - 1]) { h->knot_set[t - 1] = 1; h->n_knots_set++; }
    return CIMPC_OK;
}

}  // namespace

int cimpc_set_linearization_batch(cimpc_handle h, int t0, int N, const double* z0, const double* th0,
                                  const double* r0, const double* rz0, const double* rth0) {
    if (!h || !z0 || !th0 || !r0 || !rz0 || !rth0) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (t0 < 1 || N < 1 || N > h->dm.H_ref || t0 - 1 > h->dm.H_ref - N) return fail(h, CIMPC_ERR_INVALID, "knot range out of the table (1-based)");
    return build_tables_on_device(h, t0, N, z0, th0, r0, rz0, rth0, -1, 0, 0, nullptr, 0.0);
}

int cimpc_linearize_knots(cimpc_handle h, int model, int t0, int N, int n_terrain, const cimpc_terrain* terrain,
                          const double* z, const double* theta, double kappa) {
    if (!h || !z || !theta) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (t0 < 1 || N < 1 || N > h->dm.H_ref || t0 - 1 > h->dm.H_ref - N) return fail(h, CIMPC_ERR_INVALID, "knot range out of the table (1-based)");
    PlantLinearizeDims pd{};
    if (plant_linearize_check(model, N, n_terrain, terrain, z, theta, kappa, &pd) != CIMPC_OK)
        return fail(h, CIMPC_ERR_INVALID, "cimpc_plant_linearize would refuse these arguments");
    const cimpc_dims& d = h->dm;
    if (pd.nq != d.nq || pd.nu != d.nu || pd.nw != d.nw || pd.nc != d.nc || pd.nb != d.nb)
        return fail(h, CIMPC_ERR_INVALID, "the plant model's (nq, nu, nw, nc, nb) are not the handle's");
    return build_tables_on_device(h, t0, N, z, theta, nullptr, nullptr, nullptr, model, pd.n_terrain_up, n_terrain, terrain, kappa);
}

int cimpc_get_table(cimpc_handle h, int t, double* table) {
    if (!h || !table) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (t < 1 || t > h->dm.H_ref) return fail(h, CIMPC_ERR_INVALID, "knot index out of range (1-based)");
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    LinLayout L(0, 0, 0, 0);
    if (int rc = table_layout(h, &L); rc != CIMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(table, h->d_tab + (size_t)(t - 1) * L.size, (size_t)L.size * sizeof(double), hipMemcpyDeviceToHost));
    return CIMPC_OK;
}

int cimpc_set_objective(cimpc_handle h, const double* Q, const double* R, const double* Cg,
                        const double* Cb, const double* V, const double* q_target,
                        const double* v_target) {
    if (!h || !Q || !R) return fail(h, CIMPC_ERR_INVALID, "Q and R are required");
    const cimpc_dims& d = h->dm;
    const size_t H = d.H;
    {   // the weights are symmetric in the reference (objective.jl: Diagonal or relative_state_cost) and every backend but the dense
        // LU relies on it (Qinv / Rinv as symmetric operands of the condensed solve, a symmetric banded matrix): refuse, don't guess
        auto symmetric = [&](const double* A, int n) {
            for (size_t t = 0; t < H; ++t) {
                const double* M = A + t * n * n;
                double amax = 0.0, asym = 0.0;
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) { amax = std::max(amax, std::fabs(M[i + j * n])); asym = std::max(asym, std::fabs(M[i + j * n] - M[j + i * n])); }
                if (asym > 1e-9 * amax) return false;
            }
            return true;
        };
        // (the reference-default backend - dense jacobian! + LU, on request - takes the blocks as they are, like the reference)
        const bool lu = h->nt.kkt_backend == CIMPC_KKT_DENSE_LU;
        if (!lu && !symmetric(Q, d.nq)) return fail(h, CIMPC_ERR_INVALID, "objective block Q[i] is not symmetric");
        if (!lu && d.nu > 0 && !symmetric(R, d.nu)) return fail(h, CIMPC_ERR_INVALID, "objective block R[i] is not symmetric");
        if (!lu && V && !symmetric(V, d.nq)) return fail(h, CIMPC_ERR_INVALID, "objective block V[i] is not symmetric");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    {   // contact-impulse weights below fp64 resolution (1e-100 in every example of the reference): the cf-mode KKT
        // system reduces exactly onto the :configuration solvers (newton_kernels.hip: cf_reduce_*)
        double gmax = 0.0;
        if (Cg) for (size_t k = 0; k < H * d.nc * d.nc; ++k) gmax = std::max(gmax, std::fabs(Cg[k]));
        if (Cb) for (size_t k = 0; k < H * d.nb * d.nb; ++k) gmax = std::max(gmax, std::fabs(Cb[k]));
        h->cf_tiny = gmax <= 1e-30;
    }
    if (V != nullptr) {      // TrackingVelocityObjective (objective.jl:18-47): q_target integrates v_target when not given
        std::vector<double> vt(H * d.nq, 0.0), qt(H * d.nq, 0.0);
        if (v_target) std::copy(v_target, v_target + H * d.nq, vt.begin());
        if (q_target) std::copy(q_target, q_target + H * d.nq, qt.begin());
        else {
            bool any = false;
            for (double x : vt) any = any || x != 0.0;
            if (any) for (size_t t = 1; t < H; ++t) for (int k = 0; k < d.nq; ++k) qt[t * d.nq + k] = qt[(t - 1) * d.nq + k] + vt[(t - 1) * d.nq + k];
        }
        HIP_TRY(h, hipMemcpy(h->d_V, V, H * d.nq * d.nq * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_qt, qt.data(), qt.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_vt, vt.data(), vt.size() * sizeof(double), hipMemcpyHostToDevice));
        h->S.V = h->d_V; h->S.q_target = h->d_qt; h->S.v_target = h->d_vt;      // P is block tridiagonal: banded LDL^T / dense LU
    } else {
        h->S.V = nullptr; h->S.q_target = nullptr; h->S.v_target = nullptr;
    }
    // the inverses first: whether every R_t could be inverted decides the form of the banded LDL^T (kkt_dense.hip:
    // kkt_banded_kernel eliminates the controls when it can), and that form decides whether the backend fits
    std::vector<double> Qi(H * d.nq * d.nq), Ri(H * d.nu * d.nu), work(lin_invert_work_doubles(std::max(d.nq, d.nu)));
    auto inverse = [&](const double* A, double* Ai, int n) {      // column-major n x n; false (Ai as it was) if singular
        if (!lin_invert(A, n, n, work.data(), SoloTeam{})) return false;
        for (int c = 0; c < n; ++c)
            for (int r = 0; r < n; ++r) Ai[r + (size_t)c * n] = work[(size_t)r * 2 * n + n + c];
        return true;
    };
    bool q_inverted = true, r_inverted = true;
    for (size_t i = 0; i < H; ++i) {
        if (!inverse(Q + i * d.nq * d.nq, Qi.data() + i * d.nq * d.nq, d.nq)) q_inverted = false;
        if (d.nu > 0 && !inverse(R + i * d.nu * d.nu, Ri.data() + i * d.nu * d.nu, d.nu)) r_inverted = false;
    }
    h->band_reduce_ok = r_inverted && d.nu > 0 && (h->kn.banded_form & 4) == 0;
    set_kkt_backend(h);
    // (the inverses feed the condensed solve - also behind the cf-mode reduction - and the control elimination of the banded LDL^T)
    const bool need_inv = h->kb == KktBackend::Condensed || h->kb == KktBackend::CondensedMixed || h->kb == KktBackend::CfCondensed;
    // (a refused objective leaves NO objective: the backend selection above is already committed while the device blocks still hold
    //  the previous call's - ADVICE r05 - so the handle goes back to "set_objective has not been called" instead of solving a mix)
    if (need_inv && !q_inverted) { h->st.objective_refused(); return fail(h, CIMPC_ERR_INVALID, "objective block Q[i] is singular"); }
    if (need_inv && !r_inverted) { h->st.objective_refused(); return fail(h, CIMPC_ERR_INVALID, "objective block R[i] is singular"); }
    HIP_TRY(h, hipMemcpy(h->d_Q, Q, H * d.nq * d.nq * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_R, R, H * d.nu * d.nu * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_Qinv, Qi.data(), Qi.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_Rinv, Ri.data(), Ri.size() * sizeof(double), hipMemcpyHostToDevice));
    if (Cg) HIP_TRY(h, hipMemcpy(h->d_Cg, Cg, H * d.nc * d.nc * sizeof(double), hipMemcpyHostToDevice));
    if (Cb) HIP_TRY(h, hipMemcpy(h->d_Cb, Cb, H * d.nb * d.nb * sizeof(double), hipMemcpyHostToDevice));
    h->st.objective_replaced();
    return CIMPC_OK;
}

int cimpc_set_altitude(cimpc_handle h, const double* alt) {
    if (!h) return CIMPC_ERR_INVALID;
    if (!alt) { h->st.altitude_cleared(); return CIMPC_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    HIP_TRY(h, hipMemcpy(h->d_alt, alt, (size_t)h->dm.B * h->dm.nc * sizeof(double), hipMemcpyHostToDevice));
    h->st.altitude_set();
    return CIMPC_OK;
}

// The sensitivity memory of failed solves belongs to the reference KNOTS (newton_kernels.hip: dz_rekey_kernel).  Called around
// every change of the window: rekey_out with the window still in force, rekey_in with the new one.
// One logical store for both seams.  The reference keeps ONE ip[t].dz per knot that implicit_dynamics! (B3) and the
// evaluations inside newton_solve! (B4) both write; on the device B4 keeps the accepted evaluation in dz_good and B3 writes
// slot 0 of S.dz.  When the producer changes between two calls on one handle, the blocks of the previous producer are copied
// into the store the next call reads / falls back to, so a solve that fails there keeps what the reference would keep.
static int sync_dz_stores(cimpc_ctx* h, int next_producer) {
    if (!h->st.dz_sync_needed(next_producer)) return CIMPC_OK;
    const size_t row = (size_t)h->dm.H * h->nths * h->nd * sizeof(double), B = h->dm.B;
    if (next_producer == DZ_IMPLICIT)      // newton_solve ran last: dz_good -> slot 0 of every rollout
        HIP_TRY(h, hipMemcpy2DAsync(h->S.dz, CS * row, h->S.dz_good, row, row, B, hipMemcpyDeviceToDevice, h->stream));
    else                         // implicit_dynamics ran last: slot 0 -> dz_good
        HIP_TRY(h, hipMemcpy2DAsync(h->S.dz_good, row, h->S.dz, CS * row, row, B, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CIMPC_OK;
}

static int rekey_out(cimpc_ctx* h) {
    if (!h->st.rekey_out_needed()) return CIMPC_OK;
    if (!h->d_dz_knot && dev_alloc(h, &h->d_dz_knot, (size_t)h->dm.B * h->dm.H_ref * h->nths * h->nd) != CIMPC_OK) return CIMPC_ERR_HIP;
    int rc = launch_dz_rekey(h->S, h->d_dz_knot, h->d_window, h->st.rekey_out_store(), 0, h->stream);
    return rc == CIMPC_OK ? CIMPC_OK : fail(h, rc, "sensitivity archive launch failed");
}
static int rekey_in(cimpc_ctx* h) {
    if (!h->st.rekey_in_needed(h->d_dz_knot != nullptr)) return CIMPC_OK;
    for (int which = 0; which < 2; ++which) {      // both consumers see the knots' blocks
        int rc = launch_dz_rekey(h->S, h->d_dz_knot, h->d_window, which, 1, h->stream);
        if (rc != CIMPC_OK) return fail(h, rc, "sensitivity restore launch failed");
    }
    return CIMPC_OK;
}

// a step of a window move that the host waits for: the step's own failure first, else the stream's
static int then_sync(cimpc_ctx* h, int rc) {
    if (rc != CIMPC_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CIMPC_OK;
}

int cimpc_set_window(cimpc_handle h, const int* window) {
    if (!h || !window) return fail(h, CIMPC_ERR_INVALID, "null argument");
    h->st.unlatch();
    std::vector<int> w0(horizon_sizes(h->dm, h->nth, h->nd).win);      // the device buckets problems by 0-based knot (newton_kernels.hip: enqueue_eval)
    if (int rc = refuse(h, window_to_knots(window, w0.size(), h->dm.H_ref, w0.data())); rc != CIMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    return window_move(h->st, WindowHome::Host, w0.data(), w0.size(),
        [&] { return then_sync(h, rekey_out(h)); },
        [&]() -> int { HIP_TRY(h, hipMemcpy(h->d_window, w0.data(), w0.size() * sizeof(int), hipMemcpyHostToDevice)); return CIMPC_OK; },
        [&] { return then_sync(h, rekey_in(h)); });
}

int cimpc_set_reference(cimpc_handle h, const double* q_ref, const double* u_ref,
                        const double* w_ref, const double* gamma_ref, const double* b_ref,
                        const double* theta_ref) {
    if (!h || !q_ref || !u_ref || !theta_ref) return fail(h, CIMPC_ERR_INVALID, "q_ref, u_ref, theta_ref are required");
    h->st.unlatch();
    const HorizonSizes n = horizon_sizes(h->dm, h->nth, h->nd);
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    HIP_TRY(h, hipMemcpy(h->S.ref.q, q_ref, n.q * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->S.ref.u, u_ref, n.u * sizeof(double), hipMemcpyHostToDevice));
    if (w_ref) HIP_TRY(h, hipMemcpy(h->S.ref.w, w_ref, n.w * sizeof(double), hipMemcpyHostToDevice));
    else {      // NULL-stream fill: make it complete before the (non-blocking) solver streams can read it
        HIP_TRY(h, hipMemset(h->S.ref.w, 0, n.w * sizeof(double)));
        HIP_TRY(h, hipStreamSynchronize(nullptr));
    }
    if (gamma_ref) HIP_TRY(h, hipMemcpy(h->S.ref.g, gamma_ref, n.g * sizeof(double), hipMemcpyHostToDevice));
    if (b_ref) HIP_TRY(h, hipMemcpy(h->S.ref.b, b_ref, n.b * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->S.ref.th, theta_ref, n.th * sizeof(double), hipMemcpyHostToDevice));
    h->st.reference_replaced();
    return CIMPC_OK;
}

int cimpc_implicit_dynamics(cimpc_handle h, const double* q, const double* theta,
                            const double* gamma, const double* b, double* d_out, double* dz,
                            int* status, int* iters, double* z) {
    int rc = check_ready(h, false);
    if (rc != CIMPC_OK) return rc;
    if (!q || !theta) return fail(h, CIMPC_ERR_INVALID, "q and theta are required");
    const cimpc_dims& d = h->dm;
    const size_t B = d.B, H = d.H;
    const HorizonSizes row = horizon_rows(d, h->nth, h->nd);      // of one rollout
    if (d.mode == CIMPC_MODE_CONFIGURATIONFORCE && (!gamma || !b))
        return fail(h, CIMPC_ERR_INVALID, "gamma and b are required in configurationforce mode");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int sy = sync_dz_stores(h, DZ_IMPLICIT); sy != CIMPC_OK) return sy;
    h->st.implicit_dynamics_started();
    TrajDev& T = h->S.cand;
    // evaluation slot 0 of every rollout (slot stride = CS rows)
    auto up = [&](double* dst, const double* src, size_t row_doubles) {
        return hipMemcpy2DAsync(dst, CS * row_doubles * sizeof(double), src, row_doubles * sizeof(double),
                                row_doubles * sizeof(double), B, hipMemcpyHostToDevice, h->stream);
    };
    HIP_TRY(h, up(T.q, q, row.q));
    HIP_TRY(h, up(T.th, theta, row.th));
    if (gamma) HIP_TRY(h, up(T.g, gamma, row.g));
    if (b) HIP_TRY(h, up(T.b, b, row.b));
    // queue slot 0 of every rollout, then run rounds until no solve is parked
    HIP_TRY(h, hipMemsetAsync(h->Q.count, 0, 2 * h->Q.K * QPAD * sizeof(int), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->Q.head, 0, h->Q.K * QPAD * sizeof(int), h->stream));
    {
        NewtonDev Sk = h->S;
        Sk.WQ = h->Q; Sk.WQ.par = 0;
        rc = launch_enqueue_all(Sk, h->stream);
        if (rc != CIMPC_OK) return fail(h, rc, "enqueue launch failed");
    }
    for (int pass = 0; pass < 64; ++pass) {
        const int par = pass & 1;
        HIP_TRY(h, hipMemsetAsync(h->S.counters, 0, ROUND_COUNTER_INTS * sizeof(int), h->stream));
        rc = run_sweep(h, par, round_counter(h->S.counters, RC_PARKED), z ? h->d_zout : nullptr, h->stream);
        if (rc != CIMPC_OK) return rc;
        HIP_TRY(h, hipMemsetAsync(h->Q.count + (size_t)par * h->Q.K * QPAD, 0, h->Q.K * QPAD * sizeof(int), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->Q.head, 0, h->Q.K * QPAD * sizeof(int), h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->h_counters, round_counter(h->S.counters, RC_PARKED), sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (*h->h_counters == 0) break;      // no solve was parked
    }
    auto down = [&](void* dst, const void* src, size_t row_bytes) {
        return hipMemcpy2DAsync(dst, row_bytes, src, CS * row_bytes, row_bytes, B, hipMemcpyDeviceToHost, h->stream);
    };
    if (d_out) HIP_TRY(h, down(d_out, h->S.d, row.nu * sizeof(double)));
    if (dz) HIP_TRY(h, down(dz, h->S.dz, H * h->nths * h->nd * sizeof(double)));
    if (status) HIP_TRY(h, down(status, h->S.ip_status, H * sizeof(int)));
    if (iters) HIP_TRY(h, down(iters, h->S.ip_iters, H * sizeof(int)));
    if (z) HIP_TRY(h, down(z, h->d_zout, H * h->nz * sizeof(double)));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CIMPC_OK;
}

// B2 seam: one reference-side callback on n points of knot t (ip_kernel_impl.h: ip_callback_kernel)
static int run_ip_callback(cimpc_handle h, int t, int n, int op, const double* z, const double* theta, const double* alt,
                           const double* r, double kappa, double reg, double* out) {
    if (!h || !z || !out || n <= 0) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (t < 1 || t > h->dm.H_ref) return fail(h, CIMPC_ERR_INVALID, "knot index out of range (1-based)");
    if (!h->knot_set[t - 1]) return fail(h, CIMPC_ERR_STATE, "set_linearization has not been called for this knot");
    if (h->ki.generic) return fail(h, CIMPC_ERR_INVALID, "B2 callbacks exist for the compiled lane-group models only");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nz = h->nz, nth = h->nth, nc = h->dm.nc;
    const size_t naux = std::max(nz, nth);               // theta (op 0) or r (op 1)
    const size_t tot = (size_t)n * (2 * nz + naux + nc);
    double* buf = nullptr;
    HIP_TRY(h, hipMalloc((void**)&buf, tot * sizeof(double)));
    double* d_z = buf; double* d_out = buf + (size_t)n * nz; double* d_aux = d_out + (size_t)n * nz; double* d_alt = d_aux + (size_t)n * naux;
    auto done = [&](int rc) { (void)hipFree(buf); return rc; };
    if (hipMemcpy(d_z, z, (size_t)n * nz * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return done(fail(h, CIMPC_ERR_HIP, "upload failed"));
    const double* aux = op == 0 ? theta : r;
    if (!aux) return done(fail(h, CIMPC_ERR_INVALID, "null argument"));
    if (hipMemcpy(d_aux, aux, (size_t)n * (op == 0 ? nth : nz) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return done(fail(h, CIMPC_ERR_HIP, "upload failed"));
    if (alt && hipMemcpy(d_alt, alt, (size_t)n * nc * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return done(fail(h, CIMPC_ERR_HIP, "upload failed"));
    IpCallbackArgs a{};
    a.tab = h->d_tab; a.knot = t - 1; a.n = n; a.op = op; a.z = d_z;
    a.theta = op == 0 ? d_aux : nullptr; a.alt = (op == 0 && alt) ? d_alt : nullptr; a.r = op == 1 ? d_aux : nullptr;
    a.kappa = kappa; a.reg = reg; a.out = d_out;
    (void)hipGetLastError();                             // (a stale error of an earlier call must not be read as this launch's)
    const int rc = launch_ip_callback(&h->dm, a, h->stream);
    if (rc != CIMPC_OK) return done(fail(h, rc, "callback launch failed"));
    if (hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemcpy(out, d_out, (size_t)n * nz * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return done(fail(h, CIMPC_ERR_HIP, "callback kernel failed"));
    return done(CIMPC_OK);
}

int cimpc_ip_residual(cimpc_handle h, int t, int n, const double* z, const double* theta, const double* alt, double kappa, double* r) {
    return run_ip_callback(h, t, n, 0, z, theta, alt, nullptr, kappa, 0.0, r);
}

int cimpc_ip_linear_solve(cimpc_handle h, int t, int n, const double* z, const double* r, double reg, double* delta) {
    return run_ip_callback(h, t, n, 1, z, nullptr, nullptr, r, 0.0, reg, delta);
}

int cimpc_kkt_solve(cimpc_handle h, const double* r, double beta, double* delta) {
    int rc = check_ready(h, true);
    if (rc != CIMPC_OK) return rc;
    if (!r || !delta) return fail(h, CIMPC_ERR_INVALID, "null argument");
    const size_t n = (size_t)h->dm.B * h->N;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->d_rhs, r, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = ensure_kkt_ws(h)) != CIMPC_OK) return rc;
    // attempt 0 may take a twisted kernel (two chains per rollout with bounded hand-over waits); if one of them timed out - the
    // mapped counter moved - the numbers are poisoned and the solve is repeated ONCE on the one-ended kernels (round 6)
    for (int attempt = 0; attempt < 2; ++attempt) {
        h->S.kkt_tw_epoch += 1;
        const int fails0 = *(volatile int*)h->h_twfail;
        prof_begin(h, PC_KKT);
        rc = run_kkt_stage(h, h->S, kkt_raw_args(h->d_rhs, beta, h->S.delta), KktSite{.kind = KktSite::Seam, .attempt = attempt, .B = h->dm.B},
                           nullptr, h->S.nb_launch, nullptr, h->stream);
        prof_end(h);
        if (rc != CIMPC_OK) return fail(h, rc, "kkt launch failed");
        HIP_TRY(h, hipMemcpyAsync(delta, h->S.delta, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const int fails1 = *(volatile int*)h->h_twfail;
        if (fails1 == fails0) break;
        h->n_kkt_tw_fallbacks += fails1 - fails0;
        h->twfail_seen = fails1;
    }
    return CIMPC_OK;
}

int cimpc_kkt_solve_rho(cimpc_handle h, const double* r, double rho, double* delta) {
    if (!h) return CIMPC_ERR_INVALID;
    if (!(rho >= 0.0) || !(h->nt.kappa > 0.0)) return fail(h, CIMPC_ERR_INVALID, "rho must be >= 0 (and kappa > 0)");
    // the kernels form rho = H * beta * kappa (newton_jacobian.jl:169-186): hand them the beta that reproduces rho
    const double Hk = (double)h->dm.H, kap = h->nt.kappa;
    auto f = [&](double b) { return Hk * b * kap; };
    double beta = rho / (Hk * kap), err = std::fabs(f(beta) - rho), lo = beta, hi = beta;
    for (int k = 0; k < 4 && err != 0.0; ++k) {
        lo = std::nextafter(lo, -HUGE_VAL); hi = std::nextafter(hi, HUGE_VAL);
        for (double c : {lo, hi}) { const double e = std::fabs(f(c) - rho); if (e < err) { err = e; beta = c; } }
    }
    return cimpc_kkt_solve(h, r, beta, delta);
}

namespace {

// What a round's last decision block published in its slot of the host ring (round_protocol.h: RingWord; new_slots is
// deterministic: slots that only wait for a parked solve are re-listed, not re-requested)
struct RoundCounts { int sweep, kkt, slots, new_slots, parked, finished; };
RoundCounts read_round_counts(const int* ring, long long round) {
    const volatile int* hr = ring_slot((const volatile int*)ring, round);
    return {hr[RING_N_SWEEP], hr[RING_N_KKT], hr[RING_SLOTS], hr[RING_NEW_SLOTS], hr[RING_PARKED], hr[RING_FINISHED]};
}

// What one cimpc_newton_solve_dev call carries from step to step
struct SolveRun {
    const double *q0_dev, *q1_dev; int warm_start;
    std::chrono::steady_clock::time_point t0;
    int tw_fail0;          // time-outs of the twisted kernels' hand-overs before this solve
    bool hybrid;
    RoundStreams sb;       // the library's private streams, or the caller's stream as sb.st when one was given
    RoundCounts last;      // counts of the last completed round (before the first: what the reset kernel requests)
};

bool has_time_budget(const cimpc_ctx* h) { return h->nt.max_time > 0.0 && h->nt.max_time < 1.0e6; }
double elapsed_s(const SolveRun& run) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - run.t0).count(); }
bool over_budget(const cimpc_ctx* h, const SolveRun& run) { return h->nt.max_time > 0.0 && elapsed_s(run) >= h->nt.max_time; }
// hand-overs of the twisted kernels that timed out since the host last looked: their KKT stages are repeated one-ended.  Returns the counter.
int note_tw_fallbacks(cimpc_ctx* h) {
    const int cur = *(volatile int*)h->h_twfail;
    if (cur != h->twfail_seen) { h->n_kkt_tw_fallbacks += cur - h->twfail_seen; h->twfail_seen = cur; }
    return cur;
}

// S as the launches of a round of this parity see it: the whole batch, the parity's counter block, ring slot and lock-step queue
NewtonDev launch_view(const cimpc_ctx* h, int parity) {
    NewtonDev Sk = h->S;
    Sk.b0 = 0; Sk.nb_launch = h->dm.B;
    Sk.counters = round_counter_block(h->d_ring, parity);
    Sk.counters_next = round_counter_block(h->d_ring, parity ^ 1);
    Sk.host_flag = ring_slot(h->h_ring_dev, parity);
    Sk.WQ = h->Q; Sk.WQ.par = parity;
    return Sk;
}
// ... with the persistent kernel's own queues and job words, from the layout of its control block
void wire_async_queues(const cimpc_ctx* h, NewtonDev& Sk) {
    const AsyncCtl L = async_ctl(h->Q.K);
    int* const c = h->a_ctrl;
    Sk.WQ.items = h->a_items; Sk.WQ.cap = (int)h->a_cap; Sk.WQ.count = c + L.count; Sk.WQ.head = c + L.head;
    AsyncQ& A = Sk.A;
    A.on = 1;
    A.rq_items = h->a_jobs; A.rq_head = c + L.rq_head; A.rq_tail = c + L.rq_tail;
    A.kq_items = h->a_jobs + h->a_rq_cap; A.kq_head = c + L.kq_head; A.kq_tail = c + L.kq_tail;
    A.n_done = c + L.n_done; A.epoch = c + L.epoch; A.evals_left = h->a_evals;
    A.abort_flag = ring_abort_word((volatile int*)h->h_ring_dev);
}

// end of a solve: statistics, Newton iteration counts, r_norm and u_1 of every rollout in one block, one copy (queued on the
// solve's stream; the caller synchronises)
int finish_results(cimpc_ctx* h, hipStream_t st) {
    if (launch_dz_commit(h->S, st) != CIMPC_OK) return fail(h, CIMPC_ERR_HIP, "sensitivity flush launch failed");
    if (int rf = launch_solve_finish(h->S, h->d_result, st); rf != CIMPC_OK) return fail(h, rf, "result kernel launch failed");
    HIP_TRY(h, hipMemcpyAsync(h->h_result, h->d_result, result_doubles(h->dm.B, h->dm.nu) * sizeof(double), hipMemcpyDeviceToHost, st));
    return CIMPC_OK;
}
// ... and, once the copy has arrived, the statistics of the solve
void publish_stats(cimpc_ctx* h, long long rounds) {
    const double* r = h->h_result;
    cimpc_stats& s = h->last_stats;
    s.sweeps = (long long)r[RESULT_SWEEPS]; s.ip_solves = (long long)r[RESULT_IP_SOLVES];
    s.ip_iters = (long long)r[RESULT_IP_ITERS]; s.ip_failures = (long long)r[RESULT_IP_FAILURES];
    s.rounds = rounds; s.newton_iters = (long long)r[RESULT_NEWTON_SUM];
}

int print_async_debug(cimpc_ctx* h) {      // CIMPC_ASYNC_DEBUG: busy time and job counts of the persistent launch
    long long dv[16];
    HIP_TRY(h, hipMemcpy(dv, h->a_dbg, sizeof(dv), hipMemcpyDeviceToHost));
    fprintf(stderr, "[cimpc async] WG-ms: other %.2f kkt %.2f resid %.2f ip %.2f | jobs: kkt %lld resid %lld serve %lld | grid %d service %d | group-trips %.2fM active %.1f%% | group-ms pop %.1f fence %.1f | pop: cas %lld spins %lld claim-ms %.1f wait-ms %.1f\n",
            dv[0] * 1e-5, dv[1] * 1e-5, dv[2] * 1e-5, dv[3] * 1e-5, dv[9], dv[10], dv[11], h->sched.async_grid, h->sched.async_service, dv[5] * 1e-6, dv[5] ? 100.0 * dv[4] / dv[5] : 0.0, dv[6] * 1e-5, dv[7] * 1e-5, dv[12], dv[13], dv[14] * 1e-5, dv[15] * 1e-5);
    return CIMPC_OK;
}
// CIMPC_DEBUG_ROUNDS: the problems round r's sweep will find in its queues (a blocking read)
void print_queued_problems(cimpc_ctx* h, const SolveRun& run, long long r, int par, long long hint) {
    std::vector<int> qc((size_t)h->Q.K * QPAD);
    (void)hipStreamSynchronize(run.sb.st); (void)hipStreamSynchronize(run.sb.st_kkt);
    if (hipMemcpy(qc.data(), h->Q.count + (size_t)par * h->Q.K * QPAD, qc.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return;
    long long tot = 0;
    for (int k = 0; k < h->Q.K; ++k) tot += qc[(size_t)k * QPAD];
    fprintf(stderr, "[cimpc round %lld] sweep launch: %lld problems queued (host hint %lld)\n", r, tot, hint);
}

// ---- one persistent launch: every rollout advances on its own chain (newton_async_impl.h).  Entered
//      from the start (from_reset) or with the rollouts the lock-step rounds left active (hybrid). ----
int run_async(cimpc_ctx* h, SolveRun& run, bool from_reset, long long rounds_before) {
    NewtonDev& S = h->S;
    IpQueues LQ = h->Q; LQ.par = (int)(rounds_before & 1);      // lock-step queue of the round that would come next
    hipStream_t st = run.sb.st;
    if (h->async_dirty) {     // entries are reset by their consumers; only an aborted solve leaves some behind
        HIP_TRY(h, hipMemsetAsync(h->a_items, 0xFF, (size_t)h->Q.K * h->a_cap * sizeof(int), st));
        HIP_TRY(h, hipMemsetAsync(h->a_jobs, 0xFF, (h->a_rq_cap + h->a_kq_cap) * sizeof(int), st));
        h->async_dirty = false;
    }
    HIP_TRY(h, hipMemsetAsync(h->a_ctrl, 0, async_ctl(h->Q.K).ints * sizeof(int), st));
    volatile int* abort_word = ring_abort_word((volatile int*)h->h_ring);
    *abort_word = 0;
    NewtonDev Sk = launch_view(h, 0);
    // the tail is latency-bound: its stragglers (rollouts that exhaust the line search in every iteration)
    // evaluate all seven step lengths at once there, whatever the throughput-oriented setting of the rounds
    if (!from_reset) Sk.spec_all = h->sched.spec_tail;
    wire_async_queues(h, Sk);
    AsyncQ& A = Sk.A;
    A.n_service = from_reset ? h->sched.async_service : h->sched.tail_service;
    A.idle_sleep = async_idle_sleep; A.idle_spins = async_idle_spins; A.wake_fan = async_wake_fan;
    A.dbg = h->a_dbg; A.B = h->dm.B;
    if (h->a_dbg) HIP_TRY(h, hipMemsetAsync(h->a_dbg, 0, 16 * sizeof(long long), st));
    // KKT stage of the persistent kernel: one job, or two cooperating jobs (the chains of the twisted solve, newton_async_impl.h)
    const KktSite site{.kind = from_reset ? KktSite::Persistent : KktSite::HybridTail, .tw_off = *(volatile int*)h->h_twfail != run.tw_fail0,
                       .B = h->dm.B, .async_tail = h->sched.async_tail, .waves = std::min(h->sched.waves, 4)};
    A.kkt_tw = plan_kkt_stage(h, site) == KktForm::AsyncTwoJob ? 1 : 0;
    S.kkt_tw_epoch += h->nt.max_iter + 2;      // the launch's KKT stages take the stamps Sk.kkt_tw_epoch + 1 + (Newton iterations done)
    prof_begin(h, PC_OTHER, st);
    int rc2 = from_reset ? launch_reset(Sk, run.q0_dev, run.q1_dev, run.warm_start, st) : launch_async_handoff(Sk, LQ, st);
    prof_end(h, st);
    if (rc2 != CIMPC_OK) return fail(h, rc2, "reset / hand-off launch failed");
    IpParams p = make_ip_params(h, S.cand, 0, round_counter(h->d_ring, RC_PARKED), nullptr);
    if (S.dtn != nullptr) { p.nu = S.nu_cand; p.dtn = S.dtn; }
    p.Q = Sk.WQ;
    p.iter_cap = h->ip.max_iter + 1;      // no solve is parked (solves parked by the lock-step rounds resume and finish)
    p.A = A;
    long long solved_before = 0;      // interior-point problems the lock-step rounds had solved (profiling only)
    if (h->prof_on && !from_reset) { long long sv[4]; if (int rs = read_stats(h, sv); rs != CIMPC_OK) return rs; solved_before = sv[1]; }
    prof_begin(h, PC_ASYNC, st);
    rc2 = launch_newton_async(&h->dm, p, Sk, std::min(h->sched.waves, 4), from_reset ? h->sched.async_grid : h->sched.tail_grid, st);
    prof_end(h, st);
    if (rc2 != CIMPC_OK) return fail(h, rc2, "asynchronous newton launch failed");
    if (int rf = finish_results(h, st); rf != CIMPC_OK) return rf;      // (queued behind the persistent kernel)
    // The host watches the persistent kernel: the reference's wall-clock budget ends the loop silently
    // (newton.jl:187-277), and a watchdog turns a kernel that stopped making progress into an error
    // instead of a hang (the kernel polls the host-mapped abort flag).
    const bool budget = has_time_budget(h);
    bool timed_out = false; long long polls = 0;
    const auto tw = std::chrono::steady_clock::now();
    while (hipStreamQuery(st) == hipErrorNotReady) {
        const bool over = budget && over_budget(h, run);
        timed_out = !over && (++polls & 0x3FF) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count() > h->kn.watchdog_s;
        if (over || timed_out) { *abort_word = 1; h->async_dirty = true; break; }
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    note_tw_fallbacks(h);
    if (timed_out) return fail(h, CIMPC_ERR_HIP, "asynchronous solve: watchdog expired (no completion within CIMPC_ASYNC_WATCHDOG_S)");
    if (h->a_dbg) { if (int rd = print_async_debug(h); rd != CIMPC_OK) return rd; }
    publish_stats(h, rounds_before + 1);
    h->prof_ip_problems += solved_before;
    h->prof_async_problems += h->last_stats.ip_solves - solved_before;
    if (from_reset) h->prof_kkt_systems += h->last_stats.newton_iters;
    return CIMPC_OK;
}

// Round r: [KKT for rollouts that start an iteration] || sweep -> residual of every evaluated slot -> line-search decision.
// blind: launched ahead of the host's knowledge of round r - 1.
int launch_round(cimpc_ctx* h, SolveRun& run, long long r, bool blind) {
    const RoundStreams& sb = run.sb; const RoundCounts& last = run.last;
    const int par = (int)(r & 1);      // round r consumes Q[par] and leaves the next round's requests in Q[par ^ 1]
    h->S.kkt_tw_epoch += 1;      // stamp of this round's KKT stage (epoch-valued hand-over flags of the twisted kernels)
    // a hand-over of a twisted kernel timed out earlier in this solve (its rollouts were queued again): one-ended kernels from here on
    const bool tw_off = note_tw_fallbacks(h) != run.tw_fail0;
    NewtonDev Sk = launch_view(h, par);
    Sk.A.n_done = run.hybrid ? h->a_ctrl + async_ctl(h->Q.K).n_done : nullptr;
    Sk.round_stamp = (int)(r + 1);
    const bool kkt = (r > 0) && (blind || last.kkt > 0);
    const int n_kkt = blind ? h->dm.B : last.kkt;
    const int* n_kkt_dev = blind ? round_counter(Sk.counters_next, RC_KKT) : nullptr;      // the previous round's count of KKT requests
    if (kkt) {
        // KKT of the rollouts that start a Newton iteration (list of the previous round's decision kernel, its queue parity).  Small
        // batches: latency matters, ahead of the sweep on its stream, the result kept in this round.  Overlapped: next to the sweep
        // on its own stream, no fork event (every decision block of the previous round released its results before its ticket).
        // (Launched BEFORE the sweep: the other order was measured 10 % / 20 % slower in rounds 1 / 3, 8.37 -> 10.05 ms - behind the
        // persistent sweep the KKT workgroups wait for sweep workgroups to leave: profiles/r03/knob_order.log.)
        const bool ov = h->kp.kkt_overlap;
        const KktSite site{.kind = ov ? KktSite::Overlapped : KktSite::Round, .n_kkt = n_kkt, .blind = blind,
                           .sweep_problems = (long long)last.new_slots * h->dm.H, .tw_off = tw_off, .B = h->dm.B};
        hipStream_t kst = ov ? sb.st_kkt : sb.st;
        if (!ov) Sk.kkt_same_round = 1;
        prof_begin(h, PC_KKT, kst);
        int rk = run_kkt_stage(h, Sk, kkt_newton_args(Sk), site, Sk.kkt_list + (size_t)(par ^ 1) * h->dm.B,
                               ov ? last.kkt : n_kkt, ov ? nullptr : n_kkt_dev, kst);      // (overlapped: the host's count, blind rounds too)
        prof_end(h, kst);
        if (rk != CIMPC_OK) return fail(h, rk, "kkt launch failed");
        if (ov && hipEventRecord(sb.ev_join, sb.st_kkt) != hipSuccess) return fail(h, CIMPC_ERR_HIP, "join record failed");
    }
    const RoundPlan rp = plan_round(h->kn.sched, h->sched, h->ip.max_iter, kkt, blind, last.sweep, last.slots);
    // problems of this round as far as the host knows them: the evaluation slots requested + the solves the last sweep parked
    const long long hint = blind ? -1 : (long long)last.slots * h->dm.H + last.parked;
    if (h->kn.debug_rounds && !blind) print_queued_problems(h, run, r, par, hint);
    int rr = run_sweep(h, par, round_counter(Sk.counters, RC_PARKED), nullptr, sb.st, rp.cap, round_counter(Sk.counters, RC_DRAINED), true, hint);
    if (rr != CIMPC_OK) return rr;
    prof_begin(h, PC_RESID, sb.st);
    if (rp.split_join) {
        rr = launch_resid_decide(Sk, sb.st, rp.n_slots, 1);
        if (rr != CIMPC_OK) return fail(h, rr, "residual launch failed");
    }
    if (kkt && h->kp.kkt_overlap && hipStreamWaitEvent(sb.st, sb.ev_join, 0) != hipSuccess) return fail(h, CIMPC_ERR_HIP, "join failed");
    rr = launch_resid_decide(Sk, sb.st, rp.n_slots, rp.split_join ? 2 : 0);
    prof_end(h, sb.st);
    if (rr != CIMPC_OK) return fail(h, rr, "residual launch failed");
    return CIMPC_OK;
}

}  // namespace

int cimpc_newton_solve_dev(cimpc_handle h, const double* q0_dev, const double* q1_dev, int warm_start) {
    int rc = check_ready(h, true);
    if (rc != CIMPC_OK) return rc;
    if (!q0_dev || !q1_dev) return fail(h, CIMPC_ERR_INVALID, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int sy = sync_dz_stores(h, DZ_NEWTON); sy != CIMPC_OK) return sy;
    h->st.solve_started();
    const int B = h->dm.B;
    SolveRun run{q0_dev, q1_dev, warm_start, {}, *(volatile int*)h->h_twfail, false, h->rs, RoundCounts{B, 0, B, B, 0, 0}};
    h->twfail_seen = run.tw_fail0;
    run.t0 = std::chrono::steady_clock::now();
    // the solve runs on the caller's stream when one was given, else on the library's streams: they wait (on the device) for what
    // the caller's stream holds - the uploads of q0 / q1 - instead of the host waiting for it
    RoundStreams& sb = run.sb;
    if (h->external_stream) sb.st = h->stream;
    else {
        HIP_TRY(h, hipEventRecord(sb.ev_start, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(sb.st, sb.ev_start, 0));
    }
    HIP_TRY(h, hipMemsetAsync(h->S.stats, 0, (size_t)B * 4 * sizeof(long long), sb.st));
    if ((rc = ensure_kkt_ws(h)) != CIMPC_OK) return rc;
    const SolvePath path = choose_solve_path(h->sched, h->kb);
    if (path == SolvePath::Persistent) return run_async(h, run, true, 0);
    run.hybrid = path == SolvePath::Hybrid;
    const int round_limit = max_rounds(h->kn.sched, h->nt.max_iter, h->ip.max_iter);
    // Lock-step rounds.  Every kernel of a round is driven by device-side state (work queues, per-rollout stage); the host only
    // looks at the counters the last decision block publishes, one round at a time.  (Measured and removed again: rounds enqueued
    // one ahead of the host's knowledge - the KKT kernel must then be launched blind at full grid, 15.9 vs 13.7 ms at B = 512 - and
    // chained rounds {sweep || KKT} -> sweep of the new candidates -> residual: every extra sweep launch pays the slowest-solve
    // tail again, 10.7 -> 11.0-11.3 ms.)
    long long launched = 0, completed = 0;
    const bool ahead = round_ahead(h->sched, h->kb, warm_start != 0, has_time_budget(h));
    HIP_TRY(h, hipMemsetAsync(h->Q.count, 0, h->ctl_ints * sizeof(int), sb.st));      // queue counters, heads, round counters
    if (run.hybrid) HIP_TRY(h, hipMemsetAsync(h->a_ctrl + async_ctl(h->Q.K).jobs, 0, ASYNC_JOB_INTS * sizeof(int), sb.st));
    for (int slot = 0; slot < RING_SLOTS_COUNT; ++slot) ring_slot((volatile int*)h->h_ring, slot)[RING_STAMP] = 0;
    prof_begin(h, PC_OTHER, sb.st);
    rc = launch_reset(launch_view(h, 0), q0_dev, q1_dev, warm_start, sb.st);
    prof_end(h, sb.st);
    if (rc != CIMPC_OK) return fail(h, rc, "reset launch failed");
    while (true) {
        if (completed >= round_limit) {          // round limit reached with work left: a scheduling bug, never a silent partial solve
            (void)hipStreamSynchronize(sb.st); (void)hipStreamSynchronize(sb.st_kkt);
            return fail(h, CIMPC_ERR_STATE, "newton_solve: round limit reached with unfinished rollouts");
        }
        while (launched <= completed + (ahead ? 1 : 0)) {
            rc = launch_round(h, run, launched, launched > completed);
            if (rc != CIMPC_OK) return rc;
            ++launched;
        }
        {   // the decision kernel's last block stamps the mapped flag when round `completed` is done
            volatile int* hm = ring_slot((volatile int*)h->h_ring, completed);
            const int want = (int)(completed + 1);
            long long spins = 0;
            while (hm[RING_STAMP] != want) {
                if ((++spins & 0xFFFFF) == 0 && hipStreamQuery(sb.st) != hipErrorNotReady && hm[RING_STAMP] != want)
                    return fail(h, CIMPC_ERR_HIP, "round finished without publishing its counters");
            }
        }
        const RoundCounts& last = run.last = read_round_counts(h->h_ring, completed);
        if (h->kn.debug_rounds) fprintf(stderr, "[cimpc round %lld] t %.3f ms: next sweep %d rollouts (%d evaluation slots), next kkt %d, parked %d, finished %d\n", completed,
                                        1e3 * elapsed_s(run), last.sweep, last.slots, last.kkt, last.parked, last.finished);
        h->prof_kkt_systems += last.kkt;
        ++completed;
        if ((last.sweep == 0 && last.kkt == 0) || over_budget(h, run)) break;   // newton.jl:187-277: budget ends silently
        if (run.hybrid && hand_over(h->sched, B - last.finished)) {
            HIP_TRY(h, hipStreamSynchronize(sb.st));
            HIP_TRY(h, hipStreamSynchronize(sb.st_kkt));
            return run_async(h, run, false, completed);
        }
    }
    HIP_TRY(h, hipStreamSynchronize(sb.st_kkt));
    if (int rf = finish_results(h, sb.st); rf != CIMPC_OK) return rf;
    HIP_TRY(h, hipStreamSynchronize(sb.st));
    publish_stats(h, completed);
    h->prof_ip_problems += h->last_stats.ip_solves;
    return CIMPC_OK;
}

int cimpc_newton_solve(cimpc_handle h, const double* q0, const double* q1, int warm_start,
                       double* u1, int* newton_iters, double* r_norm) {
    if (!h || !q0 || !q1) return fail(h, CIMPC_ERR_INVALID, "null argument");
    const size_t ne = (size_t)h->dm.B * h->dm.nq;
    HIP_TRY(h, hipSetDevice(h->device));
    // [q0 | q1] through the pinned staging buffer: one asynchronous copy on the caller's stream (the solve's streams wait for it
    // on the device), and the results come back in the one block the solve leaves in pinned memory
    std::memcpy(h->h_qin, q0, ne * sizeof(double));
    std::memcpy(h->h_qin + ne, q1, ne * sizeof(double));
    HIP_TRY(h, hipMemcpyAsync(h->d_q0, h->h_qin, 2 * ne * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = cimpc_newton_solve_dev(h, h->d_q0, h->d_q1, warm_start);
    if (rc != CIMPC_OK) return rc;
    const int nu = h->dm.nu;
    for (int b = 0; b < h->dm.B; ++b) {
        const double* o = h->h_result + result_u1(b, nu);
        if (u1) std::memcpy(u1 + (size_t)b * nu, o, nu * sizeof(double));
        if (newton_iters) newton_iters[b] = (int)o[record_iters(nu)];
        if (r_norm) r_norm[b] = o[record_r_norm(nu)] / (double)h->N;
    }
    return CIMPC_OK;
}

// ---- B4 in ONE call (round 6): what the drop-in under the reference's unchanged policy() does per MPC step - window, reference,
// altitude in, newton_solve!, core.traj / core.nu out (policy.jl:113-142) - without the five synchronous calls and their blocking
// pageable copies: every input goes through ONE pinned staging block and asynchronous copies on the handle's stream (the solve's
// streams wait for that stream on the device), the window is re-keyed only when it differs from the one last uploaded, and the
// trajectory comes back through the same block with one synchronisation.
int cimpc_mpc_solve(cimpc_handle h, const int* window, const double* q_ref, const double* u_ref, const double* w_ref,
                    const double* gamma_ref, const double* b_ref, const double* theta_ref, const double* alt,
                    const double* q0, const double* q1, int warm_start, double* u1, int* newton_iters, double* r_norm,
                    double* q, double* u, double* gamma, double* b, double* nu_dual) {
    if (!h || !q0 || !q1) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (q_ref && (!u_ref || !theta_ref)) return fail(h, CIMPC_ERR_INVALID, "q_ref, u_ref, theta_ref go together");
    const HorizonSizes sz = horizon_sizes(h->dm, h->nth, h->nd);
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->h_stage) {
        // [window (as doubles' worth of ints) | q | u | w | gamma | b | theta | alt]; the way out reuses [q | u | gamma | b | nu]
        h->h_stage_doubles = (sz.win + 1) / 2 + sz.q + sz.u + sz.w + sz.g + sz.b + std::max(sz.th, sz.nu) + sz.alt + 8;
        if (hipHostMalloc((void**)&h->h_stage, h->h_stage_doubles * sizeof(double), hipHostMallocDefault) != hipSuccess)
            return fail(h, CIMPC_ERR_HIP, "hipHostMalloc failed");
    }
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    double* stage = h->h_stage;
    int* s_win = reinterpret_cast<int*>(stage);
    double* s_q = stage + (sz.win + 1) / 2; double* s_u = s_q + sz.q; double* s_w = s_u + sz.u; double* s_g = s_w + sz.w;
    double* s_b = s_g + sz.g; double* s_th = s_b + sz.b; double* s_alt = s_th + std::max(sz.th, sz.nu);
    hipStream_t st = h->stream;
    if (window) {
        if (int rc = refuse(h, window_to_knots(window, sz.win, h->dm.H_ref, s_win)); rc != CIMPC_OK) return rc;
        // the per-knot sensitivity memory moves with the window (cimpc_set_window), stream-ordered.  (A window equal to the mirror
        // is in force already: a mirror that is not empty says so, and that no gait generates the window - handle_state.h)
        if (!h->st.mirror_equals(s_win, sz.win)) {
            int rc = window_move(h->st, WindowHome::Host, s_win, sz.win, [&] { return rekey_out(h); },
                [&]() -> int { HIP_TRY(h, hipMemcpyAsync(h->d_window, s_win, sz.win * sizeof(int), hipMemcpyHostToDevice, st)); return CIMPC_OK; },
                [&] { return rekey_in(h); });
            if (rc != CIMPC_OK) return rc;
        }
    }
    if (q_ref) {
        h->st.unlatch();      // (as cimpc_set_reference; the solve below sets it again)
        auto up = [&](double* dst, double* stg, const double* src, size_t n) -> hipError_t {
            if (n == 0) return hipSuccess;
            if (src) std::memcpy(stg, src, n * sizeof(double)); else std::memset(stg, 0, n * sizeof(double));
            return hipMemcpyAsync(dst, stg, n * sizeof(double), hipMemcpyHostToDevice, st);
        };
        HIP_TRY(h, up(h->S.ref.q, s_q, q_ref, sz.q));
        HIP_TRY(h, up(h->S.ref.u, s_u, u_ref, sz.u));
        HIP_TRY(h, up(h->S.ref.w, s_w, w_ref, sz.w));                       // NULL = zeros, as cimpc_set_reference
        if (gamma_ref) HIP_TRY(h, up(h->S.ref.g, s_g, gamma_ref, sz.g));   // NULL = unchanged, as cimpc_set_reference
        if (b_ref) HIP_TRY(h, up(h->S.ref.b, s_b, b_ref, sz.b));
        HIP_TRY(h, up(h->S.ref.th, s_th, theta_ref, sz.th));
        h->st.reference_replaced();
    }
    if (alt) {
        std::memcpy(s_alt, alt, sz.alt * sizeof(double));
        HIP_TRY(h, hipMemcpyAsync(h->d_alt, s_alt, sz.alt * sizeof(double), hipMemcpyHostToDevice, st));
        h->st.altitude_set();
    }
    int rc = cimpc_newton_solve(h, q0, q1, warm_start, u1, newton_iters, r_norm);
    if (rc != CIMPC_OK) return rc;
    if (q || u || gamma || b || nu_dual) {
        // (the solve has completed on the library's streams; these copies run on the handle's stream, one synchronisation)
        auto down = [&](double* stg, const double* src, double* dst, size_t n) -> hipError_t {
            return (dst && n) ? hipMemcpyAsync(stg, src, n * sizeof(double), hipMemcpyDeviceToHost, st) : hipSuccess;
        };
        HIP_TRY(h, down(s_q, h->S.traj.q, q, sz.q));
        HIP_TRY(h, down(s_u, h->S.traj.u, u, sz.u));
        HIP_TRY(h, down(s_g, h->S.traj.g, gamma, sz.g));
        HIP_TRY(h, down(s_b, h->S.traj.b, b, sz.b));
        HIP_TRY(h, down(s_th, h->S.nu, nu_dual, sz.nu));
        HIP_TRY(h, hipStreamSynchronize(st));
        if (q) std::memcpy(q, s_q, sz.q * sizeof(double));
        if (u) std::memcpy(u, s_u, sz.u * sizeof(double));
        if (gamma && sz.g) std::memcpy(gamma, s_g, sz.g * sizeof(double));
        if (b && sz.b) std::memcpy(b, s_b, sz.b * sizeof(double));
        if (nu_dual) std::memcpy(nu_dual, s_th, sz.nu * sizeof(double));
    }
    return CIMPC_OK;
}

int cimpc_get_trajectory(cimpc_handle h, double* q, double* u, double* gamma, double* b, double* nu_dual) {
    if (!h) return CIMPC_ERR_INVALID;
    const HorizonSizes n = horizon_sizes(h->dm, h->nth, h->nd);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (q) HIP_TRY(h, hipMemcpy(q, h->S.traj.q, n.q * sizeof(double), hipMemcpyDeviceToHost));
    if (u) HIP_TRY(h, hipMemcpy(u, h->S.traj.u, n.u * sizeof(double), hipMemcpyDeviceToHost));
    if (gamma) HIP_TRY(h, hipMemcpy(gamma, h->S.traj.g, n.g * sizeof(double), hipMemcpyDeviceToHost));
    if (b) HIP_TRY(h, hipMemcpy(b, h->S.traj.b, n.b * sizeof(double), hipMemcpyDeviceToHost));
    if (nu_dual) HIP_TRY(h, hipMemcpy(nu_dual, h->S.nu, n.nu * sizeof(double), hipMemcpyDeviceToHost));
    return CIMPC_OK;
}

int cimpc_get_newton_info(cimpc_handle h, int* newton_iters, double* r_norm, double* u1) {
    if (!h) return CIMPC_ERR_INVALID;
    const cimpc_dims& d = h->dm;
    const size_t B = d.B;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (newton_iters) HIP_TRY(h, hipMemcpy(newton_iters, h->S.newton_l, B * sizeof(int), hipMemcpyDeviceToHost));
    if (r_norm) {
        HIP_TRY(h, hipMemcpy(r_norm, h->S.r_norm, B * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) r_norm[b] /= (double)h->N;
    }
    if (u1)     // core.traj.u[1] of every rollout (policy.jl:142)
        HIP_TRY(h, hipMemcpy2D(u1, d.nu * sizeof(double), h->S.traj.u, (size_t)d.H * d.nu * sizeof(double),
                               d.nu * sizeof(double), B, hipMemcpyDeviceToHost));
    return CIMPC_OK;
}

int cimpc_get_rollout_counters(cimpc_handle h, int* sweeps, int* ip_iters, int* ip_failures) {
    if (!h) return CIMPC_ERR_INVALID;
    const size_t B = h->dm.B;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (sweeps) HIP_TRY(h, hipMemcpy(sweeps, h->S.ro_sweeps, B * sizeof(int), hipMemcpyDeviceToHost));
    if (ip_iters) HIP_TRY(h, hipMemcpy(ip_iters, h->S.ro_ip_iters, B * sizeof(int), hipMemcpyDeviceToHost));
    if (ip_failures) HIP_TRY(h, hipMemcpy(ip_failures, h->S.ro_ip_fail, B * sizeof(int), hipMemcpyDeviceToHost));
    return CIMPC_OK;
}

static GaitDev gait_dev(cimpc_ctx* h) {
    return GaitDev{h->g_q, h->g_u, h->g_w, h->g_g, h->g_b, h->g_th, h->g_stride, h->g_phase, h->dm.H_ref};
}

int cimpc_set_gait(cimpc_handle h, const double* q, const double* u, const double* w, const double* gamma,
                   const double* b, const double* theta, const double* stride, const int* phase) {
    if (!h || !q || !u || !theta || !stride) return fail(h, CIMPC_ERR_INVALID, "q, u, theta, stride are required");
    h->st.unlatch();
    const cimpc_dims& d = h->dm;
    const size_t K = d.H_ref, B = d.B;
    if (d.H > d.H_ref) return fail(h, CIMPC_ERR_INVALID, "H_mpc must not exceed H_ref");
    if (phase) for (size_t i = 0; i < B; ++i) if (phase[i] < 0) return fail(h, CIMPC_ERR_INVALID, "negative phase");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    if (!h->g_q) {
        if (dev_alloc(h, &h->g_q, (K + 2) * d.nq) != CIMPC_OK || dev_alloc(h, &h->g_u, K * d.nu) != CIMPC_OK ||
            dev_alloc(h, &h->g_w, K * d.nw) != CIMPC_OK || dev_alloc(h, &h->g_g, K * d.nc) != CIMPC_OK ||
            dev_alloc(h, &h->g_b, K * d.nb) != CIMPC_OK || dev_alloc(h, &h->g_th, K * h->nth) != CIMPC_OK ||
            dev_alloc(h, &h->g_stride, d.nq) != CIMPC_OK || dev_alloc(h, &h->g_phase, B) != CIMPC_OK)
            return CIMPC_ERR_HIP;                    // (dev_alloc zero-fills: w, gamma, b default to 0)
    }
    HIP_TRY(h, hipMemcpy(h->g_q, q, (K + 2) * d.nq * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->g_u, u, K * d.nu * sizeof(double), hipMemcpyHostToDevice));
    auto opt = [&](double* dst, const double* src, size_t n) {      // NULL = zeros (also when an earlier call gave values)
        return src ? hipMemcpy(dst, src, n * sizeof(double), hipMemcpyHostToDevice) : hipMemset(dst, 0, n * sizeof(double));
    };
    HIP_TRY(h, opt(h->g_w, w, K * d.nw));
    HIP_TRY(h, opt(h->g_g, gamma, K * d.nc));
    HIP_TRY(h, opt(h->g_b, b, K * d.nb));
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    HIP_TRY(h, hipMemcpy(h->g_th, theta, K * h->nth * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->g_stride, stride, d.nq * sizeof(double), hipMemcpyHostToDevice));
    if (phase) HIP_TRY(h, hipMemcpy(h->g_phase, phase, B * sizeof(int), hipMemcpyHostToDevice));
    else { HIP_TRY(h, hipMemset(h->g_phase, 0, B * sizeof(int))); HIP_TRY(h, hipStreamSynchronize(nullptr)); }
    int rc = window_move(h->st, WindowHome::Device, nullptr, 0, [&] { return rekey_out(h); },      // the window now lives on the device only
        [&] { int rg = launch_gait_window(h->S, gait_dev(h), h->d_window, 0, h->stream); return rg == CIMPC_OK ? CIMPC_OK : fail(h, rg, "gait window launch failed"); },
        [&] { return then_sync(h, rekey_in(h)); });
    if (rc != CIMPC_OK) return rc;
    h->st.gait_installed();
    return CIMPC_OK;
}

int cimpc_mpc_advance(cimpc_handle h, const double* stride) {
    if (!h || !stride) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (int rc = refuse(h, h->st.advance_refusal()); rc != CIMPC_OK) return rc;
    h->st.unlatch();                 // the window and the reference move on: a latch now would take the NEXT step's K and target
    HIP_TRY(h, hipSetDevice(h->device));
    // The advance is QUEUED on the handle's stream and not waited for: whatever comes next is ordered behind it on the device
    // (the solve's streams wait for this stream, every getter synchronises it first).  The stride goes through a pinned word;
    // a second advance in a row waits for the first one's copy to have left it.
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    double* st_pin = h->h_qin + 2 * (size_t)h->dm.B * h->dm.nq;
    std::memcpy(st_pin, stride, (size_t)h->dm.nq * sizeof(double));
    auto launched = [&](int rc) { return rc == CIMPC_OK ? CIMPC_OK : fail(h, rc, "mpc_advance launch failed"); };
    if (h->st.advances_by_gait()) {          // full reference resident: regenerate the horizon from the gait (stride as given now)
        int rc = window_move(h->st, WindowHome::Device, nullptr, 0,
            [&]() -> int { HIP_TRY(h, hipMemcpyAsync(h->g_stride, st_pin, (size_t)h->dm.nq * sizeof(double), hipMemcpyHostToDevice, h->stream)); return rekey_out(h); },
            [&] { return launched(launch_gait_window(h->S, gait_dev(h), h->d_window, 1, h->stream)); },
            [&] { return rekey_in(h); });
        if (rc == CIMPC_OK) h->st.advance_queued();
        return rc;
    }
    return window_move(h->st, WindowHome::Device, nullptr, 0,
        [&]() -> int { HIP_TRY(h, hipMemcpyAsync(h->d_q0, stride, (size_t)h->dm.nq * sizeof(double), hipMemcpyHostToDevice, h->stream)); return rekey_out(h); },   // d_q0: staging
        [&] { return launched(launch_mpc_advance(h->S, h->d_window, h->d_q0, h->dm.H_ref, h->stream)); },
        [&] { return then_sync(h, rekey_in(h)); });
}

// ---- feedback gains on the handle (gains.hip) -------------------------------------------------------------------------------------
int cimpc_set_gains(cimpc_handle h, const double* K) {
    if (!h) return CIMPC_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    h->st.gains_changing();
    if (!K) { h->st.gains_cleared(); return CIMPC_OK; }
    const cimpc_dims& d = h->dm;
    const size_t nk = (size_t)d.nu * 2 * d.nq;
    // each buffer by itself: one that could not be allocated is asked for again by the next call, and the gains count as set only once all exist
    if (!h->d_gK && dev_alloc(h, &h->d_gK, (size_t)d.H_ref * nk) != CIMPC_OK) return CIMPC_ERR_HIP;
    if (!h->d_glatch && dev_alloc(h, &h->d_glatch, (size_t)d.B * gain_latch_doubles(d.nq, d.nu)) != CIMPC_OK) return CIMPC_ERR_HIP;
    if (!h->d_gio && dev_alloc(h, &h->d_gio, (size_t)d.B * (2 * d.nq + d.nu)) != CIMPC_OK) return CIMPC_ERR_HIP;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->d_gK, K, (size_t)d.H_ref * nk * sizeof(double), hipMemcpyHostToDevice));
    h->st.gains_replaced();
    return CIMPC_OK;
}

int cimpc_gain_latch(cimpc_handle h) {
    if (!h) return CIMPC_ERR_INVALID;
    if (int rc = refuse(h, h->st.latch_refusal()); rc != CIMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int dp = drain_pending(h); dp != CIMPC_OK) return dp;
    const cimpc_dims& d = h->dm;
    if (!gain_latch_launch(d.B, d.H, d.nq, d.nu, h->d_window, h->S.traj.u, h->S.ref.q, h->d_gK, h->d_glatch, h->stream))
        return fail(h, CIMPC_ERR_HIP, "gain latch launch failed");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->st.latched();
    return CIMPC_OK;
}

int cimpc_gain_feedback(cimpc_handle h, const double* q_prev, const double* q_cur, double n_sample, double* u) {
    if (!h || !q_prev || !q_cur || !u) return fail(h, CIMPC_ERR_INVALID, "null argument");
    if (!std::isfinite(n_sample) || n_sample <= 0.0) return fail(h, CIMPC_ERR_INVALID, "n_sample must be finite and positive");
    if (int rc = refuse(h, h->st.feedback_refusal()); rc != CIMPC_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const cimpc_dims& d = h->dm;
    const size_t nqB = (size_t)d.B * d.nq, nuB = (size_t)d.B * d.nu;
    double* dq = h->d_gio;
    HIP_TRY(h, hipMemcpyAsync(dq, q_prev, nqB * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dq + nqB, q_cur, nqB * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (!gain_feedback_launch(d.B, d.nq, d.nu, h->d_glatch, dq, dq + nqB, n_sample, dq + 2 * nqB, h->stream))
        return fail(h, CIMPC_ERR_HIP, "gain feedback launch failed");
    HIP_TRY(h, hipMemcpyAsync(u, dq + 2 * nqB, nuB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CIMPC_OK;
}

int cimpc_get_reference(cimpc_handle h, double* q_ref, double* u_ref, double* w_ref, double* gamma_ref,
                        double* b_ref, double* theta_ref, int* window) {
    if (!h) return CIMPC_ERR_INVALID;
    const HorizonSizes n = horizon_sizes(h->dm, h->nth, h->nd);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (q_ref) HIP_TRY(h, hipMemcpy(q_ref, h->S.ref.q, n.q * sizeof(double), hipMemcpyDeviceToHost));
    if (u_ref) HIP_TRY(h, hipMemcpy(u_ref, h->S.ref.u, n.u * sizeof(double), hipMemcpyDeviceToHost));
    if (w_ref) HIP_TRY(h, hipMemcpy(w_ref, h->S.ref.w, n.w * sizeof(double), hipMemcpyDeviceToHost));
    if (gamma_ref) HIP_TRY(h, hipMemcpy(gamma_ref, h->S.ref.g, n.g * sizeof(double), hipMemcpyDeviceToHost));
    if (b_ref) HIP_TRY(h, hipMemcpy(b_ref, h->S.ref.b, n.b * sizeof(double), hipMemcpyDeviceToHost));
    if (theta_ref) HIP_TRY(h, hipMemcpy(theta_ref, h->S.ref.th, n.th * sizeof(double), hipMemcpyDeviceToHost));
    if (window) {
        HIP_TRY(h, hipMemcpy(window, h->d_window, n.win * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n.win; ++k) window[k] += 1;     // 1-based at the boundary
    }
    return CIMPC_OK;
}

int cimpc_get_newton_log(cimpc_handle h, double* log, int max_entries) {
    if (!h || !log || max_entries <= 0) return CIMPC_ERR_INVALID;
    const size_t B = h->dm.B;
    const int n = std::min(max_entries, NLOG);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy2D(log, (size_t)max_entries * 4 * sizeof(double), h->S.nlog, (size_t)NLOG * 4 * sizeof(double),
                           (size_t)n * 4 * sizeof(double), B, hipMemcpyDeviceToHost));
    return CIMPC_OK;
}

int cimpc_get_kkt_twisted(cimpc_handle h, long long* n) {
    if (!h || !n) return CIMPC_ERR_INVALID;
    *n = h->n_kkt_twisted;
    return CIMPC_OK;
}

int cimpc_get_kkt_twisted_fallbacks(cimpc_handle h, long long* n) {
    if (!h || !n) return CIMPC_ERR_INVALID;
    note_tw_fallbacks(h);
    *n = h->n_kkt_tw_fallbacks;
    return CIMPC_OK;
}

int cimpc_debug_set_tw_spins(cimpc_handle h, int spins) {
    if (!h) return CIMPC_ERR_INVALID;
    h->S.kkt_tw_spins = spins > 0 ? spins : KKT_TW_SPINS;
    return CIMPC_OK;
}

int cimpc_get_kkt_fallbacks(cimpc_handle h, long long* n) {
    if (!h || !n) return CIMPC_ERR_INVALID;
    *n = 0;
    if (!h->d_mix_nfb) return CIMPC_OK;
    int v = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(&v, h->d_mix_nfb, sizeof(int), hipMemcpyDeviceToHost));
    *n = v;
    return CIMPC_OK;
}

#if defined(CIMPC_KKT_PROF) || defined(CIMPC_KKT_TWPROF)
// diagnostic builds only: raw read of the statistics buffer (the KKT kernels park their phase clocks at [8..23])
int cimpc_debug_read_stats(cimpc_handle h, long long* out, int n) {
    if (!h || !out || n > std::max(h->dm.B * 4, 64)) return CIMPC_ERR_INVALID;
    HIP_TRY(h, hipMemcpy(out, h->S.stats, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost));
    return CIMPC_OK;
}
#endif

#ifdef CIMPC_DEBUG_STATS
// diagnostic builds only: the raw per-rollout statistics records + the device addresses of the neighbouring allocations
int cimpc_debug_dump_stats(cimpc_handle h, long long* out, unsigned long long* addr8) {
    if (!h || !out || !addr8) return CIMPC_ERR_INVALID;
    HIP_TRY(h, hipMemcpy(out, h->S.stats, (size_t)h->dm.B * 4 * sizeof(long long), hipMemcpyDeviceToHost));
    const void* a[8] = {h->S.kkt_list, h->S.slot_list, h->S.counters, h->S.stats, h->S.ro_sweeps, h->S.ro_ip_iters, h->S.ro_ip_fail, h->S.nlog};
    for (int k = 0; k < 8; ++k) addr8[k] = (unsigned long long)a[k];
    return CIMPC_OK;
}
#endif

int cimpc_get_stats(cimpc_handle h, cimpc_stats* s) {
    if (!h || !s) return CIMPC_ERR_INVALID;
    *s = h->last_stats;
    return CIMPC_OK;
}

int cimpc_profile_enable(cimpc_handle h, int on) {
    if (!h) return CIMPC_ERR_INVALID;
    prof_collect(h);
    h->prof_on = on == 2 ? 2 : (on != 0 ? 1 : 0);
    return CIMPC_OK;
}

int cimpc_profile_reset(cimpc_handle h) {
    if (!h) return CIMPC_ERR_INVALID;
    prof_collect(h);
    for (int c = 0; c < PC_COUNT; ++c) { h->prof_ms[c] = 0.0; h->prof_n[c] = 0; }
    h->prof_ip_problems = 0;
    h->prof_async_problems = 0;
    h->prof_kkt_systems = 0;
    return CIMPC_OK;
}

int cimpc_profile_read(cimpc_handle h, cimpc_profile* p) {
    if (!h || !p) return CIMPC_ERR_INVALID;
    prof_collect(h);
    p->ip_sweep_ms = h->prof_ms[PC_IP]; p->ip_sweep_launches = h->prof_n[PC_IP];
    p->ip_sweep_problems = h->prof_ip_problems;
    p->kkt_ms = h->prof_ms[PC_KKT]; p->kkt_launches = h->prof_n[PC_KKT]; p->kkt_systems = h->prof_kkt_systems;
    p->resid_ms = h->prof_ms[PC_RESID]; p->resid_launches = h->prof_n[PC_RESID];
    p->other_ms = h->prof_ms[PC_OTHER]; p->other_launches = h->prof_n[PC_OTHER];
    p->async_ms = h->prof_ms[PC_ASYNC]; p->async_launches = h->prof_n[PC_ASYNC]; p->async_problems = h->prof_async_problems;
    return CIMPC_OK;
}

int cimpc_query_sizes(cimpc_handle h, int* table_doubles, int* N_kkt) {
    if (!h) return CIMPC_ERR_INVALID;
    if (table_doubles) *table_doubles = h->ki.tab_size;
    if (N_kkt) *N_kkt = h->N;
    return CIMPC_OK;
}

}  // extern "C"

#ifdef CIMPC_UBENCH
// diagnostic builds only: the device address of the handle's linearization tables (scripts/dbg/ubench_ip.py)
extern "C" const double* cimpc_debug_table_ptr(cimpc_handle h) { return h ? h->d_tab : nullptr; }
#endif
