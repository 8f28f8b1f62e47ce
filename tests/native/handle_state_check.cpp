// Host-only driver of contactimplicitmpc/jl_amd/csrc/handle_state.h (tests/test_handle_state.py): no input; one output line per case.
//   move <home> fail=<step or none> ...        window_move from a latched state with a mirror, each failure point and each home
//   knots K=<K> in=<..> rc=<code> out=<..>     window_to_knots
//   sizes <model> B=<B> H=<H> win=.. ..        horizon_sizes and horizon_rows
//   ready knots=<0|1> newton=<0|1> <state> | <code> <message>      what check_ready refuses
//   replay <entry> | <state> | <state> | <code> <message>          every entry point, as cimpc_host.cpp drives the state on a path
//                                                                  where every HIP call succeeds, from every state that can be reached
#include "../../contactimplicitmpc/jl_amd/csrc/handle_state.h"

#include <cstdio>
#include <functional>
#include <set>
#include <string>
#include <vector>

using namespace cimpc;

static std::string show(const HandleState& s) {
    char buf[256];
    snprintf(buf, sizeof buf, "obj=%d win=%d ref=%d alt=%d gait=%d gains=%d latched=%d latch=%d pending=%d dz=%d mirror=", s.objective_set, s.window_set,
             s.reference_set, s.alt_set, s.gait_set, s.gains_set, s.gains_latched, s.latch_ready, s.advance_pending, s.dz_producer);
    std::string out = buf;
    if (s.win_mirror.empty()) out += "-";
    for (size_t k = 0; k < s.win_mirror.size(); ++k) out += (k ? "," : "") + std::to_string(s.win_mirror[k]);
    return out;
}

static void moves() {
    const int codes[3] = {CIMPC_ERR_HIP, CIMPC_ERR_STATE, CIMPC_ERR_INVALID};      // a different code from each step: it must come back as it is
    const int w0[3] = {5, 6, 7};
    for (WindowHome home : {WindowHome::Host, WindowHome::Device})
        for (int gait = 0; gait < 2; ++gait)
            for (int fail = -1; fail < 3; ++fail) {
                HandleState s;
                s.window_set = s.latch_ready = true;
                s.gait_set = gait != 0;
                s.win_mirror = {1, 2, 3};
                int called[3] = {0, 0, 0};
                auto step = [&](int k) { return [&, k] { called[k]++; return fail == k ? codes[k] : CIMPC_OK; }; };
                const int rc = window_move(s, home, home == WindowHome::Host ? w0 : nullptr, home == WindowHome::Host ? 3 : 0, step(0), step(1), step(2));
                printf("move %s gait0=%d fail=%d rc=%d calls=%d,%d,%d %s\n", home == WindowHome::Host ? "host" : "device", gait, fail, rc, called[0], called[1],
                       called[2], show(s).c_str());
            }
    {   // a first window: nothing set before
        HandleState s;
        const int rc = window_move(s, WindowHome::Device, nullptr, 0, [] { return CIMPC_OK; }, [] { return CIMPC_OK; }, [] { return CIMPC_OK; });
        printf("move device gait0=0 fail=first rc=%d calls=1,1,1 %s\n", rc, show(s).c_str());
    }
}

static void knots() {
    const int K = 8;
    auto run = [&](std::vector<int> in) {
        std::vector<int> out(in.size(), -7);
        const Refusal r = window_to_knots(in.data(), in.size(), K, out.data());
        printf("knots K=%d in=", K);
        for (size_t k = 0; k < in.size(); ++k) printf("%s%d", k ? "," : "", in[k]);
        printf(" rc=%d out=", r.code);
        for (size_t k = 0; k < out.size(); ++k) printf("%s%d", k ? "," : "", out[k]);
        printf(" | %s\n", r.msg ? r.msg : "");
    };
    run({1, 8, 3, 4, 8, 1});
    for (int bad : {0, K + 1})
        for (size_t at : {(size_t)0, (size_t)3, (size_t)5}) {
            std::vector<int> in = {1, 8, 3, 4, 8, 1};
            in[at] = bad;
            run(in);
        }
}

static void sizes() {
    struct M { const char* name; int nq, nu, nw, nc, nb; };
    for (const M& m : {M{"quadruped", 11, 8, 2, 4, 8}, M{"pushbot", 2, 2, 2, 2, 4}, M{"centroidal_wall", 18, 12, 3, 8, 32}})
        for (int mode : {0, 1})
            for (int B : {1, 3})
                for (int H : {1, 8}) {
                    cimpc_dims d{};
                    d.nq = m.nq; d.nu = m.nu; d.nw = m.nw; d.nc = m.nc; d.nb = m.nb; d.mode = mode; d.H_ref = 12; d.H = H; d.B = B;
                    const int nth = 2 * d.nq + d.nu + d.nw + 2, nd = mode ? d.nq + d.nc + d.nb : d.nq;      // as cimpc_create has them
                    const HorizonSizes n = horizon_sizes(d, nth, nd), r = horizon_rows(d, nth, nd);
                    printf("sizes %s mode=%d B=%d H=%d win=%zu q=%zu u=%zu w=%zu g=%zu b=%zu th=%zu nu=%zu alt=%zu row_win=%zu row_q=%zu row_u=%zu row_w=%zu "
                           "row_g=%zu row_b=%zu row_th=%zu row_nu=%zu row_alt=%zu\n", m.name, mode, B, H, n.win, n.q, n.u, n.w, n.g, n.b, n.th, n.nu, n.alt,
                           r.win, r.q, r.u, r.w, r.g, r.b, r.th, r.nu, r.alt);
                }
}

static void ready() {
    for (int bits = 0; bits < 16; ++bits)
        for (int newton = 0; newton < 2; ++newton) {
            HandleState s;
            s.window_set = bits & 2; s.objective_set = bits & 4; s.reference_set = bits & 8;
            const Refusal r = s.solve_refusal(bits & 1, newton != 0);
            printf("ready knots=%d newton=%d %s | %d %s\n", bits & 1, newton, show(s).c_str(), r.code, r.msg ? r.msg : "");
        }
}

// ---- the entry points of cimpc_host.cpp, reduced to what they do to the state when every HIP call succeeds ----------------------------
static int ok() { return CIMPC_OK; }
static void drain(HandleState& s) { if (s.drain_needed()) s.advance_drained(); }      // drain_pending
static const std::vector<int> WIN_A = {0, 1, 2}, WIN_B = {1, 2, 3};

static Refusal newton_solve(HandleState& s) {      // cimpc_newton_solve_dev
    if (Refusal r = s.solve_refusal(true, true); r.code != CIMPC_OK) return r;
    s.solve_started();
    return {CIMPC_OK, nullptr};
}
static Refusal mpc_solve(HandleState& s, const std::vector<int>* w, bool ref, bool alt) {      // cimpc_mpc_solve
    drain(s);
    if (w && !s.mirror_equals(w->data(), w->size())) window_move(s, WindowHome::Host, w->data(), w->size(), ok, ok, ok);
    if (ref) { s.unlatch(); s.reference_replaced(); }
    if (alt) s.altitude_set();
    return newton_solve(s);
}

struct Entry {
    const char* name;
    std::function<Refusal(HandleState&)> run;
};
static const Refusal FINE = {CIMPC_OK, nullptr};

static std::vector<Entry> entries() {
    std::vector<Entry> e;
    e.push_back({"set_stream", [](HandleState& s) { s.advance_drained(); return FINE; }});
    e.push_back({"set_linearization", [](HandleState& s) { drain(s); return FINE; }});
    e.push_back({"set_objective", [](HandleState& s) { drain(s); s.objective_replaced(); return FINE; }});
    e.push_back({"set_objective_singular", [](HandleState& s) { drain(s); s.objective_refused(); return FINE; }});
    e.push_back({"set_altitude", [](HandleState& s) { drain(s); s.altitude_set(); return FINE; }});
    e.push_back({"set_altitude_null", [](HandleState& s) { s.altitude_cleared(); return FINE; }});
    for (const std::vector<int>* w : {&WIN_A, &WIN_B})
        e.push_back({w == &WIN_A ? "set_window_a" : "set_window_b", [w](HandleState& s) {
            s.unlatch(); drain(s); window_move(s, WindowHome::Host, w->data(), w->size(), ok, ok, ok); return FINE; }});
    e.push_back({"set_reference", [](HandleState& s) { s.unlatch(); drain(s); s.reference_replaced(); return FINE; }});
    e.push_back({"implicit_dynamics", [](HandleState& s) {
        if (Refusal r = s.solve_refusal(true, false); r.code != CIMPC_OK) return r;
        s.implicit_dynamics_started(); return FINE; }});
    e.push_back({"newton_solve", [](HandleState& s) { return newton_solve(s); }});
    e.push_back({"mpc_solve", [](HandleState& s) { return mpc_solve(s, nullptr, false, false); }});
    e.push_back({"mpc_solve_a", [](HandleState& s) { return mpc_solve(s, &WIN_A, false, false); }});
    e.push_back({"mpc_solve_b_ref", [](HandleState& s) { return mpc_solve(s, &WIN_B, true, false); }});
    e.push_back({"mpc_solve_ref_alt", [](HandleState& s) { return mpc_solve(s, nullptr, true, true); }});
    e.push_back({"set_gait", [](HandleState& s) {
        s.unlatch(); drain(s); window_move(s, WindowHome::Device, nullptr, 0, ok, ok, ok); s.gait_installed(); return FINE; }});
    e.push_back({"mpc_advance", [](HandleState& s) {
        if (Refusal r = s.advance_refusal(); r.code != CIMPC_OK) return r;
        s.unlatch(); drain(s);
        const bool gait = s.advances_by_gait();
        window_move(s, WindowHome::Device, nullptr, 0, ok, ok, ok);
        if (gait) s.advance_queued();
        return FINE; }});
    e.push_back({"set_gains", [](HandleState& s) { drain(s); s.gains_changing(); s.gains_replaced(); return FINE; }});
    e.push_back({"set_gains_null", [](HandleState& s) { drain(s); s.gains_changing(); s.gains_cleared(); return FINE; }});
    e.push_back({"gain_latch", [](HandleState& s) {
        if (Refusal r = s.latch_refusal(); r.code != CIMPC_OK) return r;
        drain(s); s.latched(); return FINE; }});
    e.push_back({"gain_feedback", [](HandleState& s) { return s.feedback_refusal(); }});
    return e;
}

static void replay() {
    const std::vector<Entry> es = entries();
    std::vector<HandleState> todo = {HandleState{}};
    std::set<std::string> seen = {show(todo[0])};
    while (!todo.empty()) {
        const HandleState s0 = todo.back();
        todo.pop_back();
        for (const Entry& e : es) {
            HandleState s = s0;
            const Refusal r = e.run(s);
            printf("replay %s | %s | %s | %d %s\n", e.name, show(s0).c_str(), show(s).c_str(), r.code, r.msg ? r.msg : "");
            if (seen.insert(show(s)).second) todo.push_back(s);
        }
    }
}

int main() {
    moves();
    knots();
    sizes();
    ready();
    replay();
    return 0;
}
