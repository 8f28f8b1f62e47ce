// Host-only check of contactimplicitmpc/jl_amd/csrc/plant_staging.h (tests/test_plant_staging.py).  No arguments; every property is an
// assertion that names itself on failure, and the program prints `ok <n>` with the number of assertions it made.
//   tiling     regions follow each other in take order without gaps or overlap, an absent region takes no room and is null from or_null,
//              end() is the sum and starts over
//   copier     driven with memcpy over heap buffers of exactly end() elements: up of every region then down of every region returns
//              the inputs, and zero-count or null-host copies touch nothing.  Under AddressSanitizer a copy past its region aborts.
//   layouts    plant_linesearch_layout and plant_segments_layout - the functions the library calls - at hopper_2D (nq 4, nu 2, nc 1, nb 2,
//              nz 12, nw 2), B = 2, T = 4, n_alpha = 2, segments = 2, every optional array once present and once absent.  The expected
//              offsets are worked out by hand from the chains of offsets the entries used to spell out, not by the code under test.
//   refusals   plant_refuse and plant_first_null leave, byte for byte, the strings the entries have always left
#include "../../contactimplicitmpc/jl_amd/csrc/plant_staging.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace cimpc;

namespace {
std::string g_error;
int g_checks = 0;
}  // namespace
void cimpc::set_global_error(const std::string& msg) { g_error = msg; }

namespace {

void expect(bool cond, const std::string& what) {
    ++g_checks;
    if (cond) return;
    std::printf("FAILED: %s\n", what.c_str());
    std::exit(1);
}

struct Named { const char* name; PlantSpan span; };

// `spans` in take order tile [0, need): each starts where the last one ended, and the last one ends at need
void expect_tiling(const char* what, const std::vector<Named>& spans, size_t need) {
    size_t at = 0;
    for (const Named& s : spans) {
        expect(s.span.at == at, std::string(what) + ": " + s.name + " does not start where its predecessor ends");
        at += s.span.n;
    }
    expect(at == need, std::string(what) + ": the need is not the sum of the regions");
}

void expect_spans(const char* what, const std::vector<Named>& got, const std::vector<PlantSpan>& want, size_t need, size_t want_need) {
    expect(got.size() == want.size(), std::string(what) + ": the number of regions");
    for (size_t i = 0; i < got.size(); ++i) {
        expect(got[i].span.at == want[i].at, std::string(what) + ": offset of " + got[i].name + " = " + std::to_string(got[i].span.at) + ", by hand " + std::to_string(want[i].at));
        expect(got[i].span.n == want[i].n, std::string(what) + ": extent of " + got[i].name + " = " + std::to_string(got[i].span.n) + ", by hand " + std::to_string(want[i].n));
    }
    expect(need == want_need, std::string(what) + ": need = " + std::to_string(need) + ", by hand " + std::to_string(want_need));
    expect_tiling(what, got, need);
}

// up of every region, then down of every region, over a heap buffer of exactly `need` elements; every host array is on the heap at its
// exact size, so that the sanitizer build sees a copy that runs past either end
template <class T>
void round_trip(const char* what, const std::vector<Named>& spans, size_t need) {
    const std::unique_ptr<T[]> device(new T[need]);
    std::vector<char> written(need, 0);
    for (size_t i = 0; i < need; ++i) device[i] = (T)-1;
    bool ok = true;
    PlantCopier<PlantHostCopy> copy{{}, ok};
    std::vector<std::unique_ptr<T[]>> in, out;
    int tag = 1;
    for (const Named& s : spans) {
        in.emplace_back(new T[s.span.n]);
        for (size_t i = 0; i < s.span.n; ++i) in.back()[i] = (T)(1000 * tag + (int)i);
        ++tag;
        copy.up(device.get(), s.span, (const T*)in.back().get());
        for (size_t i = 0; i < s.span.n; ++i) written[s.span.at + i]++;
        expect(s.span.or_null(device.get()) == (s.span.n ? device.get() + s.span.at : nullptr), std::string(what) + ": or_null of " + s.name);
        expect(s.span.on(device.get()) == device.get() + s.span.at, std::string(what) + ": on of " + s.name);
    }
    for (size_t i = 0; i < need; ++i) expect(written[i] == 1, std::string(what) + ": an element that is not in exactly one region");
    for (const Named& s : spans) {
        out.emplace_back(new T[s.span.n]);
        copy.down(out.back().get(), (const T*)device.get(), s.span);
    }
    expect(ok, std::string(what) + ": the copier's flag");
    for (size_t r = 0; r < spans.size(); ++r)
        for (size_t i = 0; i < spans[r].span.n; ++i) expect(out[r][i] == in[r][i], std::string(what) + ": " + spans[r].name + " does not come back as it went up");
}

void check_cursor_and_copier() {
    PlantCursor at;
    const PlantSpan a = at.take(3), none = at.take(0), b = at.take(5), c = at.take(1);
    expect(a.at == 0 && a.n == 3 && none.at == 3 && none.n == 0 && b.at == 3 && b.n == 5 && c.at == 8 && c.n == 1, "take lays regions end to end");
    expect(at.end() == 9, "end() is the sum");
    expect(at.end() == 0 && at.take(2).at == 0, "end() starts over");
    double base[1];
    expect(none.or_null(base) == nullptr && a.or_null(base) == base && b.on(base) == base + 3, "or_null is null for an absent region alone");
    const PlantSpan p = b.part(1, 3);
    expect(p.at == 4 && p.n == 3 && b.part(0, 5).n == 5 && b.part(5, 0).at == 8, "part is [from, from + cnt) of the region");
    round_trip<double>("cursor", {{"a", a}, {"none", none}, {"b", b}, {"c", c}}, 9);
    round_trip<int>("cursor, ints", {{"a", a}, {"none", none}, {"b", b}, {"c", c}}, 9);
    // zero-count and null-host copies touch nothing, in either direction, and leave the flag alone
    const std::unique_ptr<double[]> device(new double[4]), host(new double[4]);
    for (int i = 0; i < 4; ++i) { device[i] = 7.0; host[i] = 9.0; }
    bool ok = true;
    PlantCopier<PlantHostCopy> copy{{}, ok};
    copy.up(device.get(), PlantSpan{1, 0}, (const double*)host.get());
    copy.up(device.get(), PlantSpan{0, 4}, (const double*)nullptr);
    copy.down(host.get(), (const double*)device.get(), PlantSpan{1, 0});
    copy.down((double*)nullptr, (const double*)device.get(), PlantSpan{0, 4});
    for (int i = 0; i < 4; ++i) expect(device[i] == 7.0 && host[i] == 9.0, "a zero-count or null-host copy wrote something");
    expect(ok, "a copy that copies nothing cleared the flag");
    // a failed primitive clears the flag, and nothing is copied after it
    struct Failing { int* calls; bool operator()(void*, const void*, size_t, bool) const { ++*calls; return false; } };
    int calls = 0;
    bool bad = true;
    PlantCopier<Failing> failing{{&calls}, bad};
    failing.up(device.get(), PlantSpan{0, 4}, (const double*)host.get());
    failing.up(device.get(), PlantSpan{0, 4}, (const double*)host.get());
    failing.down(host.get(), (const double*)device.get(), PlantSpan{0, 4});
    expect(!bad && calls == 1, "a failure is latched and ends the copies");
}

PlantModel hopper() {
    PlantModel M{};
    expect(plant_model_by_id(CIMPC_PLANT_HOPPER_2D, &M), "hopper_2D is a model");
    expect(M.nq == 4 && M.nu == 2 && M.nc == 1 && M.nb() == 2 && M.nz() == 12 && M.nw == 2, "hopper_2D's sizes are the ones the offsets below are worked out for");
    return M;
}

std::vector<Named> cost_spans(const PlantCostSpans& c) { return {{"Q", c.Q}, {"Qf", c.Qf}, {"R", c.R}, {"x_goal", c.x_goal}, {"u_goal", c.u_goal}}; }

// cimpc_plant_tape_linesearch[_box]: B = 2, T = 4, n_alpha = 2, K_w = 2, a cost with n_Q = n_R = n_x = 1.  By hand, with n = 8, kk = 16,
// TB = 8, NB = 4:  q_nom 6 x 2 x 4 = 48 | u_nom 16 | k 16 | K 128 | w K_w B nw = 8 | mu B = 2 | dV 4 | J_nom 2 | alpha 2 | Q 64 | Qf 64 | R 4 |
// x_goal 5 x 8 = 40 | u_goal 4 x 2 = 8 | u_lo, u_hi n_lim x 2 each.
void check_linesearch_layout(const PlantModel& M) {
    const PlantCost C{nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, 4, 4, 2};
    struct Case { const char* name; bool w_each, mu_each, limits; int n_lim; std::vector<PlantSpan> in; size_t need_in; };
    const std::vector<Case> cases = {
        {"linesearch, w shared or none, mu shared, no limits", false, false, false, 1,
         {{0, 48}, {48, 16}, {64, 16}, {80, 128}, {208, 0}, {208, 0}, {208, 4}, {212, 2}, {214, 2}, {216, 64}, {280, 64}, {344, 4}, {348, 40}, {388, 8}, {396, 0}, {396, 0}}, 396},
        {"linesearch, w per robot, mu per robot, one row of limits", true, true, true, 1,
         {{0, 48}, {48, 16}, {64, 16}, {80, 128}, {208, 8}, {216, 2}, {218, 4}, {222, 2}, {224, 2}, {226, 64}, {290, 64}, {354, 4}, {358, 40}, {398, 8}, {406, 2}, {408, 2}}, 410},
        {"linesearch, w per robot, mu shared, limits per robot", true, false, true, 2,
         {{0, 48}, {48, 16}, {64, 16}, {80, 128}, {208, 8}, {216, 0}, {216, 4}, {220, 2}, {222, 2}, {224, 64}, {288, 64}, {352, 4}, {356, 40}, {396, 8}, {404, 4}, {408, 4}}, 412},
        {"linesearch, w shared or none, mu per robot, no limits", false, true, false, 1,
         {{0, 48}, {48, 16}, {64, 16}, {80, 128}, {208, 0}, {208, 2}, {210, 4}, {214, 2}, {216, 2}, {218, 64}, {282, 64}, {346, 4}, {350, 40}, {390, 8}, {398, 0}, {398, 0}}, 398},
    };
    for (const Case& c : cases) {
        const PlantLsLayout L = plant_linesearch_layout(M, C, PlantLsShape{2, 4, 2, 2, c.n_lim, c.w_each, c.mu_each, c.limits});
        std::vector<Named> in = {{"q_nom", L.q_nom}, {"u_nom", L.u_nom}, {"k", L.k}, {"K", L.K}, {"w", L.w}, {"mu", L.mu}, {"dV", L.dV}, {"J_nom", L.J_nom}, {"alpha", L.alpha}};
        for (const Named& s : cost_spans(L.cost)) in.push_back(s);
        in.push_back({"u_lo", L.u_lo}); in.push_back({"u_hi", L.u_hi});
        expect_spans(c.name, in, c.in, L.need_in, c.need_in);
        double base[1];
        expect((L.w.or_null(base) != nullptr) == c.w_each && (L.mu.or_null(base) != nullptr) == c.mu_each && (L.u_lo.or_null(base) != nullptr) == c.limits &&
               (L.u_hi.or_null(base) != nullptr) == c.limits, std::string(c.name) + ": or_null is null exactly for the absent arrays");
        // d_out: J NB = 4 | q 48 | u_applied 16 | gamma TB nc = 8 | b TB nb = 16 | lin_q 5 x 2 x 8 = 80 | lin_r 16 | z TB nz = 96
        const std::vector<Named> out = {{"J", L.J}, {"q", L.q}, {"u_applied", L.u_applied}, {"gamma", L.gamma}, {"b", L.b}, {"lin_q", L.lin_q}, {"lin_r", L.lin_r}, {"z", L.z}};
        expect_spans(c.name, out, {{0, 4}, {4, 48}, {52, 16}, {68, 8}, {76, 16}, {92, 80}, {172, 16}, {188, 96}}, L.need_out, 284);
        // d_int: ok NB = 4 | choice B = 2 | status 8 | iters 8 | conv 4
        const std::vector<Named> ints = {{"ok", L.ok}, {"choice", L.choice}, {"status", L.status}, {"iters", L.iters}, {"conv", L.conv}};
        expect_spans(c.name, ints, {{0, 4}, {4, 2}, {6, 8}, {14, 8}, {22, 4}}, L.need_int, 26);
        round_trip<double>(c.name, in, L.need_in);
        round_trip<double>(c.name, out, L.need_out);
        round_trip<int>(c.name, ints, L.need_int);
    }
}

// cimpc_plant_rollout_segments: B = 2, T = 4, segments = 2 (M B = 4), K_w = 2.  By hand:  nodes M B n = 32 | u TB nu = 16 | w K_w n_w nw |
// mu B | with a cost Q 64 | Qf 64 | R 4 | x_goal 40 | u_goal 8.
void check_segments_layout(const PlantModel& M) {
    const PlantCost C{nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, 4, 4, 2};
    struct Case { const char* name; bool has_w; int n_w; bool mu_each, cost; std::vector<PlantSpan> in; size_t need_in; };
    const std::vector<Case> cases = {
        {"segments, no w, mu shared, no cost", false, 1, false, false,
         {{0, 32}, {32, 16}, {48, 0}, {48, 0}, {48, 0}, {48, 0}, {48, 0}, {48, 0}, {48, 0}}, 48},
        {"segments, w per robot, mu per robot, a cost", true, 2, true, true,
         {{0, 32}, {32, 16}, {48, 8}, {56, 2}, {58, 64}, {122, 64}, {186, 4}, {190, 40}, {230, 8}}, 238},
        {"segments, w shared, mu shared, a cost", true, 1, false, true,
         {{0, 32}, {32, 16}, {48, 4}, {52, 0}, {52, 64}, {116, 64}, {180, 4}, {184, 40}, {224, 8}}, 232},
        {"segments, no w, mu per robot, no cost", false, 1, true, false,
         {{0, 32}, {32, 16}, {48, 0}, {48, 2}, {50, 0}, {50, 0}, {50, 0}, {50, 0}, {50, 0}}, 50},
    };
    for (const Case& c : cases) {
        const PlantSegmentsLayout L = plant_segments_layout(M, c.cost ? C : PlantCost{}, PlantSegmentsShape{2, 4, 2, 2, c.n_w, c.has_w, c.mu_each, c.cost});
        std::vector<Named> in = {{"nodes", L.nodes}, {"u", L.u}, {"w", L.w}, {"mu", L.mu}};
        for (const Named& s : cost_spans(L.cost)) in.push_back(s);
        expect_spans(c.name, in, c.in, L.need_in, c.need_in);
        double base[1];
        expect((L.w.or_null(base) != nullptr) == c.has_w && (L.mu.or_null(base) != nullptr) == c.mu_each && (L.cost.Q.or_null(base) != nullptr) == c.cost,
               std::string(c.name) + ": or_null is null exactly for the absent arrays");
        // d_out: gamma TB nc = 8 | b TB nb = 16 | defects (M - 1) B n = 16 | D 2 | J 2 | lt (T + 1) B = 10 | lin_q 80 | lin_r 16
        const std::vector<Named> out = {{"gamma", L.gamma}, {"b", L.b}, {"defects", L.defects}, {"D", L.D}, {"J", L.J}, {"lt", L.lt}, {"lin_q", L.lin_q}, {"lin_r", L.lin_r}};
        expect_spans(c.name, out, {{0, 8}, {8, 16}, {24, 16}, {40, 2}, {42, 2}, {44, 10}, {54, 80}, {134, 16}}, L.need_out, 150);
        const std::vector<Named> ints = {{"status", L.status}, {"iters", L.iters}};
        expect_spans(c.name, ints, {{0, 8}, {8, 8}}, L.need_int, 16);
        round_trip<double>(c.name, in, L.need_in);
        round_trip<double>(c.name, out, L.need_out);
        round_trip<int>(c.name, ints, L.need_int);
    }
    // one segment: no node to close, so no defect and no room for one
    const PlantSegmentsLayout one = plant_segments_layout(M, PlantCost{}, PlantSegmentsShape{2, 4, 1, 2, 1, false, false, false});
    expect(one.nodes.n == 16 && one.defects.n == 0 && one.D.at == one.defects.at && one.need_out == 134, "segments = 1 has no defects");
}

// plant_cost_up through the memcpy copier: the five arrays land in their regions and the returned cost points at them
void check_cost_upload() {
    const int T = 3, nq = 2, nu = 1, n = 4;
    std::vector<double> Q(2 * n * n, 1.0), Qf(n * n, 2.0), R(1, 3.0), xg((T + 1) * 2 * n, 4.0), ug(T * 2 * nu, 5.0);
    const PlantCost host{Q.data(), Qf.data(), R.data(), xg.data(), ug.data(), 2, 1, 2, T, nq, nu};
    PlantCursor at;
    const PlantSpan lead = at.take(3);
    const PlantCostSpans s = plant_cost_spans(at, host);
    const size_t need = at.end();
    expect(lead.n == 3 && s.Q.at == 3 && s.Q.n == 32 && s.Qf.at == 35 && s.Qf.n == 16 && s.R.at == 51 && s.R.n == 1 && s.x_goal.at == 52 && s.x_goal.n == 32 &&
           s.u_goal.at == 84 && s.u_goal.n == 6 && need == 90, "the cost's regions by hand");
    const std::unique_ptr<double[]> device(new double[need]);
    for (size_t i = 0; i < need; ++i) device[i] = 0.0;
    bool ok = true;
    PlantCopier<PlantHostCopy> copy{{}, ok};
    const PlantCost dev = plant_cost_up(copy, device.get(), s, host);
    expect(ok && dev.Q == device.get() + 3 && dev.Qf == device.get() + 35 && dev.R == device.get() + 51 && dev.x_goal == device.get() + 52 &&
           dev.u_goal == device.get() + 84, "the returned cost points into the buffer");
    expect(dev.n_Q == 2 && dev.n_R == 1 && dev.n_x == 2 && dev.T == T && dev.nq == nq && dev.nu == nu, "the returned cost keeps its sizes");
    double want = 0.0;
    for (size_t i = 0; i < need; ++i) {
        want = i < 3 ? 0.0 : i < 35 ? 1.0 : i < 51 ? 2.0 : i < 52 ? 3.0 : i < 84 ? 4.0 : 5.0;
        expect(device[i] == want, "the cost's arrays land in their regions");
    }
    at = PlantCursor{};
    const PlantCostSpans none = plant_cost_spans(at, host, false);
    expect(at.end() == 0 && none.Q.n == 0 && none.u_goal.n == 0, "a call without a cost takes no room");
    const cimpc_tracking_cost c{Q.data(), Qf.data(), R.data(), xg.data(), ug.data(), 2, 1, 2};
    const PlantCost of = plant_cost_of(c, T, nq, nu);
    expect(of.Q == host.Q && of.Qf == host.Qf && of.R == host.R && of.x_goal == host.x_goal && of.u_goal == host.u_goal && of.n_Q == 2 && of.n_R == 1 &&
           of.n_x == 2 && of.T == T && of.nq == nq && of.nu == nu, "plant_cost_of");
}

void check_refusals() {
    int a = 0;
    {      // cimpc_plant_ilqr refuses a null new_tape before it looks at anything else
        expect(plant_refuse("cimpc_plant_ilqr", "null new_tape") == CIMPC_ERR_INVALID, "plant_refuse returns CIMPC_ERR_INVALID");
        expect(g_error == "cimpc_plant_ilqr: null new_tape", "cimpc_plant_ilqr's refusal, got '" + g_error + "'");
    }
    {      // cimpc_plant_tape_linesearch names the first null of its list, in the list's order
        const PlantRequired required[] = {{"tape", &a}, {"q_nom", &a}, {"u_nom", &a}, {"mu", &a}, {"opts", &a}, {"K", nullptr}, {"k", nullptr}, {"dV", &a}};
        const char* name = plant_first_null(required);
        expect(name && std::string(name) == "K", "the first null in the order of the list");
        (void)plant_refuse("cimpc_plant_tape_linesearch", std::string("null ") + name);
        expect(g_error == "cimpc_plant_tape_linesearch: null K", "cimpc_plant_tape_linesearch's refusal, got '" + g_error + "'");
    }
    {      // cimpc_plant_mpc_control
        const PlantRequired required[] = {{"handle", &a}, {"q0", &a}, {"q1", nullptr}, {"u", &a}};
        (void)plant_refuse("cimpc_plant_mpc_control", std::string("null ") + plant_first_null(required));
        expect(g_error == "cimpc_plant_mpc_control: null q1", "cimpc_plant_mpc_control's refusal, got '" + g_error + "'");
        (void)plant_refuse("cimpc_plant_mpc_control", "a handle that met a HIP error refuses further use");
        expect(g_error == "cimpc_plant_mpc_control: a handle that met a HIP error refuses further use", "the latched handle's refusal");
    }
    const PlantRequired all[] = {{"x", &a}, {"y", &a}};
    expect(plant_first_null(all) == nullptr, "no null among the required");
    const std::unique_ptr<double[]> v(new double[3]);
    v[0] = 1.0; v[1] = -2.0; v[2] = 0.0;
    expect(plant_all_finite(v.get(), 3) && plant_all_finite(nullptr, 0), "finite arrays, and an empty one that is never read");
    v[2] = INFINITY;
    expect(!plant_all_finite(v.get(), 3) && plant_all_finite(v.get(), 2), "an infinity, and the count that stops before it");
    v[1] = NAN;
    expect(!plant_all_finite(v.get(), 2), "a NaN");
}

}  // namespace

int main() {
    check_cursor_and_copier();
    const PlantModel M = hopper();
    check_linesearch_layout(M);
    check_segments_layout(M);
    check_cost_upload();
    check_refusals();
    std::printf("ok %d\n", g_checks);
    return 0;
}
