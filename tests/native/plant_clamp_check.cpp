// The clamp's derivative on the host with a team of one: plant_feedback_free and plant_feedback_clamped of
// csrc/plant_feedback.h and the masked chains of csrc/plant_adjoint.h and csrc/plant_tangent.h, the statements plant_clamp_mask_kernel,
// plant_adjoint_kernel and plant_tangent_kernel run, on inputs read from stdin (tests/test_plant_clamp.py).  Numbers travel as C
// hexadecimal floats.  A stand-alone program: it is also built with -fsanitize=address,undefined and run directly.
//   plant_clamp_check free        in: n, then n x (u lo hi)                         out: n flags, 1 = free
//   plant_clamp_check words       in: T B nu n_lim, u_applied (T B nu), u_lo, u_hi (n_lim nu)      out: T x B words
//   plant_clamp_check adjoint     in: B T nq nu nw nc nb n_cols has_gq has_ggamma has_gb K_f n_f hold_f n_sample has_mask, status (T B),
//                                     dz (T B nr n_cols, column-major blocks), the cotangents given, K (K_f n_f nu 2nq, column-major blocks),
//                                     the mask (T B words) when has_mask
//                                 out: one line each - g_q0, g_q1, g_u_step, g_w_step, g_mu, g_h (the last three where n_cols reaches them),
//                                     n_cut, g_xref_step
//   plant_clamp_check tangent     in: B T nq nu nw nc nb n_cols n_dir group (0: the plan's) K_f n_f hold_f n_sample has_dq0 has_dq1 has_du
//                                     has_dw has_dmu has_dh has_dxref has_mask, status, dz, K, the mask when has_mask, the tangents given,
//                                     each with its leading axis of n_dir
//                                 out: one line each - dq, dgamma, db, du_applied, n_cut
// has_mask = 0 runs the closed-loop chain without a mask, the instantiation an unlimited tape launches.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_adjoint.h"
#include "../../contactimplicitmpc/jl_amd/csrc/plant_tangent.h"

static std::vector<double> read_doubles(size_t n) {
    std::vector<double> v(n);
    char tok[64];
    for (size_t i = 0; i < n; ++i) {
        if (std::scanf("%63s", tok) != 1) std::exit(2);
        v[i] = std::strtod(tok, nullptr);
    }
    return v;
}

static std::vector<int> read_ints(size_t n) {
    std::vector<int> v(n);
    for (size_t i = 0; i < n; ++i) if (std::scanf("%d", &v[i]) != 1) std::exit(2);
    return v;
}

static void print_doubles(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%a ", v[i]);
    std::printf("\n");
}

static void print_ints(const std::vector<int>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%d ", v[i]);
    std::printf("\n");
}

static int run_free() {
    const int n = read_ints(1)[0];
    const std::vector<double> rows = read_doubles((size_t)3 * n);
    for (int k = 0; k < n; ++k) std::printf("%d ", cimpc::plant_feedback_free(rows[3 * k], rows[3 * k + 1], rows[3 * k + 2]) ? 1 : 0);
    std::printf("\n");
    return 0;
}

// the mask as plant_clamp_mask_kernel writes it: one (step, robot) at a time
static int run_words() {
    using namespace cimpc;
    const std::vector<int> dims = read_ints(4);
    const int T = dims[0], B = dims[1], nu = dims[2], n_lim = dims[3];
    const std::vector<double> ua = read_doubles((size_t)T * B * nu), lo = read_doubles((size_t)n_lim * nu), hi = read_doubles((size_t)n_lim * nu);
    std::vector<int> words((size_t)T * B);
    for (int e = 0; e < T * B; ++e) {
        const int rb = e % B;
        words[e] = plant_feedback_clamped(ua.data() + (size_t)e * nu, plant_feedback_limits(lo.data(), n_lim, rb, nu),
                                          plant_feedback_limits(hi.data(), n_lim, rb, nu), nu);
    }
    print_ints(words);
    return 0;
}

static int run_adjoint() {
    using namespace cimpc;
    const std::vector<int> h = read_ints(14);
    const int B = h[0], T = h[1], nq = h[2], nu = h[3], nw = h[4], nc = h[5], nb = h[6], n_cols = h[7], has_gq = h[8], has_gg = h[9], has_gb = h[10],
              K_f = h[11], n_f = h[12], hold_f = h[13];
    const double n_sample = read_doubles(1)[0];
    const int has_mask = read_ints(1)[0];
    const int nr = nq + nc + nb, c_mu = 2 * nq + nu + nw;
    const size_t TB = (size_t)T * B;
    const std::vector<int> status = read_ints(TB);
    const std::vector<double> dz = read_doubles(TB * nr * n_cols);
    const std::vector<double> gq = read_doubles(has_gq ? (size_t)(T + 2) * B * nq : 0), gg = read_doubles(has_gg ? TB * nc : 0),
                              gb = read_doubles(has_gb ? TB * nb : 0);
    const std::vector<double> K = read_doubles((size_t)K_f * n_f * nu * 2 * nq);
    const std::vector<int> mask = read_ints(has_mask ? TB : 0);
    std::vector<double> g_q0((size_t)B * nq), g_q1((size_t)B * nq), g_u(TB * nu), g_w(n_cols >= c_mu ? TB * nw : 0), g_mu(n_cols > c_mu ? B : 0),
        g_h(n_cols > c_mu + 1 ? B : 0), g_x(TB * 2 * nq);
    std::vector<int> n_cut(B);
    PlantAdjoint P{dz.data(), status.data(), has_gq ? gq.data() : nullptr, has_gg ? gg.data() : nullptr, has_gb ? gb.data() : nullptr,
                   g_q0.data(), g_q1.data(), g_u.data(), n_cols >= c_mu ? g_w.data() : nullptr, n_cols > c_mu ? g_mu.data() : nullptr,
                   n_cols > c_mu + 1 ? g_h.data() : nullptr, n_cut.data(), B, T, nq, nu, nw, nc, nb, n_cols};
    P.fb = PlantFeedback{K.data(), nullptr, K_f, n_f, hold_f, n_sample};      // the chain does not need x_ref
    P.g_xref_step = g_x.data();
    P.clamped = has_mask ? mask.data() : nullptr;
    // exactly what the kernel's LDS holds: the mask adds nothing to it, and a sanitizer guards its ends
    std::vector<double> work(plant_adjoint_work_doubles(nr, n_cols, nq) + plant_adjoint_feedback_doubles(nu, nq));
    for (int rb = 0; rb < B; ++rb) {
        PlantAdjointSolo team;
        plant_adjoint_chain(P, rb, work.data(), team);
    }
    print_doubles(g_q0); print_doubles(g_q1); print_doubles(g_u); print_doubles(g_w); print_doubles(g_mu); print_doubles(g_h);
    print_ints(n_cut);
    print_doubles(g_x);
    return 0;
}

static int run_tangent() {
    using namespace cimpc;
    const std::vector<int> h = read_ints(13);
    const int B = h[0], T = h[1], nq = h[2], nu = h[3], nw = h[4], nc = h[5], nb = h[6], n_cols = h[7], n_dir = h[8], K_f = h[10], n_f = h[11], hold_f = h[12];
    int group = h[9];
    const double n_sample = read_doubles(1)[0];
    const std::vector<int> has = read_ints(8);
    const int nr = nq + nc + nb;
    const size_t TB = (size_t)T * B, nD = (size_t)n_dir;
    const std::vector<int> status = read_ints(TB);
    const std::vector<double> dz = read_doubles(TB * nr * n_cols);
    const std::vector<double> K = read_doubles((size_t)K_f * n_f * nu * 2 * nq);
    const std::vector<int> mask = read_ints(has[7] ? TB : 0);
    const std::vector<double> dq0 = read_doubles(has[0] ? nD * B * nq : 0), dq1 = read_doubles(has[1] ? nD * B * nq : 0),
                              du = read_doubles(has[2] ? nD * TB * nu : 0), dw = read_doubles(has[3] ? nD * TB * nw : 0),
                              dmu = read_doubles(has[4] ? nD * B : 0), dh = read_doubles(has[5] ? nD * B : 0),
                              dxref = read_doubles(has[6] ? nD * TB * 2 * nq : 0);
    std::vector<double> dq(nD * (T + 2) * B * nq), dgamma(nD * TB * nc), db(nD * TB * nb), du_applied(nD * TB * nu);
    std::vector<int> n_cut(B, -1);
    auto in = [](const std::vector<double>& v, int given) { return given ? v.data() : nullptr; };
    PlantTangent P{dz.data(), status.data(), in(dq0, has[0]), in(dq1, has[1]), in(du, has[2]), in(dw, has[3]), in(dmu, has[4]), in(dh, has[5]),
                   dq.data(), dgamma.data(), db.data(), n_cut.data(), B, T, nq, nu, nw, nc, nb, n_cols, n_dir};
    P.fb = PlantFeedback{K.data(), nullptr, K_f, n_f, hold_f, n_sample};
    P.dxref_step = in(dxref, has[6]);
    P.du_applied = du_applied.data();
    P.clamped = has[7] ? mask.data() : nullptr;
    if (group == 0) group = plant_tangent_group(nr, n_cols, nq, nu, true);
    if (group < 1) return 3;
    for (int rb = 0; rb < B; ++rb)
        for (int d0 = 0; d0 < n_dir; d0 += group) {
            const int nd = n_dir - d0 < group ? n_dir - d0 : group;
            std::vector<double> work(plant_tangent_work_doubles(nr, n_cols, nq, nu, true, nd));      // exactly what the kernel's LDS holds
            PlantTangentSolo team;
            plant_tangent_chain(P, rb, d0, nd, work.data(), team);
        }
    print_doubles(dq); print_doubles(dgamma); print_doubles(db); print_doubles(du_applied);
    print_ints(n_cut);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (std::strcmp(argv[1], "free") == 0) return run_free();
    if (std::strcmp(argv[1], "words") == 0) return run_words();
    if (std::strcmp(argv[1], "adjoint") == 0) return run_adjoint();
    if (std::strcmp(argv[1], "tangent") == 0) return run_tangent();
    return 2;
}
