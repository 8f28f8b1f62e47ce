// csrc/plant_feedback.h and the closed-loop chain of csrc/plant_adjoint.h on the host with a team of one: the statements the step kernel
// and plant_adjoint_kernel run, on inputs read from stdin (tests/test_plant_feedback.py).  Numbers travel as C hexadecimal floats.
//   in:  B T nq nu nw nc nb n_cols has_gq has_ggamma has_gb K_f n_f hold_f n_sample, status (T B), dz (T B nr n_cols, column-major
//        blocks), the cotangents given, K (K_f n_f nu 2nq, column-major blocks), x_ref (K_f n_f 2nq), q ((T + 2) B nq), ubar (T B nu)
//   out: one line per output - g_q0, g_q1, g_u_step, g_w_step, g_mu, g_h (the last three where n_cols reaches them), n_cut,
//        g_xref_step; then the law on the trajectory q: u_applied (T B nu), fb_err (T B 2nq)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_adjoint.h"

static std::vector<double> read_doubles(size_t n) {
    std::vector<double> v(n);
    char tok[64];
    for (size_t i = 0; i < n; ++i) {
        if (std::scanf("%63s", tok) != 1) std::exit(2);
        v[i] = std::strtod(tok, nullptr);
    }
    return v;
}

static void print_doubles(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%a ", v[i]);
    std::printf("\n");
}

int main() {
    using namespace cimpc;
    int B, T, nq, nu, nw, nc, nb, n_cols, has_gq, has_gg, has_gb, K_f, n_f, hold_f;
    if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &B, &T, &nq, &nu, &nw, &nc, &nb, &n_cols, &has_gq, &has_gg, &has_gb, &K_f, &n_f,
                   &hold_f) != 14)
        return 2;
    const double n_sample = read_doubles(1)[0];
    const int nr = nq + nc + nb, c_mu = 2 * nq + nu + nw;
    const size_t TB = (size_t)T * B;
    std::vector<int> status(TB);
    for (size_t i = 0; i < TB; ++i) if (std::scanf("%d", &status[i]) != 1) return 2;
    const std::vector<double> dz = read_doubles(TB * nr * n_cols);
    const std::vector<double> gq = read_doubles(has_gq ? (size_t)(T + 2) * B * nq : 0), gg = read_doubles(has_gg ? TB * nc : 0),
                              gb = read_doubles(has_gb ? TB * nb : 0);
    const std::vector<double> K = read_doubles((size_t)K_f * n_f * nu * 2 * nq), x_ref = read_doubles((size_t)K_f * n_f * 2 * nq),
                              q = read_doubles((size_t)(T + 2) * B * nq), ubar = read_doubles(TB * nu);
    std::vector<double> g_q0((size_t)B * nq), g_q1((size_t)B * nq), g_u(TB * nu), g_w(n_cols >= c_mu ? TB * nw : 0), g_mu(n_cols > c_mu ? B : 0),
        g_h(n_cols > c_mu + 1 ? B : 0), g_x(TB * 2 * nq);
    std::vector<int> n_cut(B);
    PlantAdjoint P{dz.data(), status.data(), has_gq ? gq.data() : nullptr, has_gg ? gg.data() : nullptr, has_gb ? gb.data() : nullptr,
                   g_q0.data(), g_q1.data(), g_u.data(), n_cols >= c_mu ? g_w.data() : nullptr, n_cols > c_mu ? g_mu.data() : nullptr,
                   n_cols > c_mu + 1 ? g_h.data() : nullptr, n_cut.data(), B, T, nq, nu, nw, nc, nb, n_cols};
    P.fb = PlantFeedback{K.data(), x_ref.data(), K_f, n_f, hold_f, n_sample};
    P.g_xref_step = g_x.data();
    // exactly what the kernel's LDS holds with a feedback schedule: a sanitizer guards its ends
    std::vector<double> work(plant_adjoint_work_doubles(nr, n_cols, nq) + plant_adjoint_feedback_doubles(nu, nq));
    for (int rb = 0; rb < B; ++rb) {
        PlantAdjointSolo team;
        plant_adjoint_chain(P, rb, work.data(), team);
    }
    print_doubles(g_q0); print_doubles(g_q1); print_doubles(g_u); print_doubles(g_w); print_doubles(g_mu); print_doubles(g_h);
    for (int rb = 0; rb < B; ++rb) std::printf("%d ", n_cut[rb]);
    std::printf("\n");
    print_doubles(g_x);
    // the law, as the step kernel runs it: the errors of a step first, then every control from them
    std::vector<double> u_applied(TB * nu), fb_err(TB * 2 * nq);
    for (int t = 0; t < T; ++t)
        for (int rb = 0; rb < B; ++rb) {
            const size_t row = (size_t)t * B + rb;
            const double* q0 = &q[row * nq];
            const double* q1 = &q[((size_t)(t + 1) * B + rb) * nq];
            double* e = &fb_err[row * 2 * nq];
            for (int j = 0; j < 2 * nq; ++j) e[j] = plant_feedback_error(plant_feedback_target(P.fb, t, rb, nq), q0, q1, nq, n_sample, j);
            for (int i = 0; i < nu; ++i) u_applied[row * nu + i] = plant_feedback_control(plant_feedback_gain(P.fb, t, rb, nu, nq), e, nu, nq, i, ubar[row * nu + i]);
        }
    print_doubles(u_applied); print_doubles(fb_err);
    return 0;
}
