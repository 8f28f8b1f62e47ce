// csrc/plant_adjoint.h on the host with a team of one: the statements plant_adjoint_kernel runs, on blocks and cotangents read from
// stdin (tests/test_plant_adjoint.py).  Numbers travel as C hexadecimal floats, so nothing is rounded on the way.
//   in:  B T nq nu nw nc nb n_cols has_gq has_ggamma has_gb, status (T B), dz (T B nr n_cols, column-major blocks), the cotangents given
//   out: one line per output - g_q0, g_q1, g_u_step, g_w_step, g_mu, g_h (the last three where n_cols reaches them), n_cut
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
    int B, T, nq, nu, nw, nc, nb, n_cols, has_gq, has_gg, has_gb;
    if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d", &B, &T, &nq, &nu, &nw, &nc, &nb, &n_cols, &has_gq, &has_gg, &has_gb) != 11) return 2;
    const int nr = nq + nc + nb, c_mu = 2 * nq + nu + nw;
    const size_t TB = (size_t)T * B;
    std::vector<int> status(TB);
    for (size_t i = 0; i < TB; ++i) if (std::scanf("%d", &status[i]) != 1) return 2;
    const std::vector<double> dz = read_doubles(TB * nr * n_cols);
    const std::vector<double> gq = read_doubles(has_gq ? (size_t)(T + 2) * B * nq : 0), gg = read_doubles(has_gg ? TB * nc : 0),
                              gb = read_doubles(has_gb ? TB * nb : 0);
    std::vector<double> g_q0((size_t)B * nq), g_q1((size_t)B * nq), g_u(TB * nu), g_w(n_cols >= c_mu ? TB * nw : 0), g_mu(n_cols > c_mu ? B : 0),
        g_h(n_cols > c_mu + 1 ? B : 0);
    std::vector<int> n_cut(B);
    const PlantAdjoint P{dz.data(), status.data(), has_gq ? gq.data() : nullptr, has_gg ? gg.data() : nullptr, has_gb ? gb.data() : nullptr,
                         g_q0.data(), g_q1.data(), g_u.data(), n_cols >= c_mu ? g_w.data() : nullptr, n_cols > c_mu ? g_mu.data() : nullptr,
                         n_cols > c_mu + 1 ? g_h.data() : nullptr, n_cut.data(), B, T, nq, nu, nw, nc, nb, n_cols};
    std::vector<double> work(plant_adjoint_work_doubles(nr, n_cols, nq));      // exactly what the kernel's LDS holds: ASan guards its ends
    for (int rb = 0; rb < B; ++rb) {
        PlantAdjointSolo team;
        plant_adjoint_chain(P, rb, work.data(), team);
    }
    print_doubles(g_q0); print_doubles(g_q1); print_doubles(g_u); print_doubles(g_w); print_doubles(g_mu); print_doubles(g_h);
    for (int rb = 0; rb < B; ++rb) std::printf("%d ", n_cut[rb]);
    std::printf("\n");
    return 0;
}
