// csrc/plant_tangent.h on the host with a team of one: the statements plant_tangent_kernel runs, on blocks and tangents read from stdin
// (tests/test_plant_tangent.py).  Numbers travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_tangent_check plan nr n_cols nq nu feedback      prints plant_tangent_group and the LDS bytes of a group of that size
//   plant_tangent_check                                     the chain:
//   in:  B T nq nu nw nc nb n_cols n_dir group (0: the plan's) K_f n_f hold_f (K_f = 0: an open-loop tape) n_sample
//        has_dq0 has_dq1 has_du has_dw has_dmu has_dh has_dxref, status (T B), dz (T B nr n_cols, column-major blocks),
//        K (K_f n_f nu 2nq, column-major blocks), the tangents given, each with its leading axis of n_dir
//   out: one line each - dq, dgamma, db, du_applied (empty on an open-loop tape), n_cut
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

static void print_doubles(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%a ", v[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc == 7 && std::strcmp(argv[1], "plan") == 0) {
        const int nr = std::atoi(argv[2]), n_cols = std::atoi(argv[3]), nq = std::atoi(argv[4]), nu = std::atoi(argv[5]);
        const bool fb = std::atoi(argv[6]) != 0;
        const int g = plant_tangent_group(nr, n_cols, nq, nu, fb);
        std::printf("%d %zu %d\n", g, plant_tangent_lds(nr, n_cols, nq, nu, fb, g), g >= 1 && plant_tangent_fits(nr, n_cols, nq, nu, fb, g) ? 1 : 0);
        return 0;
    }
    int B, T, nq, nu, nw, nc, nb, n_cols, n_dir, group, K_f, n_f, hold_f, has[7];
    char ns_tok[64];
    if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %63s", &B, &T, &nq, &nu, &nw, &nc, &nb, &n_cols, &n_dir, &group, &K_f, &n_f, &hold_f, ns_tok) != 14) return 2;
    for (int& h : has) if (std::scanf("%d", &h) != 1) return 2;
    const bool fb = K_f > 0;
    const int nr = nq + nc + nb;
    const size_t TB = (size_t)T * B, nD = (size_t)n_dir;
    std::vector<int> status(TB);
    for (size_t i = 0; i < TB; ++i) if (std::scanf("%d", &status[i]) != 1) return 2;
    const std::vector<double> dz = read_doubles(TB * nr * n_cols);
    const std::vector<double> K = read_doubles(fb ? (size_t)K_f * n_f * nu * 2 * nq : 0);
    const std::vector<double> dq0 = read_doubles(has[0] ? nD * B * nq : 0), dq1 = read_doubles(has[1] ? nD * B * nq : 0),
                              du = read_doubles(has[2] ? nD * TB * nu : 0), dw = read_doubles(has[3] ? nD * TB * nw : 0),
                              dmu = read_doubles(has[4] ? nD * B : 0), dh = read_doubles(has[5] ? nD * B : 0),
                              dxref = read_doubles(has[6] ? nD * TB * 2 * nq : 0);
    std::vector<double> dq(nD * (T + 2) * B * nq), dgamma(nD * TB * nc), db(nD * TB * nb), du_applied(fb ? nD * TB * nu : 0);
    std::vector<int> n_cut(B, -1);
    auto in = [](const std::vector<double>& v, int given) { return given ? v.data() : nullptr; };
    PlantTangent P{dz.data(), status.data(), in(dq0, has[0]), in(dq1, has[1]), in(du, has[2]), in(dw, has[3]), in(dmu, has[4]), in(dh, has[5]),
                   dq.data(), dgamma.data(), db.data(), n_cut.data(), B, T, nq, nu, nw, nc, nb, n_cols, n_dir};
    if (fb) {
        P.fb = PlantFeedback{K.data(), nullptr, K_f, n_f, hold_f, std::strtod(ns_tok, nullptr)};
        P.dxref_step = in(dxref, has[6]);
        P.du_applied = du_applied.data();
    }
    if (group == 0) group = plant_tangent_group(nr, n_cols, nq, nu, fb);
    if (group < 1) return 3;
    for (int rb = 0; rb < B; ++rb)
        for (int d0 = 0; d0 < n_dir; d0 += group) {
            const int nd = n_dir - d0 < group ? n_dir - d0 : group;
            std::vector<double> work(plant_tangent_work_doubles(nr, n_cols, nq, nu, fb, nd));      // exactly what the kernel's LDS holds: ASan guards its ends
            PlantTangentSolo team;
            plant_tangent_chain(P, rb, d0, nd, work.data(), team);
        }
    print_doubles(dq); print_doubles(dgamma); print_doubles(db); print_doubles(du_applied);
    for (int rb = 0; rb < B; ++rb) std::printf("%d ", n_cut[rb]);
    std::printf("\n");
    return 0;
}
