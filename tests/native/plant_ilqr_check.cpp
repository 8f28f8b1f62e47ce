// csrc/plant_ilqr.h on the host: the statements the kernels of plant_ilqr.hip run, on numbers read from stdin (tests/test_plant_ilqr.py).
// Numbers travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_ilqr_check rules    in:  N n_ladder n_alpha, rho_max tol, ladder (n_ladder), alpha (n_alpha), then N states:
//                                  level active J choice lq_status J_cand (n_alpha)
//                             out: N lines - rho J_nom level' active' J' | the history row: J alpha rho accepted
//   plant_ilqr_check valid    in:  max_iter n_ladder rho_max tol, ladder (n_ladder; none for n_ladder < 1)
//                             out: plant_ilqr_refusal's reason, or ok
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_ilqr.h"

static double read_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) std::exit(2);
    return std::strtod(tok, nullptr);
}

static std::vector<double> read_doubles(size_t n) {
    std::vector<double> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = read_double();
    return v;
}

static int read_int() {
    int v;
    if (std::scanf("%d", &v) != 1) std::exit(2);
    return v;
}

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc != 2) return 2;
    if (std::strcmp(argv[1], "rules") == 0) {
        const int N = read_int(), n_ladder = read_int(), n_alpha = read_int();
        const double rho_max = read_double(), tol = read_double();
        const std::vector<double> ladder = read_doubles(n_ladder), alpha = read_doubles(n_alpha);      // exact sizes: ASan guards their ends
        for (int i = 0; i < N; ++i) {
            PlantIlqrRobot s{};
            s.level = read_int(); s.active = read_int(); s.J = read_double();
            const int choice = read_int(), lq_status = read_int();
            const std::vector<double> J_cand = read_doubles(n_alpha);
            const double rho = plant_ilqr_rho(ladder.data(), s.level), J_nom = plant_ilqr_nominal_cost(s.active, lq_status, s.J);
            const PlantIlqrRow row = plant_ilqr_update(&s, choice, J_cand.data(), 1, alpha.data(), ladder.data(), rho_max, tol);
            std::printf("%a %a %d %d %a %a %a %a %d\n", rho, J_nom, s.level, s.active, s.J, row.J, row.alpha, row.rho, row.accepted);
        }
        return 0;
    }
    if (std::strcmp(argv[1], "valid") == 0) {
        const int max_iter = read_int(), n_ladder = read_int();
        const double rho_max = read_double(), tol = read_double();
        const std::vector<double> ladder = read_doubles(n_ladder > 0 ? n_ladder : 0);
        const char* why = plant_ilqr_refusal(max_iter, n_ladder, n_ladder > 0 ? ladder.data() : nullptr, rho_max, tol);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    return 2;
}
