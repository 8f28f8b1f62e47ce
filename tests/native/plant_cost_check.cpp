// csrc/plant_cost.h on the host with a team of one: the statements the kernels of plant_linesearch.hip run, on numbers read from stdin
// (tests/test_plant_linesearch.py).  Numbers travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_cost_check cost      in:  B T nq nu n_Q n_R n_x, q ((T+2) B nq), u (T B nu), Q (n_Q n n), Qf (n n), R (n_R m m), x_goal ((T+1) n_x n),
//                                   u_goal (T n_x m)                      out: one line each - J, lin_q, lin_r
//   plant_cost_check accept    in:  n_alpha B armijo, alpha (n_alpha), converged (n_alpha B), J (n_alpha B), J_nom (B), dV (B 2)
//                              out: ok (n_alpha B), choice (B)
//   plant_cost_check control   in:  n, then n triples u_nom alpha k    out: n controls
//   plant_cost_check valid     in:  n_alpha armijo B T, alpha (n_alpha)   out: plant_linesearch_refusal's reason or ok; plant_linesearch_fits, 1 or 0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_cost.h"

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

static void print_doubles(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%a ", v[i]);
    std::printf("\n");
}

static void print_ints(const std::vector<int>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%d ", v[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc != 2) return 2;
    if (std::strcmp(argv[1], "cost") == 0) {
        const int B = read_int(), T = read_int(), nq = read_int(), nu = read_int(), n_Q = read_int(), n_R = read_int(), n_x = read_int();
        const size_t n = (size_t)2 * nq, m = (size_t)nu;
        const std::vector<double> q = read_doubles((size_t)(T + 2) * B * nq), u = read_doubles((size_t)T * B * m), Q = read_doubles(n_Q * n * n),
                                  Qf = read_doubles(n * n), R = read_doubles(n_R * m * m), xg = read_doubles((size_t)(T + 1) * n_x * n),
                                  ug = read_doubles((size_t)T * n_x * m);
        const PlantCost C{Q.data(), Qf.data(), R.data(), xg.data(), ug.data(), n_Q, n_R, n_x, T, nq, nu};
        if (!plant_cost_valid(C, B)) return 3;
        // every output starts from a value the chain never writes, so a hole shows
        std::vector<double> J(B, -7.0), lin_q((size_t)(T + 1) * B * n, -7.0), lin_r((size_t)T * B * m, -7.0);
        for (int b = 0; b < B; ++b) {
            std::vector<double> work(plant_cost_work_doubles(nq, nu));      // exactly what a workgroup's LDS is given: ASan guards its ends
            PlantCostSolo team;
            J[b] = plant_cost_trajectory(C, n_x == 1 ? 0 : b, q.data() + (size_t)b * nq, (size_t)B * nq, u.data() + b * m, B * m, work.data(),
                                         lin_q.data() + b * n, B * n, lin_r.data() + b * m, B * m, team);
        }
        print_doubles(J); print_doubles(lin_q); print_doubles(lin_r);
        return 0;
    }
    if (std::strcmp(argv[1], "accept") == 0) {
        const int n_alpha = read_int(), B = read_int();
        const double armijo = read_double();
        const std::vector<double> alpha = read_doubles(n_alpha);
        std::vector<int> conv((size_t)n_alpha * B), ok((size_t)n_alpha * B), choice(B);
        for (auto& c : conv) c = read_int();
        const std::vector<double> J = read_doubles((size_t)n_alpha * B), J_nom = read_doubles(B), dV = read_doubles((size_t)2 * B);
        for (int b = 0; b < B; ++b) {
            for (int c = 0; c < n_alpha; ++c)
                ok[(size_t)c * B + b] = plant_candidate_acceptable(conv[(size_t)c * B + b] != 0, J[(size_t)c * B + b], J_nom[b], armijo, alpha[c], dV[2 * b], dV[2 * b + 1]);
            choice[b] = plant_linesearch_choice(J.data() + b, (size_t)B, ok.data() + b, (size_t)B, n_alpha);
        }
        print_ints(ok); print_ints(choice);
        return 0;
    }
    if (std::strcmp(argv[1], "control") == 0) {
        const int n = read_int();
        std::vector<double> out(n);
        for (int i = 0; i < n; ++i) {
            const double u = read_double(), a = read_double(), k = read_double();
            out[i] = plant_candidate_control(u, a, k);
        }
        print_doubles(out);
        return 0;
    }
    if (std::strcmp(argv[1], "valid") == 0) {
        const int n_alpha = read_int();
        const double armijo = read_double();
        const int B = read_int(), T = read_int();
        const std::vector<double> alpha = read_doubles(n_alpha > 0 && n_alpha <= 1024 ? n_alpha : 0);
        const char* why = plant_linesearch_refusal(n_alpha, alpha.empty() ? &armijo : alpha.data(), armijo);
        std::printf("%s\n%d\n", why ? why : "ok", plant_linesearch_fits(n_alpha, B, T) ? 1 : 0);
        return 0;
    }
    return 2;
}
