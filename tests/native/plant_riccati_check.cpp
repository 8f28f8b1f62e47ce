// csrc/plant_riccati.h on the host with a team of one: the statements plant_riccati_kernel runs, on blocks and weights read from stdin
// (tests/test_plant_riccati.py).  Numbers travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_riccati_check plan nq nu      prints the LDS bytes of a robot's chain and whether it fits a CU
//   plant_riccati_check                 the chain:
//   in:  B T nq nu nr n_cols laps n_Q n_R n_keep lin (1: q and r follow) rho
//        status (T B), dz (T B nr n_cols, column-major blocks), Q (n_Q n n), Qf (n n), R (n_R m m), q ((T+1) B n), r (T B m)
//   out: one line each - K, k, P0, p0, dV (k, p0, dV empty without q, r), status, n_cut
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_riccati.h"

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

static void print_ints(const std::vector<int>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%d ", v[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc == 4 && std::strcmp(argv[1], "plan") == 0) {
        const int nq = std::atoi(argv[2]), nu = std::atoi(argv[3]);
        std::printf("%zu %d\n", plant_riccati_lds(nq, nu), plant_riccati_fits(nq, nu) ? 1 : 0);
        return 0;
    }
    int B, T, nq, nu, nr, n_cols, laps, n_Q, n_R, n_keep, lin;
    char rho_tok[64];
    if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %63s", &B, &T, &nq, &nu, &nr, &n_cols, &laps, &n_Q, &n_R, &n_keep, &lin, rho_tok) != 12) return 2;
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, m = (size_t)nu;
    std::vector<int> tape_status(TB);
    for (size_t i = 0; i < TB; ++i) if (std::scanf("%d", &tape_status[i]) != 1) return 2;
    const std::vector<double> dz = read_doubles(TB * nr * n_cols), Q = read_doubles(n_Q * n * n), Qf = read_doubles(n * n), R = read_doubles(n_R * m * m),
                              q = read_doubles(lin ? (size_t)(T + 1) * B * n : 0), r = read_doubles(lin ? TB * m : 0);
    // every output starts from a value the chain never writes, so a hole shows
    std::vector<double> K((size_t)n_keep * B * m * n, -7.0), k(lin ? (size_t)n_keep * B * m : 0, -7.0), P0(B * n * n, -7.0), p0(lin ? B * n : 0, -7.0),
        dV(lin ? (size_t)B * 2 : 0, -7.0);
    std::vector<int> status(B, -1), n_cut(B, -1);
    PlantRiccati L{dz.data(), tape_status.data(), Q.data(), Qf.data(), R.data(), lin ? q.data() : nullptr, lin ? r.data() : nullptr,
                   K.data(), lin ? k.data() : nullptr, P0.data(), lin ? p0.data() : nullptr, lin ? dV.data() : nullptr,
                   status.data(), n_cut.data(), B, T, nq, nu, nr, n_cols, laps, n_Q, n_R, n_keep, std::strtod(rho_tok, nullptr)};
    if (!plant_riccati_fits(nq, nu)) return 3;
    for (int rb = 0; rb < B; ++rb) {
        std::vector<double> work(plant_riccati_work_doubles(nq, nu));      // exactly what the kernel's LDS holds: ASan guards its ends
        PlantRiccatiSolo team;
        plant_riccati_chain(L, rb, work.data(), team);
    }
    print_doubles(K); print_doubles(k); print_doubles(P0); print_doubles(p0); print_doubles(dV);
    print_ints(status); print_ints(n_cut);
    return 0;
}
