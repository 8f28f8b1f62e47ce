// csrc/plant_boxqp.h and the BOX chain of csrc/plant_riccati.h on the host with a team of one: the statements plant_riccati_kernel<true, true>
// runs, on blocks, weights and limits read from stdin (tests/test_plant_boxqp.py).  Numbers travel as C hexadecimal floats.
//   plant_boxqp_check plan nq nu       prints the LDS bytes of a robot's limited chain and the box QP's share of it in doubles
//   plant_boxqp_check limit            in: count, then count triples u lo hi; out: plant_feedback_limit of each
//   plant_boxqp_check                  the limited chain:
//   in:  B T nq nu nr n_cols n_Q n_R n_keep n_rho n_lim (0: no limits)
//        status (T B), dz (T B nr n_cols, column-major blocks), Q (n_Q n n), Qf (n n), R (n_R m m), q ((T+1) B n), r (T B m), rho (n_rho),
//        and with limits u_lo (n_lim m), u_hi (n_lim m), u_nom (T B m)
//   out: one line each - K, k, P0, p0, dV, status, n_cut, clamped
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
        std::printf("%zu %zu\n", plant_riccati_box_lds(nq, nu), plant_boxqp_work_doubles(nu));
        return 0;
    }
    if (argc == 2 && std::strcmp(argv[1], "limit") == 0) {
        int count;
        if (std::scanf("%d", &count) != 1) return 2;
        const std::vector<double> v = read_doubles((size_t)3 * count);
        std::vector<double> out(count);
        for (int i = 0; i < count; ++i) out[i] = plant_feedback_limit(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
        print_doubles(out);
        return 0;
    }
    int B, T, nq, nu, nr, n_cols, n_Q, n_R, n_keep, n_rho, n_lim;
    if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d", &B, &T, &nq, &nu, &nr, &n_cols, &n_Q, &n_R, &n_keep, &n_rho, &n_lim) != 11) return 2;
    const size_t TB = (size_t)T * B, n = (size_t)2 * nq, m = (size_t)nu;
    std::vector<int> tape_status(TB);
    for (size_t i = 0; i < TB; ++i) if (std::scanf("%d", &tape_status[i]) != 1) return 2;
    const std::vector<double> dz = read_doubles(TB * nr * n_cols), Q = read_doubles(n_Q * n * n), Qf = read_doubles(n * n), R = read_doubles(n_R * m * m),
                              q = read_doubles((size_t)(T + 1) * B * n), r = read_doubles(TB * m), rho = read_doubles(n_rho),
                              u_lo = read_doubles(n_lim * m), u_hi = read_doubles(n_lim * m), u_nom = read_doubles(n_lim ? TB * m : 0);
    // every output starts from a value the chain never writes, so a hole shows
    std::vector<double> K((size_t)n_keep * B * m * n, -7.0), k((size_t)n_keep * B * m, -7.0), P0(B * n * n, -7.0), p0(B * n, -7.0), dV((size_t)B * 2, -7.0);
    std::vector<int> status(B, -1), n_cut(B, -1), clamped((size_t)n_keep * B, -1);
    PlantRiccati L{dz.data(), tape_status.data(), Q.data(), Qf.data(), R.data(), q.data(), r.data(), K.data(), k.data(), P0.data(), p0.data(), dV.data(),
                   status.data(), n_cut.data(), B, T, nq, nu, nr, n_cols, 1, n_Q, n_R, n_keep, rho[0]};
    L.rho_b = rho.data(); L.n_rho = n_rho; L.clamped = clamped.data();
    if (n_lim) { L.u_lo = u_lo.data(); L.u_hi = u_hi.data(); L.u_nom = u_nom.data(); L.n_lim = n_lim; }
    if (nu > PLANT_BOXQP_MAX_M || plant_riccati_box_lds(nq, nu) > PLANT_RIC_MAX_LDS) return 3;
    for (int rb = 0; rb < B; ++rb) {
        std::vector<double> work(plant_riccati_box_work_doubles(nq, nu));      // exactly what the kernel's LDS holds: ASan guards its ends
        PlantRiccatiSolo team;
        plant_riccati_chain_as<true, true>(L, rb, work.data(), team);
    }
    print_doubles(K); print_doubles(k); print_doubles(P0); print_doubles(p0); print_doubles(dV);
    print_ints(status); print_ints(n_cut); print_ints(clamped);
    return 0;
}
