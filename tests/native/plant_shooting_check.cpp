// csrc/plant_shooting.h on the host with a team of one: the statements the kernels of plant_shooting.hip run, on numbers read from stdin
// (tests/test_plant_shooting.py).  Numbers travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_shooting_check cost     in:  B T M nq nu n_Q n_R n_x weight, qs ((L+2) (M B) nq), u (T B nu), Q (n_Q n n), Qf (n n), R (n_R m m),
//                                      x_goal ((T+1) n_x n), u_goal (T n_x m)      out: one line each - J, D, defects, lin_q, lin_r, phi
//   plant_shooting_check layout   in:  B T M      out: per (l, j, b) in that order the pair entry, stitched; then per t = 0 .. T the pair j, l
//   plant_shooting_check valid    in:  T M B      out: plant_shooting_refusal's reason or ok
//   plant_shooting_check nodes    in:  M B nq, nodes (M B 2nq)      out: plant_shooting_nodes_refusal's reason or ok
//   plant_shooting_check lqr      csrc/plant_riccati.h's limited chain with the defect hook (shoot 1) or without it (shoot 0):
//                                 in:  B T nq nu nr n_cols n_Q n_R n_keep n_rho n_lim (0: no limits) seg_len shoot, status (T B), dz (T B nr
//                                      n_cols, column-major blocks), Q, Qf, R, q ((T+1) B n), r (T B m), rho (n_rho), u_lo, u_hi (n_lim m each),
//                                      u_nom (T B m, with limits), defects ((T / seg_len - 1) B n, with shoot)
//                                 out: one line each - K, k, P0, p0, dV, status, n_cut, clamped
//   plant_shooting_check forward  plant_shoot_forward_chain:
//                                 in:  B T nq nu nr n_cols n_Q n_R seg_len, dz, Q, Qf, R, lin_q ((T+1) B n), lin_r (T B m), K (T B (m x n) column-major),
//                                      k (T B m), defects ((T / seg_len - 1) B n)      out: one line each - dx_nodes, du, dJ
//   plant_shooting_check accept   in:  n_alpha B armijo, alpha (n_alpha), weight (B), converged (n_alpha B), J (n_alpha B), D (n_alpha B), phi_nom (B),
//                                      D_nom (B), dJ (B 2)      out: phi (n_alpha B), ok (n_alpha B), choice (B)
//   plant_shooting_check node     in:  n, then n triples x alpha dx      out: n shifted node entries
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_riccati.h"
#include "../../contactimplicitmpc/jl_amd/csrc/plant_shooting.h"

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

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc != 2) return 2;
    if (std::strcmp(argv[1], "cost") == 0) {
        const int B = read_int(), T = read_int(), M = read_int(), nq = read_int(), nu = read_int(), n_Q = read_int(), n_R = read_int(), n_x = read_int();
        const double weight = read_double();
        if (plant_shooting_refusal(T, M, B)) return 3;
        const int L = T / M;
        const size_t n = (size_t)2 * nq, m = (size_t)nu;
        const std::vector<double> qs = read_doubles((size_t)(L + 2) * M * B * nq), u = read_doubles((size_t)T * B * m), Q = read_doubles(n_Q * n * n),
                                  Qf = read_doubles(n * n), R = read_doubles(n_R * m * m), xg = read_doubles((size_t)(T + 1) * n_x * n),
                                  ug = read_doubles((size_t)T * n_x * m);
        const PlantCost C{Q.data(), Qf.data(), R.data(), xg.data(), ug.data(), n_Q, n_R, n_x, T, nq, nu};
        if (!plant_cost_valid(C, B)) return 3;
        // every output starts from a value the chains never write, so a hole shows
        std::vector<double> J(B, -7.0), D(B, -7.0), phi(B, -7.0), d((size_t)(M - 1) * B * n, -7.0), lin_q((size_t)(T + 1) * B * n, -7.0), lin_r((size_t)T * B * m, -7.0),
            lt((size_t)(T + 1) * B, -7.0);
        for (int j = 1; j < M; ++j)
            for (int b = 0; b < B; ++b)
                for (int i = 0; i < 2 * nq; ++i) d[((size_t)(j - 1) * B + b) * n + i] = plant_shoot_defect(qs.data(), M, B, L, nq, j, b, i);
        for (int b = 0; b < B; ++b) {
            std::vector<double> work(plant_cost_work_doubles(nq, nu));      // exactly what a workgroup's LDS is given: ASan guards its ends
            PlantCostSolo team;
            J[b] = plant_shoot_cost(C, M, B, b, qs.data(), u.data(), work.data(), lin_q.data(), lin_r.data(), team);
            // the kernels' route to J: a stage per workgroup, then the running sum
            for (int t = 0; t <= T; ++t) lt[(size_t)t * B + b] = plant_shoot_stage(C, M, B, t, b, qs.data(), u.data(), work.data(), nullptr, nullptr, team);
            if (plant_shoot_total(lt.data(), T, B, b) != J[b]) return 4;
            D[b] = plant_shoot_defect_sum(d.data(), M, B, nq, b);
            phi[b] = plant_shoot_merit(J[b], weight, D[b]);
        }
        print_doubles(J); print_doubles(D); print_doubles(d); print_doubles(lin_q); print_doubles(lin_r); print_doubles(phi);
        return 0;
    }
    if (std::strcmp(argv[1], "layout") == 0) {
        const int B = read_int(), T = read_int(), M = read_int();
        if (plant_shooting_refusal(T, M, B)) return 3;
        const int L = T / M;
        for (int l = 0; l < L; ++l)
            for (int j = 0; j < M; ++j)
                for (int b = 0; b < B; ++b) std::printf("%zu %zu ", plant_shoot_entry(l, j, b, M, B), plant_shoot_stitched(l, j, b, L, B));
        std::printf("\n");
        for (int t = 0; t <= T; ++t) std::printf("%d %d ", plant_shoot_stage_rows(t, T, L).j, plant_shoot_stage_rows(t, T, L).l);
        std::printf("\n");
        return 0;
    }
    if (std::strcmp(argv[1], "valid") == 0) {
        const int T = read_int(), M = read_int(), B = read_int();
        const char* why = plant_shooting_refusal(T, M, B);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (std::strcmp(argv[1], "nodes") == 0) {
        const int M = read_int(), B = read_int(), nq = read_int();
        const std::vector<double> nodes = read_doubles((size_t)M * B * 2 * nq);
        const char* why = plant_shooting_nodes_refusal(nodes.data(), M, B, nq);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (std::strcmp(argv[1], "accept") == 0) {
        const int n_alpha = read_int(), B = read_int();
        const double armijo = read_double();
        const std::vector<double> alpha = read_doubles(n_alpha), weight = read_doubles(B);
        std::vector<int> conv((size_t)n_alpha * B), ok((size_t)n_alpha * B), choice(B);
        for (auto& c : conv) c = read_int();
        const std::vector<double> J = read_doubles((size_t)n_alpha * B), D = read_doubles((size_t)n_alpha * B), phi_nom = read_doubles(B), D_nom = read_doubles(B),
                                  dJ = read_doubles((size_t)2 * B);
        std::vector<double> phi((size_t)n_alpha * B);
        for (int b = 0; b < B; ++b) {
            for (int c = 0; c < n_alpha; ++c) {
                const size_t e = (size_t)c * B + b;
                phi[e] = plant_shoot_merit(J[e], weight[b], D[e]);
                ok[e] = plant_shoot_acceptable(conv[e] != 0, phi[e], phi_nom[b], armijo, alpha[c], dJ[2 * b], dJ[2 * b + 1], weight[b], D_nom[b]);
            }
            choice[b] = plant_linesearch_choice(phi.data() + b, (size_t)B, ok.data() + b, (size_t)B, n_alpha);
        }
        print_doubles(phi);
        for (int v : ok) std::printf("%d ", v);
        std::printf("\n");
        for (int v : choice) std::printf("%d ", v);
        std::printf("\n");
        return 0;
    }
    if (std::strcmp(argv[1], "node") == 0) {
        const int n = read_int();
        std::vector<double> out(n);
        for (int i = 0; i < n; ++i) {
            const double x = read_double(), a = read_double(), dx = read_double();
            out[i] = plant_shoot_candidate_node(x, a, dx);
        }
        print_doubles(out);
        return 0;
    }
    if (std::strcmp(argv[1], "forward") == 0) {
        const int B = read_int(), T = read_int(), nq = read_int(), nu = read_int(), nr = read_int(), n_cols = read_int(), n_Q = read_int(), n_R = read_int(),
                  seg_len = read_int();
        if (plant_shoot_forward_refusal(T, seg_len, n_Q, n_R)) return 3;
        const size_t TB = (size_t)T * B, n = (size_t)2 * nq, m = (size_t)nu, n_def = (size_t)(T / seg_len - 1) * B * n;
        const std::vector<double> dz = read_doubles(TB * nr * n_cols), Q = read_doubles(n_Q * n * n), Qf = read_doubles(n * n), R = read_doubles(n_R * m * m),
                                  lq = read_doubles((size_t)(T + 1) * B * n), lr = read_doubles(TB * m), K = read_doubles(TB * m * n), k = read_doubles(TB * m),
                                  defects = read_doubles(n_def);
        std::vector<double> dxn(n_def, -7.0), du(TB * m, -7.0), dJ((size_t)2 * B, -7.0);
        const PlantShootForward F{dz.data(), K.data(), k.data(), Q.data(), Qf.data(), R.data(), lq.data(), lr.data(), defects.data(), dxn.data(), du.data(), dJ.data(),
                                  B, T, nq, nu, nr, n_cols, n_Q, n_R, seg_len};
        for (int rb = 0; rb < B; ++rb) {
            std::vector<double> work(plant_shoot_forward_work_doubles(nq, nu));      // exactly what the kernel's LDS holds: ASan guards its ends
            PlantRiccatiSolo team;
            plant_shoot_forward_chain(F, rb, work.data(), team);
        }
        print_doubles(dxn); print_doubles(du); print_doubles(dJ);
        return 0;
    }
    if (std::strcmp(argv[1], "lqr") == 0) {
        const int B = read_int(), T = read_int(), nq = read_int(), nu = read_int(), nr = read_int(), n_cols = read_int(), n_Q = read_int(), n_R = read_int(),
                  n_keep = read_int(), n_rho = read_int(), n_lim = read_int(), seg_len = read_int(), shoot = read_int();
        const size_t TB = (size_t)T * B, n = (size_t)2 * nq, m = (size_t)nu;
        std::vector<int> tape_status(TB);
        for (auto& v : tape_status) v = read_int();
        const std::vector<double> dz = read_doubles(TB * nr * n_cols), Q = read_doubles(n_Q * n * n), Qf = read_doubles(n * n), R = read_doubles(n_R * m * m),
                                  q = read_doubles((size_t)(T + 1) * B * n), r = read_doubles(TB * m), rho = read_doubles(n_rho),
                                  u_lo = read_doubles(n_lim * m), u_hi = read_doubles(n_lim * m), u_nom = read_doubles(n_lim ? TB * m : 0),
                                  defects = read_doubles(shoot ? (size_t)(T / seg_len - 1) * B * n : 0);
        std::vector<double> K((size_t)n_keep * B * m * n, -7.0), k((size_t)n_keep * B * m, -7.0), P0(B * n * n, -7.0), p0(B * n, -7.0), dV((size_t)B * 2, -7.0);
        std::vector<int> status(B, -1), n_cut(B, -1), clamped((size_t)n_keep * B, -1);
        PlantRiccati L{dz.data(), tape_status.data(), Q.data(), Qf.data(), R.data(), q.data(), r.data(), K.data(), k.data(), P0.data(), p0.data(), dV.data(),
                       status.data(), n_cut.data(), B, T, nq, nu, nr, n_cols, 1, n_Q, n_R, n_keep, rho[0]};
        L.rho_b = rho.data(); L.n_rho = n_rho; L.clamped = clamped.data();
        if (n_lim) { L.u_lo = u_lo.data(); L.u_hi = u_hi.data(); L.u_nom = u_nom.data(); L.n_lim = n_lim; }
        if (shoot) { L.defects = defects.data(); L.seg_len = seg_len; }
        if (!plant_riccati_fits(nq, nu) || (shoot && (seg_len < 1 || T % seg_len != 0))) return 3;
        for (int rb = 0; rb < B; ++rb) {
            PlantRiccatiSolo team;
            if (shoot) {
                std::vector<double> work(plant_riccati_shoot_work_doubles(nq, nu));      // exactly what the kernel's LDS holds: ASan guards its ends
                plant_riccati_chain_as<true, true, true>(L, rb, work.data(), team);
            } else {
                std::vector<double> work(plant_riccati_box_work_doubles(nq, nu));
                plant_riccati_chain_as<true, true>(L, rb, work.data(), team);
            }
        }
        print_doubles(K); print_doubles(k); print_doubles(P0); print_doubles(p0); print_doubles(dV);
        for (int v : status) std::printf("%d ", v);
        std::printf("\n");
        for (int v : n_cut) std::printf("%d ", v);
        std::printf("\n");
        for (int v : clamped) std::printf("%d ", v);
        std::printf("\n");
        return 0;
    }
    return 2;
}
