// csrc/plant_mpc.h on the host: the statements the kernels of plant_mpc.hip and the cimpc_plant_mpc entries run, on numbers read from
// stdin (tests/test_plant_mpc.py).  Doubles travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_mpc_check rows      in:  H L n, then n values of s            out: per s one line: the H + 1 x rows, then the H u rows
//   plant_mpc_check warm      in:  H n, then n values of shift          out: per shift one line: the H warm-start rows
//   plant_mpc_check window    in:  s H L n_x n m, x_ref ((L + 1) n_x n), u_ref (L n_x m)
//                             out: x_goal ((H + 1) n_x n) on one line, u_goal (H n_x m) on the next
//   plant_mpc_check shift     in:  shift H B nu, u_plan (H B nu)        out: u_warm (H B nu) on one line
//   plant_mpc_check reset     in:  level active                        out: level active after plant_mpc_reset_robot
//   plant_mpc_check problem   in:  H L n_iter                           out: plant_mpc_problem_refusal's reason, or ok
//   plant_mpc_check step      in:  s shift has_plan                     out: plant_mpc_step_refusal's reason, or ok
//   plant_mpc_check state     in:  n, q0 (n), q1 (n)                    out: plant_mpc_state_refusal's reason, or ok
//   plant_mpc_check plan      in:  H B nu n_lim (0: no limits), u0 (H B nu), u_lo, u_hi (n_lim nu each)
//                             out: plant_mpc_plan_refusal's reason, or ok
// Every array has its exact size, so AddressSanitizer guards both ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_mpc.h"

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
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%a", i ? " " : "", v[i]);
    std::printf("\n");
}

static int say(const char* why) {
    std::printf("%s\n", why ? why : "ok");
    return 0;
}

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc != 2) return 2;
    const char* mode = argv[1];
    if (std::strcmp(mode, "rows") == 0) {
        const int H = read_int(), L = read_int(), n = read_int();
        for (int k = 0; k < n; ++k) {
            const int s = read_int();
            for (int t = 0; t <= H; ++t) std::printf("%d ", plant_mpc_x_row(s, t, L));
            for (int t = 0; t < H; ++t) std::printf("%d%s", plant_mpc_u_row(s, t, L), t + 1 < H ? " " : "");
            std::printf("\n");
        }
        return 0;
    }
    if (std::strcmp(mode, "warm") == 0) {
        const int H = read_int(), n = read_int();
        for (int k = 0; k < n; ++k) {
            const int shift = read_int();
            for (int t = 0; t < H; ++t) std::printf("%d%s", plant_mpc_warm_row(t, shift, H), t + 1 < H ? " " : "");
            std::printf("\n");
        }
        return 0;
    }
    if (std::strcmp(mode, "window") == 0) {
        const int s = read_int(), H = read_int(), L = read_int(), n_x = read_int(), n = read_int(), m = read_int();
        const std::vector<double> x_ref = read_doubles((size_t)(L + 1) * n_x * n), u_ref = read_doubles((size_t)L * n_x * m);
        std::vector<double> x_goal((size_t)(H + 1) * n_x * n, -1.0), u_goal((size_t)H * n_x * m, -1.0);
        for (int t = 0; t <= H; ++t)
            for (int g = 0; g < n_x; ++g)
                for (int rank = 0; rank < 3; ++rank)      // a team of three, one member after the other
                    plant_mpc_window(x_goal.data(), u_goal.data(), x_ref.data(), u_ref.data(), s, t, g, H, L, n_x, n, m, rank, 3);
        print_doubles(x_goal);
        print_doubles(u_goal);
        return 0;
    }
    if (std::strcmp(mode, "shift") == 0) {
        const int shift = read_int(), H = read_int(), B = read_int(), nu = read_int();
        const std::vector<double> u_plan = read_doubles((size_t)H * B * nu);
        std::vector<double> u_warm(u_plan.size(), -1.0);
        for (int t = 0; t < H; ++t)
            for (int b = 0; b < B; ++b)
                for (int rank = 0; rank < 2; ++rank) plant_mpc_warm_start(u_warm.data(), u_plan.data(), t, b, shift, H, B, nu, rank, 2);
        print_doubles(u_warm);
        return 0;
    }
    if (std::strcmp(mode, "reset") == 0) {
        int level = read_int(), active = read_int();
        plant_mpc_reset_robot(&level, &active);
        std::printf("%d %d\n", level, active);
        return 0;
    }
    if (std::strcmp(mode, "problem") == 0) {
        const int H = read_int(), L = read_int(), n_iter = read_int();
        return say(plant_mpc_problem_refusal(H, L, n_iter));
    }
    if (std::strcmp(mode, "step") == 0) {
        const int s = read_int(), shift = read_int(), has_plan = read_int();
        return say(plant_mpc_step_refusal(s, shift, has_plan != 0));
    }
    if (std::strcmp(mode, "state") == 0) {
        const int n = read_int();
        const std::vector<double> q0 = read_doubles(n), q1 = read_doubles(n);
        return say(plant_mpc_state_refusal(q0.data(), q1.data(), (size_t)n));
    }
    if (std::strcmp(mode, "plan") == 0) {
        const int H = read_int(), B = read_int(), nu = read_int(), n_lim = read_int();
        const std::vector<double> u0 = read_doubles((size_t)H * B * nu), lo = read_doubles((size_t)n_lim * nu), hi = read_doubles((size_t)n_lim * nu);
        return say(plant_mpc_plan_refusal(u0.data(), H, B, nu, n_lim ? lo.data() : nullptr, n_lim ? hi.data() : nullptr, n_lim ? n_lim : 1));
    }
    return 2;
}
