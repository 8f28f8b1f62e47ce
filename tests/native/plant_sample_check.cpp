// csrc/plant_sample.h on the host: the statements the kernels of plant_sample.hip and the cimpc_plant_sampler entries run, on numbers read
// from stdin (tests/test_plant_sample.py).  Doubles travel as C hexadecimal floats, so nothing is rounded on the way.
//   plant_sample_check philox   in:  n, then n x (c0 c1 c2 c3 k0 k1)        out: per counter one line: the four output words in hex
//   plant_sample_check eps      in:  n, then n x (seed draw b c e)          out: the n deviates on one line
//   plant_sample_check draw     in:  n, then n x (s n_iter it)              out: per triple plant_sample_draw
//   plant_sample_check rows     in:  n, then n x (H noise_hold)             out: per pair plant_sample_noise_rows
//   plant_sample_check cand     in:  H B N nu noise_hold n_lim (0: no limits) seed draw, u_nom (H B nu), sigma (nu), u_lo, u_hi (n_lim nu each)
//                               out: the candidates' controls (H, N B, nu) on one line, as the expansion kernel writes them
//   plant_sample_check update   in:  H B N nu n_lim (0: none) lam, u_nom (H B nu), cand (H, N B, nu), J (N B), conv (N B ints), u_lo, u_hi
//                               out: choice (B) | n_eligible (B) | J_nom (B) | J_best (B) | weights (N B) | the unnormalised weights (N B) |
//                                    the new plan (H B nu), a line each
//   plant_sample_check refusal  in:  N B H nu has_sigma, sigma (nu), noise_hold lam n_iter    out: plant_sample_refusal's reason, or ok
// Every array has its exact size, so AddressSanitizer guards both ends.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_sample.h"

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

static uint64_t read_u64() {
    unsigned long long v;
    if (std::scanf("%llu", &v) != 1) std::exit(2);
    return (uint64_t)v;
}

static void print_doubles(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%a", i ? " " : "", v[i]);
    std::printf("\n");
}

static void print_ints(const std::vector<int>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? " " : "", v[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    using namespace cimpc;
    if (argc != 2) return 2;
    const char* mode = argv[1];
    if (std::strcmp(mode, "philox") == 0) {
        const int n = read_int();
        for (int k = 0; k < n; ++k) {
            uint32_t ctr[4], key[2], out[4];
            for (auto& c : ctr) c = (uint32_t)read_u64();
            for (auto& c : key) c = (uint32_t)read_u64();
            plant_sample_philox(ctr, key, out);
            std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", out[0], out[1], out[2], out[3]);
        }
        return 0;
    }
    if (std::strcmp(mode, "eps") == 0) {
        const int n = read_int();
        std::vector<double> out((size_t)n);
        for (int k = 0; k < n; ++k) {
            const uint64_t seed = read_u64();
            const uint32_t draw = (uint32_t)read_u64(), b = (uint32_t)read_u64(), c = (uint32_t)read_u64(), e = (uint32_t)read_u64();
            out[k] = plant_sample_eps(seed, draw, b, c, e);
        }
        print_doubles(out);
        return 0;
    }
    if (std::strcmp(mode, "draw") == 0) {
        const int n = read_int();
        for (int k = 0; k < n; ++k) {
            const int s = read_int(), n_iter = read_int(), it = read_int();
            std::printf("%" PRIu32 "\n", plant_sample_draw(s, n_iter, it));
        }
        return 0;
    }
    if (std::strcmp(mode, "rows") == 0) {
        const int n = read_int();
        for (int k = 0; k < n; ++k) {
            const int H = read_int(), hold = read_int();
            std::printf("%d\n", plant_sample_noise_rows(H, hold));
        }
        return 0;
    }
    if (std::strcmp(mode, "cand") == 0) {
        const int H = read_int(), B = read_int(), N = read_int(), nu = read_int(), hold = read_int(), n_lim = read_int();
        const uint64_t seed = read_u64();
        const uint32_t draw = (uint32_t)read_u64();
        const std::vector<double> u_nom = read_doubles((size_t)H * B * nu), sigma = read_doubles((size_t)nu), lo = read_doubles((size_t)n_lim * nu),
                                  hi = read_doubles((size_t)n_lim * nu);
        const size_t NB = (size_t)N * B;
        std::vector<double> u((size_t)H * NB * nu, -1.0);
        for (int j = 0; j < plant_sample_noise_rows(H, hold); ++j)
            for (size_t r = 0; r < NB; ++r)
                for (int i = 0; i < nu; ++i) {
                    const int c = (int)(r / B), b = (int)(r % B);
                    const double eps = c == 0 ? 0.0 : plant_sample_eps(seed, draw, (uint32_t)b, (uint32_t)c, (uint32_t)j * (uint32_t)nu + (uint32_t)i);
                    const double *l = n_lim ? plant_feedback_limits(lo.data(), n_lim, b, nu) : nullptr, *h = n_lim ? plant_feedback_limits(hi.data(), n_lim, b, nu) : nullptr;
                    for (long long t = (long long)j * hold; t < (long long)(j + 1) * hold && t < H; ++t)
                        u[((size_t)t * NB + r) * nu + i] = plant_sample_candidate(u_nom[((size_t)t * B + b) * nu + i], sigma[i], eps, c, l, h, i);
                }
        print_doubles(u);
        return 0;
    }
    if (std::strcmp(mode, "update") == 0) {
        const int H = read_int(), B = read_int(), N = read_int(), nu = read_int(), n_lim = read_int();
        const double lam = read_double();
        const size_t NB = (size_t)N * B;
        std::vector<double> plan = read_doubles((size_t)H * B * nu);
        const std::vector<double> cand = read_doubles((size_t)H * NB * nu), J = read_doubles(NB);
        std::vector<int> conv(NB);
        for (auto& v : conv) v = read_int();
        const std::vector<double> lo = read_doubles((size_t)n_lim * nu), hi = read_doubles((size_t)n_lim * nu);
        std::vector<int> ok(NB, -1), choice((size_t)B, -7), n_eligible((size_t)B, -7);
        std::vector<double> raw(NB, -1.0), weights(NB, -1.0), J_nom((size_t)B, -1.0), J_best((size_t)B, -1.0);
        const PlantSampleUpdate P{J.data(), conv.data(), cand.data(), plan.data(), n_lim ? lo.data() : nullptr, n_lim ? hi.data() : nullptr, n_lim ? n_lim : 1,
                                  ok.data(), raw.data(), weights.data(), J_nom.data(), J_best.data(), choice.data(), n_eligible.data(), B, N, H, nu, lam};
        PlantCostSolo team;
        for (int b = 0; b < B; ++b)
            if (plant_sample_update(P, b, team) != choice[b]) return 3;
        print_ints(choice); print_ints(n_eligible); print_doubles(J_nom); print_doubles(J_best); print_doubles(weights); print_doubles(raw);
        print_doubles(plan);
        return 0;
    }
    if (std::strcmp(mode, "refusal") == 0) {
        const int N = read_int(), B = read_int(), H = read_int(), nu = read_int(), has_sigma = read_int();
        const std::vector<double> sigma = read_doubles((size_t)nu);
        const int hold = read_int();
        const double lam = read_double();
        const int n_iter = read_int();
        const char* why = plant_sample_refusal(N, B, H, nu, has_sigma ? sigma.data() : nullptr, hold, lam, n_iter);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    return 2;
}
