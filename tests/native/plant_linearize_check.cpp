// Host harness for the θ-generic residuals of contactimplicitmpc/jl_amd/csrc/plant_model.h, evaluated as plant_linearize_kernel
// evaluates them: reads "model kappa has_terrain [kind n_pieces p[4] brk[8] off[8] coef[8][4]] z... th..." from stdin and prints
//   nz nth | r (double, double) at kappa | dr/dz (row-major) and dr/dθ (row-major) from (Dual, DualTh), one seeded tangent per
//   column | dr/dz from (Dual, double), the Jacobian of the step kernel.
// has_terrain = 0 is plant_residual (or the box / wall / walls residual of the model), 1 is plant_residual_terrain.
#include <cstdio>
#include <type_traits>
#include <vector>
#include "../../contactimplicitmpc/jl_amd/csrc/plant_model.h"
using cimpc::Dual;
using cimpc::DualTh;
int main() {
    int model, has_terrain; double kappa;
    if (scanf("%d %lf %d", &model, &kappa, &has_terrain) != 3) return 1;
    cimpc_terrain E{};
    if (has_terrain) {
        if (scanf("%d %d", &E.kind, &E.n_pieces) != 2) return 1;
        for (double& v : E.p) if (scanf("%lf", &v) != 1) return 1;
        for (double& v : E.brk) if (scanf("%lf", &v) != 1) return 1;
        for (double& v : E.off) if (scanf("%lf", &v) != 1) return 1;
        for (auto& row : E.coef) for (double& v : row) if (scanf("%lf", &v) != 1) return 1;
    }
    cimpc::PlantModel M{};
    if (!cimpc::plant_model_by_id(model, &M)) return 1;
    if (has_terrain ? !cimpc::terrain_valid_for(M, E) : model == CIMPC_PLANT_PARTICLE_2D) { printf("invalid\n"); return 0; }
    const int nz = M.nz(), nth = M.nth();
    std::vector<double> z(nz), th(nth), r(nz);
    for (auto& v : z) if (scanf("%lf", &v) != 1) return 1;
    for (auto& v : th) if (scanf("%lf", &v) != 1) return 1;
    auto residual = [&](const auto* zz, const auto* tt, double kap, auto* rr) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(zz)>>;
        if (has_terrain) cimpc::plant_residual_terrain<T>(M, E, zz, tt, kap, rr);
        else if (M.kind == cimpc::PLANT_KIND_CENTROIDAL_BOX || M.kind == cimpc::PLANT_KIND_CENTROIDAL_WALL) cimpc::plant_residual_centroidal_env<T>(M, zz, tt, kap, rr);
        else if (M.kind == cimpc::PLANT_KIND_PUSHBOT || M.kind == cimpc::PLANT_KIND_WALLEDCARTPOLE) cimpc::plant_residual_walls<T>(M, zz, tt, kap, rr);
        else cimpc::plant_residual<T>(M, zz, tt, kap, rr);
    };
    auto print = [](const std::vector<double>& a) { for (double v : a) printf("%.17g ", v); printf("\n"); };
    printf("%d %d\n", nz, nth);
    residual(z.data(), th.data(), kappa, r.data());
    print(r);
    std::vector<Dual> zd(nz), rd(nz);
    std::vector<DualTh> td(nth);
    std::vector<double> Jz((size_t)nz * nz), Jth((size_t)nz * nth), Jold((size_t)nz * nz);
    for (int c = 0; c < nz + nth; ++c) {
        for (int i = 0; i < nz; ++i) zd[i] = {z[i], i == c ? 1.0 : 0.0};
        for (int i = 0; i < nth; ++i) td[i] = {{th[i], nz + i == c ? 1.0 : 0.0}};
        residual(zd.data(), td.data(), 0.0, rd.data());
        for (int i = 0; i < nz; ++i) (c < nz ? Jz[(size_t)i * nz + c] : Jth[(size_t)i * nth + (c - nz)]) = rd[i].d;
    }
    print(Jz);
    print(Jth);
    for (int c = 0; c < nz; ++c) {
        for (int i = 0; i < nz; ++i) zd[i] = {z[i], i == c ? 1.0 : 0.0};
        residual(zd.data(), th.data(), 0.0, rd.data());
        for (int i = 0; i < nz; ++i) Jold[(size_t)i * nz + c] = rd[i].d;
    }
    print(Jold);
    return 0;
}
