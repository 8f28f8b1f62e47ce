// Host harness for hopper_3D of contactimplicitmpc/jl_amd/csrc/plant_model.h: reads "kappa kind p[4] z[19] th[22]" from stdin
// (kind: a CIMPC_TERRAIN_* of the flat or 3-D kinds) and prints, for plant_residual_terrain on that terrain and then for the flat
// plant_residual, the residual and the dual-number Jacobian dr/dz (row-major), one line each.  "invalid" if the model refuses
// the terrain.
#include <cstdio>
#include <type_traits>
#include <vector>
#include "../../contactimplicitmpc/jl_amd/csrc/plant_model.h"
using cimpc::Dual;
template <class F>
static void dump(int nz, const std::vector<double>& z, F eval) {
    std::vector<double> r(nz);
    eval(z.data(), r.data());
    for (double v : r) printf("%.17g ", v);
    printf("\n");
    std::vector<Dual> zd(nz), rd(nz);
    std::vector<double> J((size_t)nz * nz);
    for (int j = 0; j < nz; ++j) {
        for (int i = 0; i < nz; ++i) zd[i] = {z[i], i == j ? 1.0 : 0.0};
        eval(zd.data(), rd.data());
        for (int i = 0; i < nz; ++i) J[(size_t)i * nz + j] = rd[i].d;
    }
    for (double v : J) printf("%.17g ", v);
    printf("\n");
}
int main() {
    double kappa;
    cimpc_terrain E{};
    if (scanf("%lf %d", &kappa, &E.kind) != 2) return 1;
    for (double& v : E.p) if (scanf("%lf", &v) != 1) return 1;
    cimpc::PlantModel M{};
    if (!cimpc::plant_model_by_id(CIMPC_PLANT_HOPPER_3D, &M)) return 1;
    if (!cimpc::terrain_valid_for(M, E)) { printf("invalid\n"); return 0; }
    const int nz = M.nz(), nth = M.nth();
    if (nz != 19 || nth != 22) return 1;
    std::vector<double> z(nz), th(nth);
    for (auto& v : z) if (scanf("%lf", &v) != 1) return 1;
    for (auto& v : th) if (scanf("%lf", &v) != 1) return 1;
    dump(nz, z, [&](const auto* zz, auto* rr) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(zz)>>;
        cimpc::plant_residual_terrain<T>(M, E, zz, th.data(), kappa, rr);
    });
    dump(nz, z, [&](const auto* zz, auto* rr) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(zz)>>;
        cimpc::plant_residual<T>(M, zz, th.data(), kappa, rr);
    });
    return 0;
}
