// Host harness for pushbot and walledcartpole of contactimplicitmpc/jl_amd/csrc/plant_model.h: reads "id kappa z[nz] th[nth]" from
// stdin (id: CIMPC_PLANT_PUSHBOT or CIMPC_PLANT_WALLEDCARTPOLE) and prints "nz nth", the residual of plant_residual_walls and its
// dual-number Jacobian dr/dz (row-major), one line each; then one line per CIMPC_TERRAIN_* kind 0..6: whether the model takes it.
#include <cstdio>
#include <vector>
#include "../../contactimplicitmpc/jl_amd/csrc/plant_model.h"
using cimpc::Dual;
int main() {
    int id;
    double kappa;
    if (scanf("%d %lf", &id, &kappa) != 2) return 1;
    cimpc::PlantModel M{};
    if (!cimpc::plant_model_by_id(id, &M)) return 1;
    if (M.kind != cimpc::PLANT_KIND_PUSHBOT && M.kind != cimpc::PLANT_KIND_WALLEDCARTPOLE) return 1;
    const int nz = M.nz(), nth = M.nth();
    std::vector<double> z(nz), th(nth), r(nz);
    for (auto& v : z) if (scanf("%lf", &v) != 1) return 1;
    for (auto& v : th) if (scanf("%lf", &v) != 1) return 1;
    printf("%d %d\n", nz, nth);
    cimpc::plant_residual_walls<double>(M, z.data(), th.data(), kappa, r.data());
    for (double v : r) printf("%.17g ", v);
    printf("\n");
    std::vector<Dual> zd(nz), rd(nz);
    std::vector<double> J((size_t)nz * nz);
    for (int j = 0; j < nz; ++j) {
        for (int i = 0; i < nz; ++i) zd[i] = {z[i], i == j ? 1.0 : 0.0};
        cimpc::plant_residual_walls<Dual>(M, zd.data(), th.data(), kappa, rd.data());
        for (int i = 0; i < nz; ++i) J[(size_t)i * nz + j] = rd[i].d;
    }
    for (double v : J) printf("%.17g ", v);
    printf("\n");
    for (int kind = CIMPC_TERRAIN_FLAT; kind <= CIMPC_TERRAIN_BOWL_3D; ++kind) {
        cimpc_terrain E{};
        E.kind = kind; E.n_pieces = 1; E.p[1] = 1.0;
        printf("%d\n", cimpc::terrain_valid_for(M, E) ? 1 : 0);
    }
    return 0;
}
