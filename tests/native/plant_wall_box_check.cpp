// Host harness for the box and wall residual of contactimplicitmpc/jl_amd/csrc/plant_model.h: reads "model kappa z... th..."
// (model 7 = centroidal_quadruped_box, 8 = centroidal_quadruped_wall) from stdin and prints nz nth, then the residual and the
// dual-number Jacobian dr/dz (row-major) of plant_residual_centroidal_env; for the box also the two of plant_residual on the
// centroidal model with the box's 0.5 kg feet (equal where e(x) = 0).
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
    int model; double kappa;
    if (scanf("%d %lf", &model, &kappa) != 2) return 1;
    cimpc::PlantModel M{};
    if (!cimpc::plant_model_by_id(model, &M)) return 1;
    const int nz = M.nz(), nth = M.nth();
    std::vector<double> z(nz), th(nth);
    for (auto& v : z) if (scanf("%lf", &v) != 1) return 1;
    for (auto& v : th) if (scanf("%lf", &v) != 1) return 1;
    printf("%d %d\n", nz, nth);
    dump(nz, z, [&](const auto* zz, auto* rr) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(zz)>>;
        cimpc::plant_residual_centroidal_env<T>(M, zz, th.data(), kappa, rr);
    });
    if (model == CIMPC_PLANT_CENTROIDAL_BOX) {
        cimpc::PlantModel C = cimpc::plant_centroidal(true);
        C.mass[1] = M.mass[1];
        dump(nz, z, [&](const auto* zz, auto* rr) {
            using T = std::remove_const_t<std::remove_pointer_t<decltype(zz)>>;
            cimpc::plant_residual<T>(C, zz, th.data(), kappa, rr);
        });
    }
    return 0;
}
