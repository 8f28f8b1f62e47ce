// Host build of contactimplicitmpc/jl_amd/csrc/plant_sensitivity_plan.h for tests/test_plant_gradients.py: one query per input line,
// "nz n_cols", answered by "<dynamic LDS bytes> <static LDS bytes set aside> <LDS of a CU> <1 if the launch fits, else 0>".
#include <cstdio>

#include "../../contactimplicitmpc/jl_amd/csrc/plant_sensitivity_plan.h"

int main() {
    int nz, n_cols;
    while (std::scanf("%d %d", &nz, &n_cols) == 2)
        std::printf("%zu %zu %zu %d\n", cimpc::plant_sensitivity_lds(nz, n_cols), cimpc::PLANT_SENS_STATIC_LDS, cimpc::PLANT_SENS_MAX_LDS,
                    cimpc::plant_sensitivity_fits(nz, n_cols) ? 1 : 0);
    return 0;
}
