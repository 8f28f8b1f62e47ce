// What a launch of plant_sensitivity_kernel (plant_sensitivity.hip) needs of a CU's LDS, in one place (plain C++, host only:
// tests/native/plant_sensitivity_plan_check.cpp builds it with g++).  The kernel holds the augmented matrix [R | -dr/dtheta[:, :n_cols]]
// of one knot row-major in dynamic LDS - nz rows of nz + n_cols doubles -, one multiplier column (nz doubles) and two words (the
// pivot row and the verdict), next to its static arrays: the knot's z and theta and its terrain.  Whatever does not fit is refused
// by the entry points before any device work.
#pragma once
#include <cstddef>

namespace cimpc {

constexpr size_t PLANT_SENS_MAX_LDS = 160 * 1024;      // of a gfx950 CU
// the static LDS of the largest instantiation (z[114], theta[53], a cimpc_terrain of 424 bytes), rounded up
constexpr size_t PLANT_SENS_STATIC_LDS = 2048;

constexpr size_t plant_sensitivity_lds(int nz, int n_cols) {
    return ((size_t)nz * ((size_t)nz + (size_t)n_cols) + (size_t)nz + 2) * sizeof(double);
}
constexpr bool plant_sensitivity_fits(int nz, int n_cols) {
    return nz >= 1 && n_cols >= 1 && plant_sensitivity_lds(nz, n_cols) + PLANT_SENS_STATIC_LDS <= PLANT_SENS_MAX_LDS;
}

static_assert(plant_sensitivity_lds(66, 53) == 63376 && plant_sensitivity_fits(66, 53), "centroidal_quadruped, every column of theta: 62 KB");
static_assert(plant_sensitivity_lds(114, 53) == 153232 && plant_sensitivity_fits(114, 53), "centroidal_quadruped_wall, every column: 150 KB, the largest model");
static_assert(!plant_sensitivity_fits(118, 53), "four more rows would not fit");

}  // namespace cimpc
