// The models the library is compiled for, each stated ONCE (plain C++: tests/native/model_table_check.cpp builds it with g++), and the
// lookups the dispatchers share.  A further model is one row here + one instantiation file per kernel family it wants
// (ip_model_<name>.hip; async_model_<name>.hip if its last column is 1) + the file names in the Makefile's SRCS.
#pragma once
#include "../../../include/cimpc.h"

namespace cimpc {

// name, nq, nu, nw, nc, nb (src/dynamics/*/model.jl of the reference; point_foot_quadruped and centroidal_quadruped_box share the centroidal row), single-launch solve
#define CIMPC_MODEL_TABLE(X)                \
    X(pushbot, 2, 2, 2, 2, 4, 1)            \
    X(hopper, 4, 2, 2, 1, 2, 1)             \
    X(quadruped, 11, 8, 2, 4, 8, 1)         \
    X(flamingo, 9, 6, 2, 4, 8, 1)           \
    X(centroidal, 18, 12, 3, 4, 16, 1)      \
    X(hopper3d, 7, 3, 3, 1, 4, 0)           \
    X(walledcartpole, 4, 1, 4, 2, 4, 0)     \
    X(particle, 3, 3, 3, 1, 4, 0)           \
    X(particle2d, 2, 2, 2, 1, 2, 0)         \
    X(centroidal_wall, 18, 12, 3, 8, 32, 0)

struct ModelRow { const char* name; int nq, nu, nw, nc, nb; bool async; };
#define CIMPC_MODEL_ID(name, q, u, w, c, b, a) MODEL_##name,
#define CIMPC_MODEL_ROW(name, q, u, w, c, b, a) {#name, q, u, w, c, b, a != 0},
enum ModelId : int { CIMPC_MODEL_TABLE(CIMPC_MODEL_ID) MODEL_COUNT };
constexpr ModelRow MODEL_TABLE[MODEL_COUNT] = {CIMPC_MODEL_TABLE(CIMPC_MODEL_ROW)};

// lanes per interior-point problem: the smallest of 16, 32, 64 that holds the nx = nq and ny = 2 nc + nb rows (= Model<...>::G, asserted in
// ip_kernel_impl.h).  A 64-lane row (one problem per wavefront) is compiled for :configuration mode only and has no B2 callbacks.
constexpr int model_lanes(const ModelRow& r) {
    const int ny = 2 * r.nc + r.nb, n = r.nq > ny ? r.nq : ny;
    return n <= 16 ? 16 : n <= 32 ? 32 : 64;
}
// the row of dm's five dimensions, MODEL_COUNT = none
constexpr int model_find(const cimpc_dims* dm) {
    const auto is = [dm](const ModelRow& r) { return r.nq == dm->nq && r.nu == dm->nu && r.nw == dm->nw && r.nc == dm->nc && r.nb == dm->nb; };
    int id = 0;
    while (id < MODEL_COUNT && !is(MODEL_TABLE[id])) ++id;
    return id;
}
// ... if it has B2 callbacks / a compiled sweep kernel and kernel info / a single-launch solve (newton_async_impl.h: horizons of at most 96) for dm
constexpr int model_callback(const cimpc_dims* dm) { const int id = model_find(dm); return id < MODEL_COUNT && model_lanes(MODEL_TABLE[id]) <= 32 ? id : MODEL_COUNT; }
constexpr int model_sweep(const cimpc_dims* dm) { return dm->mode == CIMPC_MODE_CONFIGURATION ? model_find(dm) : model_callback(dm); }
constexpr int model_async(const cimpc_dims* dm) { const int id = model_find(dm); return id < MODEL_COUNT && MODEL_TABLE[id].async && dm->mode == CIMPC_MODE_CONFIGURATION && dm->H <= 96 ? id : MODEL_COUNT; }
// the horizon-level kernels (newton_kernels.hip) depend on (nq, nu) only: compiled for the projection of the rows
constexpr bool model_has_nqnu(int nq, int nu) {
    for (const ModelRow& r : MODEL_TABLE) if (r.nq == nq && r.nu == nu) return true;
    return false;
}

}  // namespace cimpc
