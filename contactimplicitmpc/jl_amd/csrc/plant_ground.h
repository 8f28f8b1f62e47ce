// The ground a plant kernel stands on, the sizes its instantiations are built at and which of them a model runs on, in one place for
// plant_kernel.hip (step, rollout), plant_linearize.hip and plant_sensitivity.hip.  Plain C++ like plant_model.h
// (tests/native/plant_ground_check.cpp builds it with g++); the device helpers at the end are for hipcc alone.  A new model or a new
// ground is added HERE: its size, its line in plant_instance, its tag in plant_visit_instance, its branch in plant_ground_residual
// (and in the copy of that dispatch plant_step_kernel keeps).
#pragma once
#include "../../../include/cimpc.h"
#include "plant_model.h"

namespace cimpc {

// The ground of a kernel instantiation.  FLAT: plant_residual.  TERRAIN: robot or knot i stands on terrain[n_terrain == 1 ? 0 : i],
// staged in LDS; a flat one (or, for the linearization and the sensitivity, no terrain list at all) still evaluates plant_residual, so
// its result is the FLAT one (a branch that is uniform over the workgroup).  ENV: plant_residual_centroidal_env on flat ground,
// centroidal_quadruped_box (nz = 66) and centroidal_quadruped_wall (nz = 114).  WALLS: plant_residual_walls on flat ground, pushbot and
// walledcartpole.
enum { GROUND_FLAT, GROUND_TERRAIN, GROUND_ENV, GROUND_WALLS };

// The sizes (NZ, NTH) the per-lane z, r and theta copies and the LDS arrays of an instantiation are built at.  The two override macros
// build hopper_3D or the walled models at the shared size for the comparisons of DESIGN.md section 5.5 (EXTRA=-DCIMPC_NZ_HOPPER_3D=66).
constexpr int NZM = PLANT_MAX_Q + 4 * PLANT_NC + 2 * PLANT_NB;                       // 66 (centroidal); the planar models have 43, hopper_2D 12
constexpr int NTHM = 2 * PLANT_MAX_Q + PLANT_MAX_U + PLANT_NW + 2;                   // 53
constexpr int NZ_WALL = PLANT_MAX_Q + 4 * PLANT_WALL_NC + 2 * PLANT_WALL_NB;         // 114: centroidal_quadruped_wall, with NTHM
#ifndef CIMPC_NZ_HOPPER_3D
#define CIMPC_NZ_HOPPER_3D (7 + 4 + 8)      // 19
#endif
#ifndef CIMPC_NZ_WALLS
#define CIMPC_NZ_WALLS (4 + 8 + 8)          // 20
#endif
constexpr int NZ_HOPPER_3D = CIMPC_NZ_HOPPER_3D, NTH_HOPPER_3D = 22;
constexpr int NZ_WALLS = CIMPC_NZ_WALLS, NTH_WALLS = 15;                             // walledcartpole; pushbot has 18 and 10
static_assert(NZ_HOPPER_3D >= 19, "hopper_3D: nz = 19");
static_assert(NZ_WALLS >= 20, "walledcartpole: nz = 20");
constexpr int TERRAIN_WORDS = (int)(sizeof(cimpc_terrain) / sizeof(double));
static_assert(sizeof(cimpc_terrain) % sizeof(double) == 0 && TERRAIN_WORDS <= 64, "a terrain is staged one word per lane");

// The instantiation a model runs on.  on_terrain: the terrain list reaches the device - the step kernel's `rough` (some terrain is not
// flat, or particle_2D), the other two kernels' d_ter != nullptr.  for_step: hopper_3D has a size of its own on terrain only - on flat
// ground it measured 1.8 % slower than on the shared FLAT instantiation and stays there; the linearization and
// the sensitivity always give it its own size, and their TERRAIN instantiation takes a null terrain list.
struct PlantInstance { int NZ, NTH, GROUND; };
constexpr PlantInstance plant_instance(const PlantModel& M, bool on_terrain, bool for_step) {
    if (M.kind == PLANT_KIND_PUSHBOT || M.kind == PLANT_KIND_WALLEDCARTPOLE) return {NZ_WALLS, NTH_WALLS, GROUND_WALLS};
    if (M.kind == PLANT_KIND_HOPPER_3D && (on_terrain || !for_step)) return {NZ_HOPPER_3D, NTH_HOPPER_3D, GROUND_TERRAIN};
    if (M.kind == PLANT_KIND_CENTROIDAL_BOX) return {NZM, NTHM, GROUND_ENV};
    if (M.kind == PLANT_KIND_CENTROIDAL_WALL) return {NZ_WALL, NTHM, GROUND_ENV};
    return {NZM, NTHM, on_terrain ? GROUND_TERRAIN : GROUND_FLAT};
}

// An instance as a type: f(tag) reads tag.NZ, tag.NTH and tag.GROUND as constants.
template <int NZ_, int NTH_, int GROUND_>
struct PlantInstanceTag { static constexpr int NZ = NZ_, NTH = NTH_, GROUND = GROUND_; };

// Calls f with the tag of plant_instance(M, on_terrain, for_step) and returns what it returns; false without calling it when the model
// does not fit its instance (a kernel would leave its outputs unwritten).  The six tags below are every instantiation there is: a
// kernel template that f launches is built exactly six times.
template <class F>
bool plant_visit_instance(const PlantModel& M, bool on_terrain, bool for_step, F&& f) {
    const PlantInstance w = plant_instance(M, on_terrain, for_step);
    if (M.nz() > w.NZ || M.nth() > w.NTH) return false;
    auto is = [&](auto tag) { return tag.NZ == w.NZ && tag.NTH == w.NTH && tag.GROUND == w.GROUND; };
    if (PlantInstanceTag<NZ_WALLS, NTH_WALLS, GROUND_WALLS> t; is(t)) return f(t);
    if (PlantInstanceTag<NZ_HOPPER_3D, NTH_HOPPER_3D, GROUND_TERRAIN> t; is(t)) return f(t);
    if (PlantInstanceTag<NZM, NTHM, GROUND_ENV> t; is(t)) return f(t);
    if (PlantInstanceTag<NZ_WALL, NTHM, GROUND_ENV> t; is(t)) return f(t);
    if (PlantInstanceTag<NZM, NTHM, GROUND_TERRAIN> t; is(t)) return f(t);
    return f(PlantInstanceTag<NZM, NTHM, GROUND_FLAT>{});
}

#if defined(__HIPCC__)
// Terrain i of the list into the workgroup's LDS copy, a word per lane (lanes 0 .. TERRAIN_WORDS - 1); the caller synchronizes.
__device__ __forceinline__ void plant_stage_terrain(cimpc_terrain& ter, const cimpc_terrain* terrain, int n_terrain, int i, int lane) {
    const double* src = reinterpret_cast<const double*>(terrain + (n_terrain == 1 ? 0 : i));
    if (lane < TERRAIN_WORDS) reinterpret_cast<double*>(&ter)[lane] = src[lane];
}

// Whether the staged terrain is evaluated at all: particle_2D has no flat residual, every other model's flat terrain is plant_residual.
__device__ __forceinline__ bool plant_rough(const PlantModel& M, const cimpc_terrain& ter) {
    return ter.kind != CIMPC_TERRAIN_FLAT || M.kind == PLANT_KIND_PARTICLE_2D;
}

// r(z, theta, kappa) on the ground of the instantiation; `ter` and `rough` are read by GROUND_TERRAIN alone.  plant_step_kernel spells
// the same dispatch out in its own lambda: through this helper pushbot's step came out with other bits.
template <int GROUND, class T, class TH>
__device__ __forceinline__ void plant_ground_residual(const PlantModel& M, const cimpc_terrain& ter, bool rough, const T* z, const TH* theta,
                                                      double kappa, T* r) {
    if constexpr (GROUND == GROUND_ENV) plant_residual_centroidal_env<T>(M, z, theta, kappa, r);
    else if constexpr (GROUND == GROUND_WALLS) plant_residual_walls<T>(M, z, theta, kappa, r);
    else {
        if constexpr (GROUND == GROUND_TERRAIN) if (rough) return plant_residual_terrain<T>(M, ter, z, theta, kappa, r);
        plant_residual<T>(M, z, theta, kappa, r);
    }
}

// The seed of Jacobian column c of [dr/dz | dr/dtheta]: (z, theta) on dual numbers with tangent 1 on z[c], or on theta[c - nz].
__device__ __forceinline__ void plant_seed_column(int nz, int nth, const double* z, const double* theta, int c, Dual* zl, DualTh* tl) {
    for (int i = 0; i < nz; ++i) zl[i] = {z[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nth; ++i) tl[i] = {{theta[i], nz + i == c ? 1.0 : 0.0}};
}
#endif

}  // namespace cimpc
