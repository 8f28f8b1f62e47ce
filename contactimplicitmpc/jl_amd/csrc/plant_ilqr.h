// The rules of the iLQR loop, stated ONCE for the kernels of plant_ilqr.hip and a host program
// (tests/native/plant_ilqr_check.cpp): the per-robot bookkeeping that `plant.ilqr` does in NumPy between its backward pass and its line
// search, line for line.
//
// THE STATE of a robot: level (its place on the regularization ladder), active (still updated) and J (its nominal's cost).
// THE LADDER is a table of n_ladder doubles the HOST computes (rho0 rho_factor^j) and uploads once: nothing here evaluates a power, so
// the values are bit for bit the host loop's.  A loop of max_iter iterations reads entries 0 .. max_iter (a robot moves at most one
// level up per iteration), which is what the entry point asks of n_ladder; the functions here do not test the index again.
//
//   rho      = ladder[level]                                                       before the backward pass   (plant_ilqr_rho)
//   J_nom    = active and lq_status == 0 ? J : -inf                                before the line search     (plant_ilqr_nominal_cost)
//   accepted = choice >= 0                                                         after it                   (plant_ilqr_update)
//   J_new    = accepted ? J_cand[choice] : J
//   small    = accepted and (J - J_new < tol |J|)                                  one rounded difference, one rounded product
//   level'   = accepted ? max(level - 1, 0) : (active ? level + 1 : level)
//   active'  = active and not small and ladder[level'] <= rho_max
//   history  = (J_new, accepted ? alpha[choice] : NaN, rho, accepted)
//
// A backward pass that ended early (lq_status != 0) makes J_nom -inf, so no candidate is acceptable: a rejection, one level up.  An
// inactive robot rides along the same way and keeps its level.  No contraction in these functions; the pragma stands inside each body, as
// in plant_cost.h.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>

#ifdef __HIPCC__
#define PILQR_HD __host__ __device__
#else
#define PILQR_HD
#endif

namespace cimpc {

struct PlantIlqrRobot {
    int level, active;
    double J;
};

// one robot's row of the history of an iteration
struct PlantIlqrRow {
    double J, alpha, rho;
    int accepted;
};

PILQR_HD inline double plant_ilqr_rho(const double* ladder, int level) { return ladder[level]; }

PILQR_HD inline double plant_ilqr_nominal_cost(int active, int lq_status, double J) {
    return (active && lq_status == 0) ? J : -std::numeric_limits<double>::infinity();
}

// The robot after an iteration whose line search chose `choice` (-1: no acceptable candidate) among candidates of cost J_cand[c J_stride]
// and step length alpha[c]; returns the iteration's history row.  level' must be an index of the ladder (see above).
PILQR_HD inline PlantIlqrRow plant_ilqr_update(PlantIlqrRobot* s, int choice, const double* J_cand, size_t J_stride, const double* alpha,
                                               const double* ladder, double rho_max, double tol) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const bool accepted = choice >= 0, active = s->active != 0;
    const double J = s->J, J_new = accepted ? J_cand[(size_t)choice * J_stride] : J;
    const PlantIlqrRow row{J_new, accepted ? alpha[choice] : std::numeric_limits<double>::quiet_NaN(), plant_ilqr_rho(ladder, s->level), accepted ? 1 : 0};
    const double decrease = J - J_new, bound = tol * std::fabs(J);
    const bool small = accepted && decrease < bound;
    const int level = accepted ? (s->level - 1 > 0 ? s->level - 1 : 0) : (active ? s->level + 1 : s->level);
    s->level = level;
    s->active = (active && !small && ladder[level] <= rho_max) ? 1 : 0;
    s->J = J_new;
    return row;
}

// What cimpc_plant_ilqr refuses of the loop's own arguments before any device is touched; the reason, or null.
inline const char* plant_ilqr_refusal(int max_iter, int n_ladder, const double* ladder, double rho_max, double tol) {
    if (max_iter < 1) return "max_iter below 1";
    if (!ladder) return "null ladder";
    if (n_ladder < 1 || (long long)n_ladder < (long long)max_iter + 1) return "a ladder shorter than max_iter + 1";
    for (int j = 0; j < n_ladder; ++j)
        if (!(ladder[j] >= 0.0) || !std::isfinite(ladder[j])) return "a ladder entry that is negative or not finite";
    if (rho_max != rho_max || tol != tol) return "rho_max or tol not a number";
    return nullptr;
}

}  // namespace cimpc
