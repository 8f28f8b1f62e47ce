// Partial pivoting of an LU factorization held in LDS, as gains.hip (gains_dynamics_kernel, tvlqr_kernel) and
// plant_sensitivity.hip (plant_sensitivity_kernel) do it.  The pieces here compare and select only - no arithmetic that could
// contract - so they mean the same in a translation unit that contracts and in one that does not; the elimination and the
// back-substitution stay with each kernel, whose layouts and roundings differ on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>

namespace cimpc {

__device__ inline bool bad_pivot(double pv) { return !(fabs(pv) > 0.0) || !isfinite(pv); }
// |a| beats |b| in a pivot search: larger, or not a number (which then stays: the pivot test refuses it)
__device__ inline bool pivot_beats(double a, double b) { return a > b || (a != a && b == b); }

// The pivot row of column k: the first largest |W(i, k)|, k <= i < n, of a row-major W with rows of ld words.  Called by the 64 lanes
// of the workgroup's first wavefront (threadIdx.x < 64), every one of which gets the row.
__device__ inline int lds_pivot_row(const double* W, int ld, int k, int n) {
    double best = -1.0;
    int bi = INT_MAX;
    for (int i = k + (int)threadIdx.x; i < n; i += 64) {
        const double a = fabs(W[i * ld + k]);
        if (pivot_beats(a, best)) { best = a; bi = i; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (pivot_beats(ob, best) || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    return bi;
}

}  // namespace cimpc
