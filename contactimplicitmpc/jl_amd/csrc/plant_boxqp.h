// The box-constrained step of the limited LQ backward pass: control-limited DDP (Tassa, Mansard, Todorov
// 2014) at one walk step of plant_riccati.h.  With G = Quu + rho I (m x m, column-major, NOT symmetrized), F = [Qux | Qu] (m x (n + 1)),
// the step's bounds lo <= x <= hi on the control change and the previous walk step's k:
//
//   1. lo_i = u_lo[i] - u_nom[i], hi_i = u_hi[i] - u_nom[i], one rounded difference each (null limits: -inf, +inf)
//   2. every lo_i = -inf and every hi_i = +inf: nothing is clamped and no iteration runs.  Otherwise projected Newton on
//      min 0.5 x'(G x) + Qu'x, lo <= x <= hi, from x = limit(k of the previous walk step) (zeros at the first):
//        g_i = Qu_i + sum_j G_ij x_j                          (ascending j from 0.0)
//        c = {i : (x_i == lo_i and g_i > 0) or (x_i == hi_i and g_i < 0)}, f the rest, ascending
//        stop when f is empty or max_f |g_i| <= MIN_GRAD (1 + max_i |Qu_i|)
//        G_ff d_f = -g_f, d_c = 0                             (plant_boxqp_eliminate on a copy of G, then plant_boxqp_backsolve)
//        sdg = sum_f d_i g_i (ascending); not sdg < 0: the chain ends
//        value(v) = 0.5 (sum_i v_i (sum_j G_ij v_j)) + sum_i Qu_i v_i        (every sum ascending from 0.0)
//        step = 1, then step <- step STEP_DEC until value(xc) - value(x) <= ARMIJO (step sdg), xc = limit(x + step d);
//        step < MIN_STEP: the chain ends.  x <- xc.  MAX_ITER iterations without a stop: the chain ends.
//   3. the final solve on the final f: y_i = Qu_i + sum_{j in c} G_ij x_j (ascending j, starting FROM Qu_i), G_ff [K_f | y] = [Qux_f | y]
//      with the elimination of plant_riccati.h over the rows and columns of f; K rows of c are 0.0, k_f = limit(-y), k_c = x_c.
//      With c empty these are the statements of the unlimited chain one for one, so the bits are its bits.
//
// No square root anywhere, no contraction; every sum is one ordered chain, so a host team of one and a workgroup round alike.  The work
// is shared as the bits allow: the matrix-vector products an element per member, the elimination an entry per member, the ordered
// scalar sums (sdg, value, the stopping test) by every member alike from the shared vectors, so no scalar has to be handed round.
// Team: rank(), size(), sync().  A chain that ends returns false from every member at the same statement.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>

#include "plant_feedback.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define PBQ_HD __host__ __device__
#else
#define PBQ_HD
#endif

namespace cimpc {

constexpr int PLANT_BOXQP_MAX_ITER = 100;           // projected-Newton iterations of one walk step
constexpr double PLANT_BOXQP_MIN_GRAD = 1e-8;       // the free gradient's floor, relative to 1 + max |Qu|
constexpr double PLANT_BOXQP_ARMIJO = 0.1;          // the fraction of the linear decrease a step must reach
constexpr double PLANT_BOXQP_STEP_DEC = 0.6;        // the factor of the backtracking search
constexpr double PLANT_BOXQP_MIN_STEP = 1e-22;      // a step below it ends the chain
constexpr int PLANT_BOXQP_MAX_M = 31;               // controls: the clamped set is the bits of an int

// the plan: a second m x m (the copy of G a Newton direction is eliminated in), six m-vectors (lo, hi, x, g, d, xc) and m + 2 ints
// (the free indices, their count, the clamped bits) in m + 2 doubles
PBQ_HD constexpr size_t plant_boxqp_work_doubles(int nu) { return (size_t)nu * nu + 7 * (size_t)nu + 2; }

struct PlantBoxQPWork {
    double *Gw, *lo, *hi, *x, *g, *d, *xc;
    int* idx;      // idx[0 .. m): the free indices ascending; idx[m]: how many; idx[m + 1]: the clamped bits
};
PBQ_HD inline PlantBoxQPWork plant_boxqp_carve(double* w, int m) {
    PlantBoxQPWork W;
    W.Gw = w; W.lo = w + m * m; W.hi = W.lo + m; W.x = W.hi + m; W.g = W.x + m; W.d = W.g + m; W.xc = W.d + m;
    W.idx = reinterpret_cast<int*>(W.xc + m);
    return W;
}

// the team of one: a host caller
struct PlantBoxQPSolo {
    PBQ_HD int rank() const { return 0; }
    PBQ_HD int size() const { return 1; }
    PBQ_HD void sync() const {}
};

PBQ_HD inline bool plant_boxqp_bad_pivot(double pv) { return !(std::fabs(pv) > 0.0) || !std::isfinite(pv); }
PBQ_HD inline bool plant_boxqp_pivot_beats(double a, double b) { return a > b || (a != a && b == b); }

// LU with partial pivoting (the first largest |entry|, l = a_ik (1 / a_kk), a_ij -= l a_kj) over the rows and columns fi[0 .. nf) of A
// (m x m, column-major), carried through the ncol columns of Fm (leading dimension m): the loops of plant_riccati.h's elimination with
// the indices looked up.  false: a zero or non-finite pivot, the same answer for every member.
template <class Team>
PBQ_HD inline bool plant_boxqp_eliminate(const Team& team, double* A, double* Fm, int m, int ncol, const int* fi, int nf) {
    const int me = team.rank(), np = team.size();
    for (int k = 0; k < nf; ++k) {
        const int ck = fi[k];
        double best = -1.0;
        int p = k;
        for (int i = k; i < nf; ++i) {
            const double v = std::fabs(A[ck * m + fi[i]]);
            if (plant_boxqp_pivot_beats(v, best)) { best = v; p = i; }
        }
        team.sync();
        if (p != k) {
            const int rp = fi[p];
            for (int j = k + me; j < nf + ncol; j += np) {
                double* col = j < nf ? A + fi[j] * m : Fm + (j - nf) * m;
                const double v = col[ck]; col[ck] = col[rp]; col[rp] = v;
            }
        }
        team.sync();
        const double pv = A[ck * m + ck];
        if (plant_boxqp_bad_pivot(pv)) return false;
        const double rcp = 1.0 / pv;
        const int rem = nf - k - 1;
        for (int e = me; e < rem * (rem + ncol); e += np) {      // (i, j), i fastest
            const int i = fi[k + 1 + e % rem], j = k + 1 + e / rem;
            const double l = A[ck * m + i] * rcp;
            double* col = j < nf ? A + fi[j] * m : Fm + (j - nf) * m;
            col[i] -= l * col[ck];
        }
        team.sync();
    }
    return true;
}

// U x = col over fi, in place: s -= u_kj x_j ascending j, then s / u_kk.  true: every entry finite.
PBQ_HD inline bool plant_boxqp_backsolve(const double* A, double* col, int m, const int* fi, int nf) {
    bool finite = true;
    for (int k = nf - 1; k >= 0; --k) {
        const int rk = fi[k];
        double a = col[rk];
        for (int j = k + 1; j < nf; ++j) a -= A[fi[j] * m + rk] * col[fi[j]];
        a /= A[rk * m + rk];
        col[rk] = a;
        finite = finite && std::isfinite(a);
    }
    return finite;
}

// 0.5 v'(G v) + Qu'v
PBQ_HD inline double plant_boxqp_value(const double* G, const double* Qu, const double* v, int m) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < m; ++i) {
        double y = 0.0;
        for (int j = 0; j < m; ++j) y += G[j * m + i] * v[j];
        a += v[i] * y;
    }
    for (int i = 0; i < m; ++i) b += Qu[i] * v[i];
    return 0.5 * a + b;
}

// One walk step.  In: G (m x m), F = [Qux | Qu] (m x (n + 1)), Qu (m), kv = k of the previous walk step (first: none), u_lo, u_hi and
// u_nom this robot's rows of this step (u_lo null: no limits).  Out: F = [K | .] with the rows of the clamped set 0.0, KT = K' (n x m),
// kv = k; W.idx[m + 1] the clamped bits; *finite is cleared by a member that computed a non-finite entry of K or k.  G is overwritten
// by its factors.  The caller synchronizes the team before it reads the outputs.  false: this robot's chain ends here.
template <class Team>
PBQ_HD inline bool plant_boxqp_step(const Team& team, int m, int n, double* G, double* F, const double* Qu, double* kv, double* KT,
                                    const PlantBoxQPWork& W, const double* u_lo, const double* u_hi, const double* u_nom, bool first, bool* finite) {
    const int me = team.rank(), np = team.size();
    const double inf = std::numeric_limits<double>::infinity();
    int* fi = W.idx;
    for (int i = me; i < m; i += np) {
        const double lo = u_lo ? u_lo[i] - u_nom[i] : -inf, hi = u_lo ? u_hi[i] - u_nom[i] : inf;
        W.lo[i] = lo;
        W.hi[i] = hi;
        W.x[i] = plant_feedback_limit(first ? 0.0 : kv[i], lo, hi);
    }
    if (me == 0) {
        for (int i = 0; i < m; ++i) fi[i] = i;
        fi[m] = m;
        fi[m + 1] = 0;
    }
    team.sync();
    bool open = true;
    for (int i = 0; i < m; ++i) open = open && W.lo[i] == -inf && W.hi[i] == inf;
    if (!open) {
        double qmax = 0.0;
        for (int i = 0; i < m; ++i) {
            const double a = std::fabs(Qu[i]);
            if (a > qmax) qmax = a;
        }
        const double floor = PLANT_BOXQP_MIN_GRAD * (1.0 + qmax);
        bool done = false;
        for (int it = 0; it < PLANT_BOXQP_MAX_ITER && !done; ++it) {
            for (int i = me; i < m; i += np) {
                double a = 0.0;
                for (int j = 0; j < m; ++j) a += G[j * m + i] * W.x[j];
                W.g[i] = Qu[i] + a;
            }
            team.sync();
            if (me == 0) {
                int nf = 0, mask = 0;
                for (int i = 0; i < m; ++i) {
                    const bool c = (W.x[i] == W.lo[i] && W.g[i] > 0.0) || (W.x[i] == W.hi[i] && W.g[i] < 0.0);
                    if (c) mask |= 1 << i;
                    else fi[nf++] = i;
                }
                fi[m] = nf;
                fi[m + 1] = mask;
            }
            team.sync();
            const int nf = fi[m], mask = fi[m + 1];
            double gmax = 0.0;
            for (int jj = 0; jj < nf; ++jj) {
                const double a = std::fabs(W.g[fi[jj]]);
                if (!(a <= gmax)) gmax = a;      // a NaN stays
            }
            if (nf == 0 || gmax <= floor) { done = true; break; }
            for (int e = me; e < m * m; e += np) W.Gw[e] = G[e];
            for (int i = me; i < m; i += np) W.d[i] = (mask >> i) & 1 ? 0.0 : -W.g[i];
            team.sync();
            if (!plant_boxqp_eliminate(team, W.Gw, W.d, m, 1, fi, nf)) return false;
            if (me == 0) plant_boxqp_backsolve(W.Gw, W.d, m, fi, nf);
            team.sync();
            double sdg = 0.0;
            for (int jj = 0; jj < nf; ++jj) sdg += W.d[fi[jj]] * W.g[fi[jj]];
            if (!(sdg < 0.0)) return false;      // not a descent direction (or not a number)
            const double fo = plant_boxqp_value(G, Qu, W.x, m);
            double step = 1.0;
            bool took = false;
            while (step >= PLANT_BOXQP_MIN_STEP) {
                for (int i = me; i < m; i += np) W.xc[i] = plant_feedback_limit(W.x[i] + step * W.d[i], W.lo[i], W.hi[i]);
                team.sync();
                const double fn = plant_boxqp_value(G, Qu, W.xc, m);
                if (fn - fo <= PLANT_BOXQP_ARMIJO * (step * sdg)) { took = true; break; }
                step *= PLANT_BOXQP_STEP_DEC;
                team.sync();                     // xc's readers are done
            }
            if (!took) return false;
            for (int i = me; i < m; i += np) W.x[i] = W.xc[i];
            team.sync();
        }
        if (!done) return false;
    }
    // the final solve on the final free set
    const int nf = fi[m], mask = fi[m + 1];
    if (mask) {
        for (int i = me; i < m; i += np)
            if (!((mask >> i) & 1)) {
                double a = Qu[i];
                for (int j = 0; j < m; ++j)
                    if ((mask >> j) & 1) a += G[j * m + i] * W.x[j];
                F[n * m + i] = a;
            }
        team.sync();
    }
    if (!plant_boxqp_eliminate(team, G, F, m, n + 1, fi, nf)) return false;
    for (int c = me; c < n + 1; c += np) {       // U K = F over the free set, a column per member
        double* col = F + c * m;
        if (!plant_boxqp_backsolve(G, col, m, fi, nf)) *finite = false;
        for (int i = 0; i < m; ++i) {
            const bool clamped = (mask >> i) & 1;
            if (clamped) col[i] = 0.0;
            if (c < n) KT[i * n + c] = col[i];
            else kv[i] = clamped ? W.x[i] : plant_feedback_limit(-col[i], W.lo[i], W.hi[i]);
        }
    }
    return true;
}

}  // namespace cimpc
