// One knot's packed linearization table (lin_table.h) from (z0, th0, r0, rz0, rth0), stated once for a TEAM of workers and run by
// all who build a table: the device kernel (lin_table_build.hip: a workgroup per knot), cimpc_set_linearization (cimpc_host.cpp: a
// team of one, SoloTeam) and a host program (tests/native/lin_table_build_check.cpp: SoloTeam too).  Every element of the table
// has one operation chain whatever the team - the pivot choice, the skipped rows, plain multiply then add where the text writes
// `s += a * b`, a correctly rounded fma where it writes std::fma, the even / odd partial sums of Gs - so the table does not depend
// by a bit on who built it (tests/golden/lin_table_sha256.json records it); the work is only spread over the team where elements
// are independent.
//
// Team: rank() in [0, size()), sync() a barrier of the team that also orders its memory operations (__syncthreads).
#pragma once
#include <cmath>

#include "lin_table.h"

// no contraction in this header's arithmetic: a * b + c rounds twice unless it is spelled fma
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#define LTB_HD __host__ __device__
#else
#define LTB_HD
#endif

// the reductions read rz0 and rth0 from global memory on the device: n loads in flight (the terms are still added in order)
#ifdef __clang__
#define LTB_PRAGMA(x) _Pragma(#x)
#define LTB_UNROLL(n) LTB_PRAGMA(unroll n)
#else
#define LTB_UNROLL(n)
#endif

namespace cimpc {

// the team of one: a host caller
struct SoloTeam {
    LTB_HD int rank() const { return 0; }
    LTB_HD int size() const { return 1; }
    LTB_HD void sync() const {}
};

// The walk of member `me` of `np` over the elements e = r * C + c of an R x C block that it owns, e = me, me + np, ...
// (consecutive members take consecutive elements), row by row:
//     for (TeamWalk w(C, me, np); w.r < R; w.next_row())
//         for (; w.c < C; w.c += np) ... element (w.r, w.c)
// Two divisions by C for the whole block, none per element: a team of one walks plain nested loops, a team wider than a row
// visits one element per row it stops at.
struct TeamWalk {
    int r, c;               // where the member stands; c >= C: past the row's end by that much
    int C, rows, cols;      // of the np elements from one of its elements to the next, `rows` whole rows = `cols` elements
    LTB_HD TeamWalk(int C_, int me, int np) : r(0), c(me), C(C_), rows(C_ > 0 ? np / C_ : 1), cols(rows * C_) {
        if (C > 0) { r = me / C; c = me - r * C; }
    }
    LTB_HD void next_row() {      // from c in [C, C + np), where a row's elements leave it, to the row of the next one
        r += rows;
        c -= cols;
        if (c >= C) { c -= C; ++r; }
    }
};

template <class F>
LTB_HD inline void team_for(int R, int C, int me, int np, F body) {
    for (TeamWalk w(C, me, np); w.r < R; w.next_row())
        for (; w.c < C; w.c += np) body(w.r, w.c);
}

// doubles of lin_invert's workspace: [A | I] (n x 2 n, row-major) and the multipliers of one elimination step (n)
LTB_HD inline size_t lin_invert_work_doubles(int n) { return (size_t)2 * n * n + n; }

// doubles of the team's shared workspace: lin_invert's for Dx (its right half ends as inv(Dx)), CAi (ny x nx) and CAiB (ny x ny),
// both column-major
LTB_HD inline size_t lin_table_work_doubles(int nx, int ny) {
    return lin_invert_work_doubles(nx) + (size_t)ny * nx + (size_t)ny * ny;
}

// Gauss-Jordan with partial pivoting: the inverse of A (n x n, column-major with leading dimension lda) into the right half of
// M = [A | I] (work: shared by the team, lin_invert_work_doubles(n); element (r, c) of the inverse at M[r * 2 n + n + c]).
// Returns false - the same value on every member - at a zero or non-finite pivot; M then holds nothing of use.
template <class Team>
LTB_HD bool lin_invert(const double* A, int lda, int n, double* work, Team team) {
    const int n2 = 2 * n, me = team.rank(), np = team.size();
    double* M = work;                         // at(r, c) = M[r * n2 + c]
    double* fcol = M + (size_t)n * n2;        // column k of M as the step found it
    team_for(n, n, me, np, [&](int c, int r) {
        M[(size_t)r * n2 + c] = A[r + (size_t)c * lda];
        M[(size_t)r * n2 + n + c] = (r == c) ? 1.0 : 0.0;
    });
    team.sync();
    const TeamWalk rows_of_step(n2, me, np);      // every step walks the same n x n2 elements
    for (int k = 0; k < n; ++k) {
        // every member finds the pivot row for itself: the first row with the strictly largest |a|
        int p = k;
        for (int r = k + 1; r < n; ++r)
            if (std::fabs(M[(size_t)r * n2 + k]) > std::fabs(M[(size_t)p * n2 + k])) p = r;
        const double piv = M[(size_t)p * n2 + k], akk = M[(size_t)k * n2 + k];
        if (piv == 0.0 || !std::isfinite(piv)) return false;
        for (int r = me; r < n; r += np) fcol[r] = M[(size_t)r * n2 + k];      // the multipliers, read before any row changes
        team.sync();
        double* Mk = M + (size_t)k * n2;
        double* Mp = M + (size_t)p * n2;
        for (int c = me; c < n2; c += np) {               // rows p and k change places, row k is divided by the pivot
            const double a = Mp[c];
            if (p != k) Mp[c] = Mk[c];
            Mk[c] = a / piv;
        }
        team.sync();
        for (TeamWalk w = rows_of_step; w.r < n; w.next_row()) {   // team_for, with what a row's elements share taken once per row
            const int r = w.r;
            const double f = (r == p) ? akk : fcol[r];    // at(r, k) after the exchange
            const bool skip = r == k || f == 0.0;
            double* Mr = M + (size_t)r * n2;
            for (; w.c < n2; w.c += np)
                if (!skip) Mr[w.c] -= f * Mk[w.c];
        }
        team.sync();
    }
    return true;
}

// Builds table T (L.size doubles) of one knot.  rz0: nz x nz, rth0: nz x nth, column-major (nz = nx + 2 ny).  work: shared by the
// team, lin_table_work_doubles(nx, ny).  Returns false - the same value on every member - where lin_invert refuses Dx; T then
// holds nothing of use.
template <class Team>
LTB_HD bool lin_table_build_knot(const LinLayout& L, const double* z0, const double* th0, const double* r0, const double* rz0,
                                 const double* rth0, double* work, double* T, Team team) {
    const int nx = L.nx, ny = L.ny, nth = L.nth, G = L.G, nz = nx + 2 * ny, n2 = 2 * nx;
    const int me = team.rank(), np = team.size();
    const double* M = work;                   // [Dx | I]
    double* CAi = work + lin_invert_work_doubles(nx);
    double* CAiB = CAi + (size_t)ny * nx;
    auto RZ = [&](int r, int c) { return rz0[r + (size_t)c * nz]; };
    auto RTH = [&](int r, int c) { return rth0[r + (size_t)c * nz]; };
    auto AI = [&](int r, int c) { return M[(size_t)r * n2 + nx + c]; };

    for (int e = me; e < L.size; e += np) T[e] = 0.0;      // the padding that lanes beyond nx / ny read
    if (!lin_invert(rz0, nz, nx, work, team)) return false;

    // CAi = Rx * Ai ; CAiB = (Rx * Ai) * Dy1   (schur.jl:40-41)
    team_for(nx, ny, me, np, [&](int c, int r) {
        double s = 0.0;
        LTB_UNROLL(4) for (int k = 0; k < nx; ++k) s += RZ(nx + r, k) * AI(k, c);
        CAi[r + (size_t)c * ny] = s;
    });
    team.sync();
    team_for(ny, ny, me, np, [&](int c, int r) {
        double s = 0.0;
        LTB_UNROLL(8) for (int k = 0; k < nx; ++k) s += CAi[r + (size_t)k * ny] * RZ(k, nx + c);
        CAiB[r + (size_t)c * ny] = s;
    });
    team.sync();

    // the table, block by block; consecutive members write consecutive doubles
    team_for(ny, ny, me, np, [&](int i, int j) {          // W = Ry1 - CAiB, row i at i * ldw, diagonal kept apart
        T[L.oW + i * L.ldw + j] = (i == j) ? 0.0 : RZ(nx + i, nx + j) - CAiB[i + (size_t)j * ny];
    });
    team_for(nx, ny, me, np, [&](int k, int i) {
        T[L.oCAi + k * G + i] = CAi[i + (size_t)k * ny];
        T[L.oRx + k * G + i] = RZ(nx + i, k);
    });
    team_for(nx, nx, me, np, [&](int k, int i) {
        T[L.oAi + k * G + i] = AI(i, k);
        T[L.oDx + k * G + i] = RZ(i, k);
    });
    team_for(ny, nx, me, np, [&](int k, int i) { T[L.oDy1 + k * G + i] = RZ(i, nx + k); });
    team_for(ny, ny, me, np, [&](int k, int i) { T[L.oRy1 + k * G + i] = RZ(nx + i, nx + k); });
    team_for(nth, nx, me, np, [&](int k, int i) { T[L.oRthDyn + k * G + i] = RTH(i, k); });
    team_for(nth, ny, me, np, [&](int k, int i) { T[L.oRthRst + k * G + i] = RTH(nx + i, k); });
    // right-hand sides of the sensitivity pass (lin_table.h: oGs): Gs[i, c] = (CAi rthdyn[:, c])_i - rthrst[i, c] in two partial sums
    // over even / odd k, correctly rounded multiply-adds - the kernel's own chain (IpSolver::schur_solve), so that the columns the
    // sweep writes do not change by a bit
    auto gs = [&](int c, int i) {
        double bq[2] = {0.0, 0.0};
        LTB_UNROLL(8) for (int k = 0; k < nx; ++k) bq[k & 1] = std::fma(RTH(k, c), CAi[i + (size_t)k * ny], bq[k & 1]);
        return (bq[0] + bq[1]) - RTH(nx + i, c);
    };
    if (L.gst) team_for(ny, L.nths, me, np, [&](int i, int c) { T[L.oGs + i * L.nths + c] = gs(c, i); });
    else team_for(L.nths, ny, me, np, [&](int c, int i) { T[L.oGs + c * G + i] = gs(c, i); });
    // constants of the adjoint form of the sensitivity pass (lin_table.h: oK0, oAiB)
    if (L.adj) {
        team_for(L.nths, nx, me, np, [&](int c, int i) {
            double s = 0.0;
            LTB_UNROLL(8) for (int k = 0; k < nx; ++k) s = std::fma(AI(i, k), RTH(k, c), s);
            T[L.oK0 + c * nx + i] = s;
        });
        team_for(nx, ny, me, np, [&](int i, int k) {
            double s = 0.0;
            LTB_UNROLL(8) for (int m = 0; m < nx; ++m) s = std::fma(AI(i, m), RZ(m, nx + k), s);
            T[L.oAiB + i * ny + k] = s;
        });
    }
    for (int i = me; i < ny; i += np) {
        T[L.oVec + LinLayout::V_RY2 * G + i] = RZ(nx + i, nx + ny + i);
        T[L.oVec + LinLayout::V_RY1D * G + i] = RZ(nx + i, nx + i);
        T[L.oVec + LinLayout::V_CAIBD * G + i] = CAiB[i + (size_t)i * ny];
        T[L.oVec + LinLayout::V_RRST0 * G + i] = r0[nx + i];
        T[L.oVec + LinLayout::V_Y10 * G + i] = z0[nx + i];
        T[L.oVec + LinLayout::V_Y20 * G + i] = z0[nx + ny + i];
    }
    for (int i = me; i < nx; i += np) {
        T[L.oVec + LinLayout::V_RDYN0 * G + i] = r0[i];
        T[L.oVec + LinLayout::V_X0 * G + i] = z0[i];
    }
    for (int k = me; k < nth; k += np) T[L.oTh0 + k] = th0[k];
    return true;
}

#ifdef __HIPCC__
// lin_table_build.hip: N knots, a workgroup each, on `st`.  All pointers are device memory: z0 N x nz, th0 N x nth, r0 N x nz,
// rz0 N x (nz x nz), rth0 N x (nz x nth); tables N x L.size; status[k] = 0, or 1 where Dx of knot k is singular.  No
// synchronization.  False: the launch failed (or the dimensions ask for more LDS than a CU has).
bool lin_table_build_launch(const LinLayout& L, int N, const double* z0, const double* th0, const double* r0, const double* rz0,
                            const double* rth0, double* tables, int* status, hipStream_t st);
#endif

}  // namespace cimpc
