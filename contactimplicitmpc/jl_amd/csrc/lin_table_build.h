// One knot's packed linearization table (lin_table.h) from (z0, th0, r0, rz0, rth0): the arithmetic of cimpc_set_linearization
// (cimpc_host.cpp) stated once for a TEAM of workers, so that the device kernel (lin_table_build.hip: a workgroup per knot) and
// a host program (tests/native/lin_table_build_check.cpp: a team of one) run the same text.  Every element of the table goes
// through the operation chain the host packer gives it - the same pivot choice, the same skipped rows, plain multiply then add
// where the packer writes `s += a * b`, a correctly rounded fma where it writes std::fma, the even / odd partial sums of Gs - so
// the table is the packer's bit for bit; the work is only spread over the team where the packer's loops are independent.
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

namespace cimpc {

// doubles of the team's shared workspace: [Dx | I] (nx x 2 nx, row-major; its right half ends as inv(Dx)), the multipliers of
// one elimination step (nx), CAi (ny x nx) and CAiB (ny x ny), both column-major
LTB_HD inline size_t lin_table_work_doubles(int nx, int ny) {
    return (size_t)2 * nx * nx + nx + (size_t)ny * nx + (size_t)ny * ny;
}

// Builds table T (L.size doubles) of one knot.  rz0: nz x nz, rth0: nz x nth, column-major (nz = nx + 2 ny).  work: shared by the
// team, lin_table_work_doubles(nx, ny).  Returns false - the same value on every member - where the packer's invert() refuses
// Dx (a zero or non-finite pivot); T then holds nothing of use.
template <class Team>
LTB_HD bool lin_table_build_knot(const LinLayout& L, const double* z0, const double* th0, const double* r0, const double* rz0,
                                 const double* rth0, double* work, double* T, Team team) {
    const int nx = L.nx, ny = L.ny, nth = L.nth, G = L.G, nz = nx + 2 * ny, n2 = 2 * nx;
    const int me = team.rank(), np = team.size();
    double* M = work;                         // at(r, c) = M[r * n2 + c]
    double* fcol = M + (size_t)nx * n2;       // column k of M as the step found it
    double* CAi = fcol + nx;
    double* CAiB = CAi + (size_t)ny * nx;
    auto RZ = [&](int r, int c) { return rz0[r + (size_t)c * nz]; };
    auto RTH = [&](int r, int c) { return rth0[r + (size_t)c * nz]; };
    auto AI = [&](int r, int c) { return M[(size_t)r * n2 + nx + c]; };

    for (int e = me; e < L.size; e += np) T[e] = 0.0;      // the padding that lanes beyond nx / ny read
    for (int e = me; e < nx * nx; e += np) {
        const int r = e % nx, c = e / nx;
        M[(size_t)r * n2 + c] = RZ(r, c);
        M[(size_t)r * n2 + nx + c] = (r == c) ? 1.0 : 0.0;
    }
    team.sync();

    // invert(): Gauss-Jordan with partial pivoting on [Dx | I]
    for (int k = 0; k < nx; ++k) {
        // every member finds the pivot row for itself: the first row with the strictly largest |a|
        int p = k;
        for (int r = k + 1; r < nx; ++r)
            if (std::fabs(M[(size_t)r * n2 + k]) > std::fabs(M[(size_t)p * n2 + k])) p = r;
        const double piv = M[(size_t)p * n2 + k], akk = M[(size_t)k * n2 + k];
        if (piv == 0.0 || !std::isfinite(piv)) return false;
        for (int r = me; r < nx; r += np) fcol[r] = M[(size_t)r * n2 + k];
        team.sync();
        for (int c = me; c < n2; c += np) {               // rows p and k change places, row k is divided by the pivot
            const double a = M[(size_t)p * n2 + c];
            if (p != k) M[(size_t)p * n2 + c] = M[(size_t)k * n2 + c];
            M[(size_t)k * n2 + c] = a / piv;
        }
        team.sync();
        for (int e = me; e < nx * n2; e += np) {          // the rows of one step are independent
            const int r = e / n2, c = e % n2;
            if (r == k) continue;
            const double f = (r == p) ? akk : fcol[r];    // at(r, k) after the exchange
            if (f == 0.0) continue;
            M[e] -= f * M[(size_t)k * n2 + c];
        }
        team.sync();
    }

    // CAi = Rx * Ai ; CAiB = (Rx * Ai) * Dy1   (schur.jl:40-41)
    for (int e = me; e < ny * nx; e += np) {
        const int r = e % ny, c = e / ny;
        double s = 0.0;
        for (int k = 0; k < nx; ++k) s += RZ(nx + r, k) * AI(k, c);
        CAi[e] = s;
    }
    team.sync();
    for (int e = me; e < ny * ny; e += np) {
        const int r = e % ny, c = e / ny;
        double s = 0.0;
        for (int k = 0; k < nx; ++k) s += CAi[r + (size_t)k * ny] * RZ(k, nx + c);
        CAiB[e] = s;
    }
    team.sync();

    // the table, block by block; consecutive members write consecutive doubles
    for (int e = me; e < ny * ny; e += np) {              // W = Ry1 - CAiB, row i at i * ldw, diagonal kept apart
        const int i = e / ny, j = e % ny;
        T[L.oW + i * L.ldw + j] = (i == j) ? 0.0 : RZ(nx + i, nx + j) - CAiB[i + (size_t)j * ny];
    }
    for (int e = me; e < nx * ny; e += np) {
        const int k = e / ny, i = e % ny;
        T[L.oCAi + k * G + i] = CAi[i + (size_t)k * ny];
        T[L.oRx + k * G + i] = RZ(nx + i, k);
    }
    for (int e = me; e < nx * nx; e += np) {
        const int k = e / nx, i = e % nx;
        T[L.oAi + k * G + i] = AI(i, k);
        T[L.oDx + k * G + i] = RZ(i, k);
    }
    for (int e = me; e < ny * nx; e += np) {
        const int k = e / nx, i = e % nx;
        T[L.oDy1 + k * G + i] = RZ(i, nx + k);
    }
    for (int e = me; e < ny * ny; e += np) {
        const int k = e / ny, i = e % ny;
        T[L.oRy1 + k * G + i] = RZ(nx + i, nx + k);
    }
    for (int e = me; e < nth * nx; e += np) {
        const int k = e / nx, i = e % nx;
        T[L.oRthDyn + k * G + i] = RTH(i, k);
    }
    for (int e = me; e < nth * ny; e += np) {
        const int k = e / ny, i = e % ny;
        T[L.oRthRst + k * G + i] = RTH(nx + i, k);
    }
    // right-hand sides of the sensitivity pass (lin_table.h: oGs): two partial sums over even / odd k, correctly rounded
    // multiply-adds - the kernel's own chain (IpSolver::schur_solve)
    for (int e = me; e < L.nths * ny; e += np) {
        const int c = L.gst ? e % L.nths : e / ny, i = L.gst ? e / L.nths : e % ny;
        double bq[2] = {0.0, 0.0};
        for (int k = 0; k < nx; ++k) bq[k & 1] = std::fma(RTH(k, c), CAi[i + (size_t)k * ny], bq[k & 1]);
        T[L.gst ? L.oGs + i * L.nths + c : L.oGs + c * G + i] = (bq[0] + bq[1]) - RTH(nx + i, c);
    }
    // constants of the adjoint form of the sensitivity pass (lin_table.h: oK0, oAiB)
    if (L.adj) {
        for (int e = me; e < L.nths * nx; e += np) {
            const int c = e / nx, i = e % nx;
            double s = 0.0;
            for (int k = 0; k < nx; ++k) s = std::fma(AI(i, k), RTH(k, c), s);
            T[L.oK0 + c * nx + i] = s;
        }
        for (int e = me; e < nx * ny; e += np) {
            const int i = e / ny, k = e % ny;
            double s = 0.0;
            for (int m = 0; m < nx; ++m) s = std::fma(AI(i, m), RZ(m, nx + k), s);
            T[L.oAiB + i * ny + k] = s;
        }
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
