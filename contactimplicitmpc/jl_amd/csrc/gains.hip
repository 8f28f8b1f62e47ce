// Time-varying LQR feedback gains along the reference trajectory: reference_gains / tvlqr of src/controller/gains.jl:1-51 and the
// feedback line of examples/centroidal_quadruped/continuous_policy_v3.jl:74-85.
//
//   gains_dynamics_kernel   one workgroup per knot: the q rows of dz/dtheta = -rz \ rtheta (gains.jl:31-39) by LU with partial pivoting in
//                           LDS, in the ADJOINT form - only nq rows of the solution are consumed, so nq right-hand sides go through
//                           rz^T (Y = rz^-T E) and one product D = -Y^T rtheta[:, 1:2nq+nu] follows, instead of 2nq + nu + ... columns
//                           through rz.  Written out as the blocks the Riccati chain reads (gains.jl:41-42):
//                           A_t = [0 I; D1 D2] (2nq x 2nq), B_t = [0; Du] (2nq x nu).
//   tvlqr_kernel            one workgroup per problem walking the T - 1 steps backwards (gains.jl:8-12) with P and the step's
//                           matrices in LDS; A_t, B_t are read as A[t mod n_ab] (the N repeats of gains.jl:22-23 cost no memory).
//   gain_latch_kernel, gain_feedback_kernel   the policy's two calls (cimpc_gain_latch, cimpc_gain_feedback), a workgroup per rollout.
//
// LDS: the dynamics kernel holds rz^T (nz^2), the nq right-hand sides (nz nq) and one multiplier column - 121 KB at nz = 114, nq = 18
// (centroidal_quadruped_wall), 47 KB at nz = 66; the Riccati kernel 4 n^2 + 6 n m + 2 m^2 doubles - 64 KB at n = 36, m = 12, 113 KB at
// the largest size it takes (48, 16).  Both run one workgroup per CU at those sizes; the chain is a latency chain and the knots are few.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/cimpc.h"
#include "gains.h"
#include "lds_pivot.h"
#include "plant_linearize.h"
#include "plant_workspace.h"

namespace cimpc {

namespace {

constexpr int GAINS_THREADS = 256;
constexpr int GAINS_NO_KNOT = 0x7f7f7f7f;          // the status word of the dynamics kernel as hipMemsetAsync(0x7f) leaves it
constexpr size_t GAINS_MAX_LDS = 160 * 1024;       // of a gfx950 CU

// ---- dz/dtheta of one knot, q rows ---------------------------------------------------------------------------------------------
// rz: H x (nz x nz) column-major, rth: knot t at rth + t * rth_stride, nz x (>= 2nq + nu) column-major.  The flat copy of rz is rz^T
// ROW-major: W(i, j) = W[i nz + j] = rz(j, i), so a row operation runs over consecutive LDS words.  status: the smallest knot whose
// rz has a zero or non-finite pivot, or whose D has a non-finite entry.
__global__ __launch_bounds__(GAINS_THREADS) void gains_dynamics_kernel(int nq, int nu, int nz, const double* rz, const double* rth,
                                                                       size_t rth_stride, double* A, double* B, int* status) {
    extern __shared__ __attribute__((aligned(16))) double gains_lds[];
    double* W = gains_lds;
    double* Y = W + (size_t)nz * nz;       // nz x nq row-major: the right-hand sides E = I[:, 1:nq], then rz^-T E
    double* lcol = Y + (size_t)nz * nq;
    int* ipiv = reinterpret_cast<int*>(lcol + nz);
    const int t = blockIdx.x, tid = threadIdx.x;
    const double* g = rz + (size_t)t * nz * nz;
    for (int e = tid; e < nz * nz; e += GAINS_THREADS) W[e] = g[e];
    for (int e = tid; e < nz * nq; e += GAINS_THREADS) Y[e] = (e / nq == e % nq) ? 1.0 : 0.0;
    __syncthreads();
    const int wcols = nz + nq;             // the augmented row [W_i | Y_i]
    const int tx = tid & 63, ty = tid >> 6;
    for (int k = 0; k < nz; ++k) {
        if (tid < 64) {
            const int bi = lds_pivot_row(W, nz, k, nz);
            if (tid == 0) ipiv[0] = bi;
        }
        __syncthreads();
        const int p = ipiv[0];
        if (p != k)
            for (int j = k + tid; j < wcols; j += GAINS_THREADS) {
                double* a = j < nz ? &W[k * nz + j] : &Y[k * nq + j - nz];
                double* b = j < nz ? &W[p * nz + j] : &Y[p * nq + j - nz];
                const double v = *a; *a = *b; *b = v;
            }
        __syncthreads();
        const double pv = W[k * nz + k];
        if (bad_pivot(pv)) {               // the same word for every thread: all leave together
            if (tid == 0) atomicMin(status, t);
            return;
        }
        const double rp = 1.0 / pv;
        for (int i = k + 1 + tid; i < nz; i += GAINS_THREADS) lcol[i] = W[i * nz + k] * rp;
        __syncthreads();
        for (int i = k + 1 + ty; i < nz; i += GAINS_THREADS / 64) {
            const double l = lcol[i];
            for (int j = k + 1 + tx; j < wcols; j += 64) {
                if (j < nz) W[i * nz + j] -= l * W[k * nz + j];
                else Y[i * nq + j - nz] -= l * Y[k * nq + j - nz];
            }
        }
        __syncthreads();
    }
    {   // U Y = Y: 32 lanes over the columns (nq <= 24), 8 row groups; row k is scaled after its last reader has passed
        const int c = tid & 31, rg = tid >> 5;
        for (int k = nz - 1; k >= 0; --k) {
            const double pv = W[k * nz + k];
            const double yk = c < nq ? Y[k * nq + c] / pv : 0.0;
            __syncthreads();               // every thread holds its y_k before row k is overwritten
            if (c < nq) {
                if (rg == 0) Y[k * nq + c] = yk;
                for (int i = rg; i < k; i += GAINS_THREADS / 32) Y[i * nq + c] -= W[i * nz + k] * yk;
            }
            __syncthreads();
        }
    }
    // D = -Y^T rtheta[:, 1:2nq+nu], scattered into A_t = [0 I; D1 D2] and B_t = [0; Du]
    const int n = 2 * nq, ncol = 2 * nq + nu;
    const double* gth = rth + (size_t)t * rth_stride;
    double* At = A + (size_t)t * n * n;
    double* Bt = B + (size_t)t * n * nu;
    bool finite = true;
    for (int e = tid; e < nq * ncol; e += GAINS_THREADS) {
        const int r = e % nq, c = e / nq;
        double s = 0.0;
        for (int i = 0; i < nz; ++i) s += Y[i * nq + r] * gth[(size_t)c * nz + i];
        s = -s;
        finite = finite && isfinite(s);
        if (c < n) At[c * n + nq + r] = s;
        else Bt[(c - n) * n + nq + r] = s;
    }
    for (int e = tid; e < nq * n; e += GAINS_THREADS) { const int r = e % nq, c = e / nq; At[c * n + r] = (c == r + nq) ? 1.0 : 0.0; }
    for (int e = tid; e < nq * nu; e += GAINS_THREADS) { const int r = e % nq, c = e / nq; Bt[c * n + r] = 0.0; }
    if (!finite) atomicMin(status, t);
}

// ---- the Riccati chain -----------------------------------------------------------------------------------------------------------
struct TvlqrArgs {
    int n, m, T, n_ab, n_q, n_r, n_keep;
    const double *A, *B, *Q, *R;       // problem p at A + p n_ab n^2, B + p n_ab n m, Q + p n_q n^2, R + p n_r m^2
    double *K, *P1;                    // K + p n_keep m n; P1 + p n^2 or null
    int* status;                       // [n_prob]: 0, or the first 1-based step (in walk order, T - 1 first) whose R + B'PB had a zero or
                                       // non-finite pivot, or whose K_t or updated P holds a non-finite entry
    const int* dyn_status;             // null, or the dynamics kernel's word: anything but GAINS_NO_KNOT and the chain is not walked
};

// C(r, c) = sum_k X(r, k) Y(k, c) for a rows x cols result, a TR x TC tile of it per thread: TR + TC LDS reads feed TR TC multiply-adds,
// and the tile's sums are independent chains (a lone workgroup pays the latency of every dependent read).  X and Y are
// given as accessors; every operand below is stored so that X(r, k) runs over consecutive words with r, i.e. with the lane.  Every
// entry is one running sum in the order k = 0, 1, ..., so a problem's result does not depend on the batch it is solved in.
template <int TR, int TC, class FX, class FY, class FOUT>
__device__ inline void tile_product(int rows, int cols, int depth, FX X, FY Y, FOUT out) {
    const int tr = (rows + TR - 1) / TR, tc = (cols + TC - 1) / TC;
    for (int e = threadIdx.x; e < tr * tc; e += GAINS_THREADS) {
        const int r0 = (e % tr) * TR, c0 = (e / tr) * TC;
        int ri[TR], ci[TC];
#pragma unroll
        for (int i = 0; i < TR; ++i) ri[i] = min(r0 + i, rows - 1);      // a tile over the edge repeats the last row / column and drops it
#pragma unroll
        for (int j = 0; j < TC; ++j) ci[j] = min(c0 + j, cols - 1);
        double acc[TR][TC];
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int j = 0; j < TC; ++j) acc[i][j] = 0.0;
#pragma unroll 2
        for (int k = 0; k < depth; ++k) {
            double x[TR], y[TC];
#pragma unroll
            for (int i = 0; i < TR; ++i) x[i] = X(ri[i], k);
#pragma unroll
            for (int j = 0; j < TC; ++j) y[j] = Y(k, ci[j]);
#pragma unroll
            for (int i = 0; i < TR; ++i)
#pragma unroll
                for (int j = 0; j < TC; ++j) acc[i][j] += x[i] * y[j];
        }
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
            for (int j = 0; j < TC; ++j)
                if (r0 + i < rows && c0 + j < cols) out(r0 + i, c0 + j, acc[i][j]);
    }
}

// All matrices column-major.  K_t and A_t - B_t K_t are kept in both orientations (KT, AcT) and B_t transposed (BT), so that the
// products with a transposed left factor read it along the lanes too (a stride of n = 36 doubles is an 8-way bank conflict).
__global__ __launch_bounds__(GAINS_THREADS) void tvlqr_kernel(TvlqrArgs a) {
    extern __shared__ __attribute__((aligned(16))) double gains_lds[];
    const int n = a.n, m = a.m, tid = threadIdx.x, prob = blockIdx.x;
    if (a.dyn_status && *a.dyn_status != GAINS_NO_KNOT) return;
    double* P = gains_lds;             // n x n
    double* Ac = P + n * n;            // n x n: A_t, then A_t - B_t K_t
    double* AcT = Ac + n * n;          // n x n: (A_t - B_t K_t)'
    double* T1 = AcT + n * n;          // n x n: P (A - B K)
    double* Bm = T1 + n * n;           // n x m
    double* BT = Bm + n * m;           // m x n: B_t'
    double* BtP = BT + n * m;          // m x n
    double* F = BtP + n * m;           // m x n: B'PA, then K_t
    double* KT = F + n * m;            // n x m: K_t'
    double* RK = KT + n * m;           // m x n
    double* G = RK + n * m;            // m x m: R + B'PB, then its LU factors
    double* Rm = G + m * m;            // m x m
    const double* Ag = a.A + (size_t)prob * a.n_ab * n * n;
    const double* Bg = a.B + (size_t)prob * a.n_ab * n * m;
    const double* Qg = a.Q + (size_t)prob * a.n_q * n * n;
    const double* Rg = a.R + (size_t)prob * a.n_r * m * m;
    double* Kg = a.K + (size_t)prob * a.n_keep * m * n;
    const int tx = tid & 63, ty = tid >> 6;
    {
        const double* QT = Qg + (a.n_q == 1 ? 0 : (size_t)(a.T - 1) * n * n);      // P[T] = Q[T]
        for (int e = tid; e < n * n; e += GAINS_THREADS) P[e] = QT[e];
    }
    for (int t = a.T - 2; t >= 0; --t) {
        bool finite = true;            // of the entries of K_t and of the updated P this thread computes
        const double* At = Ag + (size_t)(t % a.n_ab) * n * n;
        const double* Bt = Bg + (size_t)(t % a.n_ab) * n * m;
        const double* Rt = Rg + (a.n_r == 1 ? 0 : (size_t)t * m * m);
        const double* Qt = Qg + (a.n_q == 1 ? 0 : (size_t)t * n * n);
        for (int e = tid; e < n * n; e += GAINS_THREADS) Ac[e] = At[e];
        for (int e = tid; e < n * m; e += GAINS_THREADS) { const double v = Bt[e]; Bm[e] = v; BT[(e % n) * m + e / n] = v; }
        for (int e = tid; e < m * m; e += GAINS_THREADS) Rm[e] = Rt[e];
        __syncthreads();
        tile_product<2, 3>(m, n, n, [&](int r, int k) { return BT[k * m + r]; }, [&](int k, int c) { return P[c * n + k]; },
                           [&](int r, int c, double v) { BtP[c * m + r] = v; });                                  // B'P
        __syncthreads();
        tile_product<2, 3>(m, m + n, n, [&](int r, int k) { return BtP[k * m + r]; },
                           [&](int k, int c) { return c < m ? Bm[c * n + k] : Ac[(c - m) * n + k]; },
                           [&](int r, int c, double v) {                                                          // G = R + (B'P) B | F = (B'P) A
                               if (c < m) G[c * m + r] = Rm[c * m + r] + v;
                               else F[(c - m) * m + r] = v;
                           });
        __syncthreads();
        for (int k = 0; k < m; ++k) {                              // G K = F, LU with partial pivoting; every thread finds the pivot
            double best = -1.0;
            int p = k;
            for (int i = k; i < m; ++i) {
                const double v = fabs(G[k * m + i]);
                if (pivot_beats(v, best)) { best = v; p = i; }
            }
            __syncthreads();
            if (p != k && tid >= k && tid < m + n) {
                double* col = tid < m ? G + tid * m : F + (tid - m) * m;
                const double v = col[k]; col[k] = col[p]; col[p] = v;
            }
            __syncthreads();
            const double pv = G[k * m + k];
            if (bad_pivot(pv)) {
                if (tid == 0) a.status[prob] = t + 1;
                return;
            }
            const double rp = 1.0 / pv;
            for (int i = k + 1 + ty; i < m; i += GAINS_THREADS / 64) {
                const double l = G[k * m + i] * rp;
                for (int j = k + 1 + tx; j < m + n; j += 64) {
                    double* col = j < m ? G + j * m : F + (j - m) * m;
                    col[i] -= l * col[k];
                }
            }
            __syncthreads();
        }
        if (tid < n) {                                             // U K = F, a column per thread
            double* col = F + tid * m;
            for (int k = m - 1; k >= 0; --k) {
                double s = col[k];
                for (int j = k + 1; j < m; ++j) s -= G[j * m + k] * col[j];
                s /= G[k * m + k];
                col[k] = s;
                KT[k * n + tid] = s;
                finite = finite && isfinite(s);
            }
        }
        __syncthreads();
        tile_product<2, 3>(n, n, m, [&](int r, int k) { return Bm[k * n + r]; }, [&](int k, int c) { return F[c * m + k]; },
                           [&](int r, int c, double v) { const double d = Ac[c * n + r] - v; Ac[c * n + r] = d; AcT[r * n + c] = d; });      // A - B K
        tile_product<2, 3>(m, n, m, [&](int r, int k) { return Rm[k * m + r]; }, [&](int k, int c) { return F[c * m + k]; },
                           [&](int r, int c, double v) { RK[c * m + r] = v; });                                   // R K
        if (t < a.n_keep) for (int e = tid; e < m * n; e += GAINS_THREADS) Kg[(size_t)t * m * n + e] = F[e];
        __syncthreads();
        tile_product<2, 3>(n, n, n, [&](int r, int k) { return P[k * n + r]; }, [&](int k, int c) { return Ac[c * n + k]; },
                           [&](int r, int c, double v) { T1[c * n + r] = v; });                                   // P (A - B K)
        __syncthreads();
        // P <- Q + K'RK + (A - B K)' P (A - B K), not symmetrized (gains.jl:10-11): the two products as one sum over m + n terms would
        // change the order of the additions, so they stay two sums
        tile_product<2, 3>(n, n, m, [&](int r, int k) { return KT[k * n + r]; }, [&](int k, int c) { return RK[c * m + k]; },
                           [&](int r, int c, double v) { P[c * n + r] = Qt[c * n + r] + v; });
        tile_product<2, 3>(n, n, n, [&](int r, int k) { return AcT[k * n + r]; }, [&](int k, int c) { return T1[c * n + k]; },
                           [&](int r, int c, double v) { const double s = P[c * n + r] + v; P[c * n + r] = s; finite = finite && isfinite(s); });
        // A_t enters F = B'PA and A - B K, Q_t enters P alone: neither meets a pivot test at this step, and at the last step walked
        // (t = 0) none follows.  A non-finite K_t or P counts as singular here, on the values the threads hold.
        if (__syncthreads_or(!finite)) {
            if (tid == 0) a.status[prob] = t + 1;
            return;
        }
    }
    if (a.P1) for (int e = tid; e < n * n; e += GAINS_THREADS) a.P1[(size_t)prob * n * n + e] = P[e];
    if (tid == 0) a.status[prob] = 0;
}

// ---- the policy's two kernels ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gain_latch_kernel(int H, int nq, int nu, const int* window, const double* traj_u, const double* ref_q,
                                                        const double* K, double* latch) {
    const int b = blockIdx.x, tid = threadIdx.x, nk = nu * 2 * nq;
    double* L = latch + (size_t)b * (nu + nk + 2 * nq);
    const double* Kt = K + (size_t)window[(size_t)b * (H + 2)] * nk;          // K[window[1]]
    for (int e = tid; e < nu; e += 64) L[e] = traj_u[(size_t)b * H * nu + e];
    for (int e = tid; e < nk; e += 64) L[nu + e] = Kt[e];
    for (int e = tid; e < 2 * nq; e += 64) L[nu + nk + e] = ref_q[(size_t)b * (H + 2) * nq + e];      // [q_ref[1]; q_ref[2]]
}

__global__ __launch_bounds__(64) void gain_feedback_kernel(int nq, int nu, const double* latch, const double* q_prev, const double* q_cur,
                                                           double n_sample, double* u) {
    const int b = blockIdx.x, nk = nu * 2 * nq;
    const double* L = latch + (size_t)b * (nu + nk + 2 * nq);
    const double* Kt = L + nu;
    const double* target = Kt + nk;
    const double* qp = q_prev + (size_t)b * nq;
    const double* qc = q_cur + (size_t)b * nq;
    for (int i = threadIdx.x; i < nu; i += 64) {
        double s = L[i];
        for (int j = 0; j < 2 * nq; ++j) {
            const double x = j < nq ? qc[j] - n_sample * (qc[j] - qp[j]) : qc[j - nq];      // [q0; q1], q0 = q1 - n_sample (q1 - q_prev)
            s += Kt[j * nu + i] * (target[j] - x);
        }
        u[(size_t)b * nu + i] = s / n_sample;
    }
}

size_t dynamics_lds(int nq, int nz) { return ((size_t)nz * nz + (size_t)nz * nq + nz + 2) * sizeof(double); }
size_t tvlqr_lds(int n, int m) { return (4 * (size_t)n * n + 6 * (size_t)n * m + 2 * (size_t)m * m) * sizeof(double); }

bool dynamics_launch(int nq, int nu, int nz, int H, const double* d_rz, const double* d_rth, size_t rth_stride, double* d_A, double* d_B,
                     int* d_status, hipStream_t st) {
    const size_t lds = dynamics_lds(nq, nz);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(gains_dynamics_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(gains_dynamics_kernel, dim3(H), dim3(GAINS_THREADS), lds, st, nq, nu, nz, d_rz, d_rth, rth_stride, d_A, d_B, d_status);
    return hipGetLastError() == hipSuccess;
}

bool tvlqr_launch(int n_prob, const TvlqrArgs& a, hipStream_t st) {
    const size_t lds = tvlqr_lds(a.n, a.m);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(tvlqr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(tvlqr_kernel, dim3(n_prob), dim3(GAINS_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess;
}

int gains_fail(int code, const std::string& msg) {
    set_global_error(msg);
    return code;
}

// grow-only device buffer of the stateless entries, one per device, next to the plant workspace whose stream and mutex they use
struct GainsWs { double* d = nullptr; size_t cap = 0; };
GainsWs g_gains_ws[PLANT_MAX_DEVICES];

bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

// The sizes of a reference_gains call; model >= 0: the entry that linearizes on the device.  reference_gains_run, which the two
// entries share, takes them with `in`: what goes to the device behind Q and R - rz0 | the leading columns of rth0, or z | theta | terrains,
// from which plant_linearize_kernel then fills rz0, rth0 on the device.
struct GainsJob {
    int nq, nu, nz, nth, H, N;
    int model = -1, n_terrain = 0, n_ter_up = 0;      // the device-linearized entry
};

int reference_gains_run(const GainsJob& J, const std::vector<double>& in, const double* Qq, const double* Qv, const double* Ru,
                        double U_scaling, double V_scaling, double* K, double* P1) {
    const int nq = J.nq, nu = J.nu, nz = J.nz, nth = J.nth, H = J.H, n = 2 * nq, m = nu, ncol = 2 * nq + nu;
    const size_t n_QR = (size_t)n * n + (size_t)m * m, n_in = in.size();
    const size_t n_rz = (size_t)H * nz * nz, n_rth_full = (size_t)H * nz * nth;
    const size_t n_A = (size_t)H * n * n, n_B = (size_t)H * n * m, n_K = (size_t)H * m * n, n_P = (size_t)n * n;
    // device layout: Q | R | in | (rz0 | rth0 of the device linearization) | A | B | K | P1 | status (dynamics, Riccati)
    const size_t o_in = n_QR, o_lin = o_in + n_in, o_A = o_lin + (J.model >= 0 ? n_rz + n_rth_full : 0), o_B = o_A + n_A, o_K = o_B + n_B,
                 o_P = o_K + n_K, o_st = o_P + n_P, total = o_st + 1;
    std::vector<double> up(n_QR + n_in), out(n_K + n_P + 1);
    for (int j = 0; j < n; ++j)          // gains.jl:43-46
        for (int i = 0; i < n; ++i) {
            const size_t e = (size_t)(j % nq) * nq + (i % nq);
            up[(size_t)j * n + i] = (i / nq == j / nq) ? Qq[e] + V_scaling * Qv[e] : -V_scaling * Qv[e];
        }
    for (int e = 0; e < m * m; ++e) up[(size_t)n * n + e] = U_scaling * Ru[e];      // gains.jl:47
    std::memcpy(up.data() + o_in, in.data(), n_in * sizeof(double));
    int dev = 0;
    if (!plant_current_device(&dev)) return gains_fail(CIMPC_ERR_NO_DEVICE, "no gfx950 device is current");
    std::lock_guard<std::mutex> lock(g_plant_mu);
    PlantWs* ws = plant_ws_open(dev);
    GainsWs& G = g_gains_ws[dev];
    if (!ws || !plant_grow(&G.d, &G.cap, total)) return gains_fail(CIMPC_ERR_HIP, "the gains workspace could not be allocated");
    hipStream_t st = ws->st;
    double* D = G.d;
    int* d_status = reinterpret_cast<int*>(D + o_st);
    bool ok = hipMemcpyAsync(D, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemsetAsync(d_status, 0x7f, 2 * sizeof(int), st) == hipSuccess;
    const double *d_rz = D + o_in, *d_rth = D + o_in + n_rz;
    size_t rth_stride = (size_t)nz * ncol;                       // the host packed the columns that are read
    if (J.model >= 0) {
        const size_t n_z = (size_t)H * nz, n_th = (size_t)H * nth;
        const cimpc_terrain* d_ter = J.n_ter_up ? reinterpret_cast<const cimpc_terrain*>(D + o_in + n_z + n_th) : nullptr;
        d_rz = D + o_lin; d_rth = D + o_lin + n_rz; rth_stride = (size_t)nz * nth;
        ok = ok && plant_linearize_launch(J.model, H, D + o_in, D + o_in + n_z, d_ter, J.n_terrain, 0.0, nullptr, D + o_lin, D + o_lin + n_rz, st);
    }
    ok = ok && dynamics_launch(nq, nu, nz, H, d_rz, d_rth, rth_stride, D + o_A, D + o_B, d_status, st);
    TvlqrArgs a{n, m, J.N * H + 1, H, 1, 1, H, D + o_A, D + o_B, D, D + (size_t)n * n, D + o_K, D + o_P, d_status + 1, d_status};
    ok = ok && tvlqr_launch(1, a, st);
    ok = ok && hipMemcpyAsync(out.data(), D + o_K, out.size() * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = (hipStreamSynchronize(st) == hipSuccess) && ok;
    if (!ok) return gains_fail(CIMPC_ERR_HIP, std::string("reference_gains: ") + hipGetErrorString(hipGetLastError()));
    int status[2];
    std::memcpy(status, out.data() + n_K + n_P, sizeof(status));
    if (status[0] != GAINS_NO_KNOT)
        return gains_fail(CIMPC_ERR_SINGULAR, "rz is singular (a zero or non-finite pivot, or a non-finite dz/dtheta) at knot " + std::to_string(status[0] + 1) +
                                              " (1-based); K is untouched");
    if (status[1] != 0)
        return gains_fail(CIMPC_ERR_SINGULAR, "R + B'PB is singular (a zero or non-finite pivot, or a non-finite K or P) at Riccati step " + std::to_string(status[1]) +
                                              " (1-based) of " + std::to_string(J.N * H) + "; K is untouched");
    std::memcpy(K, out.data(), n_K * sizeof(double));
    if (P1) std::memcpy(P1, out.data() + n_K, n_P * sizeof(double));
    return CIMPC_OK;
}

// Which of plant_linearize_check's conditions a refused call missed, in its order (it returns a code alone)
std::string linearize_refusal(int model, int H, int n_terrain, const cimpc_terrain* terrain, const double* z, const double* theta) {
    if (H < 1) return "H < 1";
    if (!z || !theta) return "null z or theta";
    if ((n_terrain != 0) != (terrain != nullptr)) return "n_terrain and terrain do not go together (0 and NULL, or a count and a list)";
    PlantModel M{};
    bool rough = false;
    if (!plant_model_by_id(model, &M)) return "unknown plant model " + std::to_string(model);
    if (!plant_model_and_ground(model, H, n_terrain, terrain, &M, &rough))
        return terrain ? "the terrain count is neither 1 nor H, or a terrain is not one the model takes" : "the model needs a terrain";
    return "a knot's h (the last entry of its theta) is not positive";
}

// the checks the two reference_gains entries share; nz and nth are the caller's or the model's
int reference_gains_validate(int nq, int nu, int nz, int nth, int H, int N, const double* Qq, const double* Qv, const double* Ru, double U_scaling,
                             double V_scaling, const double* K) {
    if (!Qq || !Qv || !Ru || !K) return gains_fail(CIMPC_ERR_INVALID, "null argument");
    if (nq < 1 || nu < 1 || nz < 1 || nth < 1 || H < 1 || N < 1) return gains_fail(CIMPC_ERR_INVALID, "sizes and N must be at least 1");
    if (!positive_finite(U_scaling) || !positive_finite(V_scaling)) return gains_fail(CIMPC_ERR_INVALID, "the scalings must be finite and positive");
    if (nz < nq || nth < 2 * nq + nu) return gains_fail(CIMPC_ERR_INVALID, "nz < nq or ntheta < 2 nq + nu");
    if (2 * nq > GAINS_MAX_N || nu > GAINS_MAX_M) return gains_fail(CIMPC_ERR_INVALID, "2 nq <= 48 and nu <= 16 are supported");
    if (dynamics_lds(nq, nz) > GAINS_MAX_LDS) return gains_fail(CIMPC_ERR_INVALID, "rz and its right-hand sides do not fit the LDS of a CU");
    if ((long long)N * H + 1 > INT_MAX / 2) return gains_fail(CIMPC_ERR_INVALID, "N H is too large");
    return CIMPC_OK;
}

}  // namespace

bool gain_latch_launch(int B, int H, int nq, int nu, const int* window, const double* traj_u, const double* ref_q, const double* K,
                       double* latch, hipStream_t st) {
    hipLaunchKernelGGL(gain_latch_kernel, dim3(B), dim3(64), 0, st, H, nq, nu, window, traj_u, ref_q, K, latch);
    return hipGetLastError() == hipSuccess;
}

bool gain_feedback_launch(int B, int nq, int nu, const double* latch, const double* q_prev, const double* q_cur, double n_sample, double* u,
                          hipStream_t st) {
    hipLaunchKernelGGL(gain_feedback_kernel, dim3(B), dim3(64), 0, st, nq, nu, latch, q_prev, q_cur, n_sample, u);
    return hipGetLastError() == hipSuccess;
}

}  // namespace cimpc

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
// Each entry validates first (no device needed), then runs on the calling thread's current device on the plant workspace's private
// stream: one upload, the kernels, one read-back, one synchronize.  The outputs are written only when every step went through.
extern "C" int cimpc_tvlqr(int n_prob, int n, int m, int T, int n_ab, const double* A, const double* B, int n_q, const double* Q, int n_r,
                           const double* R, int n_keep, double* K, double* P1) {
    using namespace cimpc;
    if (!A || !B || !Q || !R || !K) return gains_fail(CIMPC_ERR_INVALID, "null argument");
    if (n_prob < 1 || n < 1 || m < 1 || T < 2 || n_ab < 1) return gains_fail(CIMPC_ERR_INVALID, "n_prob, n, m, n_ab >= 1 and T >= 2 are required");
    if (n > GAINS_MAX_N || m > GAINS_MAX_M) return gains_fail(CIMPC_ERR_INVALID, "n <= 48 and m <= 16 are supported");
    if ((n_q != 1 && n_q != T) || (n_r != 1 && n_r != T - 1)) return gains_fail(CIMPC_ERR_INVALID, "n_q must be 1 or T, n_r 1 or T - 1");
    if (n_keep < 1 || n_keep > T - 1) return gains_fail(CIMPC_ERR_INVALID, "n_keep must be in 1 .. T - 1");
    const size_t P = n_prob, nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    const size_t n_A = P * n_ab * nn, n_B = P * n_ab * nm, n_Q = P * n_q * nn, n_R = P * n_r * mm, n_K = P * n_keep * nm, n_P = P * nn;
    const size_t o_B = n_A, o_Q = o_B + n_B, o_R = o_Q + n_Q, o_K = o_R + n_R, o_P = o_K + n_K, o_st = o_P + n_P, total = o_st + (P + 1) / 2;
    std::vector<double> up(o_K), out(total - o_K);
    std::memcpy(up.data(), A, n_A * sizeof(double));
    std::memcpy(up.data() + o_B, B, n_B * sizeof(double));
    std::memcpy(up.data() + o_Q, Q, n_Q * sizeof(double));
    std::memcpy(up.data() + o_R, R, n_R * sizeof(double));
    int dev = 0;
    if (!plant_current_device(&dev)) return gains_fail(CIMPC_ERR_NO_DEVICE, "no gfx950 device is current");
    std::lock_guard<std::mutex> lock(g_plant_mu);
    PlantWs* ws = plant_ws_open(dev);
    GainsWs& G = g_gains_ws[dev];
    if (!ws || !plant_grow(&G.d, &G.cap, total)) return gains_fail(CIMPC_ERR_HIP, "the gains workspace could not be allocated");
    hipStream_t st = ws->st;
    double* D = G.d;
    int* d_status = reinterpret_cast<int*>(D + o_st);
    bool ok = hipMemcpyAsync(D, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemsetAsync(d_status, 0x7f, P * sizeof(int), st) == hipSuccess;
    TvlqrArgs a{n, m, T, n_ab, n_q, n_r, n_keep, D, D + o_B, D + o_Q, D + o_R, D + o_K, D + o_P, d_status, nullptr};
    ok = ok && tvlqr_launch(n_prob, a, st);
    ok = ok && hipMemcpyAsync(out.data(), D + o_K, out.size() * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = (hipStreamSynchronize(st) == hipSuccess) && ok;
    if (!ok) return gains_fail(CIMPC_ERR_HIP, std::string("cimpc_tvlqr: ") + hipGetErrorString(hipGetLastError()));
    const int* status = reinterpret_cast<const int*>(out.data() + n_K + n_P);
    for (int p = 0; p < n_prob; ++p)
        if (status[p] != 0)
            return gains_fail(CIMPC_ERR_SINGULAR, "R + B'PB is singular (a zero or non-finite pivot, or a non-finite K or P) at Riccati step " + std::to_string(status[p]) +
                                                  " (1-based) of " + std::to_string(T - 1) + ", problem " + std::to_string(p) + "; K is untouched");
    std::memcpy(K, out.data(), n_K * sizeof(double));
    if (P1) std::memcpy(P1, out.data() + n_K, n_P * sizeof(double));
    return CIMPC_OK;
}

extern "C" int cimpc_reference_gains_lin(int nq, int nu, int nz, int nth, int H, int N, const double* rz0, const double* rth0, const double* Qq,
                                         const double* Qv, const double* Ru, double U_scaling, double V_scaling, double* K, double* P1) {
    using namespace cimpc;
    if (!rz0 || !rth0) return gains_fail(CIMPC_ERR_INVALID, "null argument");
    if (int rc = reference_gains_validate(nq, nu, nz, nth, H, N, Qq, Qv, Ru, U_scaling, V_scaling, K); rc != CIMPC_OK) return rc;
    const size_t n_rz = (size_t)H * nz * nz, per = (size_t)nz * (2 * nq + nu);
    std::vector<double> in(n_rz + (size_t)H * per);
    std::memcpy(in.data(), rz0, n_rz * sizeof(double));
    for (int t = 0; t < H; ++t)          // the q0, q1, u1 columns of rtheta: the leading ones, contiguous in a column-major knot
        std::memcpy(in.data() + n_rz + (size_t)t * per, rth0 + (size_t)t * nz * nth, per * sizeof(double));
    return reference_gains_run(GainsJob{nq, nu, nz, nth, H, N}, in, Qq, Qv, Ru, U_scaling, V_scaling, K, P1);
}

extern "C" int cimpc_reference_gains(int model, int H, int N, int n_terrain, const cimpc_terrain* terrain, const double* z, const double* theta,
                                     const double* Qq, const double* Qv, const double* Ru, double U_scaling, double V_scaling, double* K,
                                     double* P1) {
    using namespace cimpc;
    PlantLinearizeDims pd{};
    if (plant_linearize_check(model, H, n_terrain, terrain, z, theta, 0.0, &pd) != CIMPC_OK)
        return gains_fail(CIMPC_ERR_INVALID, "cimpc_plant_linearize would refuse these arguments: " + linearize_refusal(model, H, n_terrain, terrain, z, theta));
    const int nz = pd.nq + 4 * pd.nc + 2 * pd.nb, nth = 2 * pd.nq + pd.nu + pd.nw + 2;
    if (int rc = reference_gains_validate(pd.nq, pd.nu, nz, nth, H, N, Qq, Qv, Ru, U_scaling, V_scaling, K); rc != CIMPC_OK) return rc;
    constexpr size_t TW = sizeof(cimpc_terrain) / sizeof(double);
    const size_t n_z = (size_t)H * nz, n_th = (size_t)H * nth, n_ter = (size_t)pd.n_terrain_up * TW;
    std::vector<double> in(n_z + n_th + n_ter);
    std::memcpy(in.data(), z, n_z * sizeof(double));
    std::memcpy(in.data() + n_z, theta, n_th * sizeof(double));
    if (n_ter) std::memcpy(in.data() + n_z + n_th, terrain, n_ter * sizeof(double));
    GainsJob J{pd.nq, pd.nu, nz, nth, H, N};
    J.model = model; J.n_terrain = n_terrain; J.n_ter_up = pd.n_terrain_up;
    return reference_gains_run(J, in, Qq, Qv, Ru, U_scaling, V_scaling, K, P1);
}
