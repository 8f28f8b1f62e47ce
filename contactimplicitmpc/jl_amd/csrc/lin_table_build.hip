// The packed linearization tables built on the device (A1 for N knots at once): lin_table_build_knot of lin_table_build.h, the
// text cimpc_set_linearization runs on the host, here by one workgroup per knot.  [Dx | I], CAi and CAiB live in dynamic LDS sized from
// the handle's run-time (nx, ny): 30 KB for the largest compiled model (centroidal_quadruped_wall, nx 18, ny 48), 129 KB at the
// generic kernel's bound nx = ny = 64 - above 64 KB the kernel's limit is raised for that launch shape alone.  rz0 (104 KB for the
// wall) is read from global memory where it is used, never staged whole.  Runs when tables are built, not per MPC step.
#include <hip/hip_runtime.h>

// every operation rounds as it does in the host's run of the same header; the multiply-adds that are fused are spelled std::fma there
#pragma clang fp contract(off)

#include "lin_table_build.h"

namespace cimpc {

namespace {

constexpr int LTB_THREADS = 256;
constexpr size_t LTB_LDS_DEFAULT = 64 * 1024, LTB_LDS_CU = 160 * 1024;

struct WorkgroupTeam {
    __device__ int rank() const { return (int)threadIdx.x; }
    __device__ int size() const { return (int)blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(LTB_THREADS) void lin_table_build_kernel(LinLayout L, int N, const double* z0, const double* th0,
                                                                      const double* r0, const double* rz0, const double* rth0,
                                                                      double* tables, int* status) {
    extern __shared__ double ltb_work[];
    const int k = blockIdx.x;
    if (k >= N) return;                                              // uniform over the workgroup
    const size_t nz = (size_t)L.nx + 2 * (size_t)L.ny, nth = (size_t)L.nth;
    const bool ok = lin_table_build_knot(L, z0 + k * nz, th0 + k * nth, r0 + k * nz, rz0 + k * nz * nz, rth0 + k * nz * nth, ltb_work,
                                         tables + (size_t)k * L.size, WorkgroupTeam{});
    if (threadIdx.x == 0) status[k] = ok ? 0 : 1;
}

}  // namespace

bool lin_table_build_launch(const LinLayout& L, int N, const double* z0, const double* th0, const double* r0, const double* rz0,
                            const double* rth0, double* tables, int* status, hipStream_t st) {
    const size_t lds = lin_table_work_doubles(L.nx, L.ny) * sizeof(double);
    if (N < 1 || lds > LTB_LDS_CU) return false;
    if (lds > LTB_LDS_DEFAULT &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(lin_table_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(lin_table_build_kernel, dim3(N), dim3(LTB_THREADS), lds, st, L, N, z0, th0, r0, rz0, rth0, tables, status);
    return hipGetLastError() == hipSuccess;
}

}  // namespace cimpc
