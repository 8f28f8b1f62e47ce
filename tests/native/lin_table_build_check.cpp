// lin_table_build_knot (contactimplicitmpc/jl_amd/csrc/lin_table_build.h), the text the device kernel and the library's host path
// run, on the host with its team of one.  stdin: nx ny nth G nths adj, then z0 (nz), th0 (nth), r0 (nz), rz0 (nz x nz, column-major), rth0 (nz x nth,
// column-major).  stdout: the LinLayout (one line: ldw gst oW oCAi oAi oDy1 oDx oRx oRy1 oRthDyn oRthRst oGs oK0 oAiB oVec oTh0
// size), then "singular" or the table, one %a per entry.
//   g++ -O2 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] lin_table_build_check.cpp
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#include "../../contactimplicitmpc/jl_amd/csrc/lin_table_build.h"

static bool read(std::vector<double>& v) {
    for (double& x : v)
        if (std::scanf("%lf", &x) != 1) return false;
    return true;
}

int main() {
    int nx, ny, nth, G, nths, adj;
    if (std::scanf("%d %d %d %d %d %d", &nx, &ny, &nth, &G, &nths, &adj) != 6 || nx < 1 || ny < 1 || nth < 1 || nx > G || ny > G || nths < 0 ||
        nths > nth) {
        std::puts("invalid");
        return 0;
    }
    const cimpc::LinLayout L(nx, ny, nth, G, nths, adj);
    const size_t nz = (size_t)nx + 2 * (size_t)ny;
    std::vector<double> z0(nz), th0(nth), r0(nz), rz0(nz * nz), rth0(nz * nth);
    if (!read(z0) || !read(th0) || !read(r0) || !read(rz0) || !read(rth0)) {
        std::puts("invalid");
        return 0;
    }
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", L.ldw, L.gst, L.oW, L.oCAi, L.oAi, L.oDy1, L.oDx, L.oRx, L.oRy1, L.oRthDyn,
                L.oRthRst, L.oGs, L.oK0, L.oAiB, L.oVec, L.oTh0, L.size);
    std::vector<double> work(cimpc::lin_table_work_doubles(nx, ny)), T(L.size, -1.0);      // -1: the build itself must write the padding
    if (!cimpc::lin_table_build_knot(L, z0.data(), th0.data(), r0.data(), rz0.data(), rth0.data(), work.data(), T.data(), cimpc::SoloTeam{})) {
        std::puts("singular");
        return 0;
    }
    for (double v : T) std::printf("%a\n", v);
    return 0;
}
