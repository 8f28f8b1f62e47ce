// Host-only driver of contactimplicitmpc/jl_amd/csrc/model_table.h (tests/test_model_table.py).  First the table,
//   row <name> <nq> <nu> <nw> <nc> <nb> <lanes> <async>          one line per row, in table order
//   pair <nq> <nu>                                               every (nq, nu) in [0, 40)^2 that model_has_nqnu accepts
// then, for each input line "nq nu nw nc nb mode H", one line "<sweep> <callback> <async>": the row's name, or none.
#include "../../contactimplicitmpc/jl_amd/csrc/model_table.h"

#include <cstdio>
#include <iostream>

using namespace cimpc;

static const char* name_of(int id) { return id < MODEL_COUNT ? MODEL_TABLE[id].name : "none"; }

int main() {
    for (const ModelRow& r : MODEL_TABLE)
        std::printf("row %s %d %d %d %d %d %d %d\n", r.name, r.nq, r.nu, r.nw, r.nc, r.nb, model_lanes(r), r.async ? 1 : 0);
    for (int q = 0; q < 40; ++q)
        for (int u = 0; u < 40; ++u)
            if (model_has_nqnu(q, u)) std::printf("pair %d %d\n", q, u);
    cimpc_dims d{};
    while (std::cin >> d.nq >> d.nu >> d.nw >> d.nc >> d.nb >> d.mode >> d.H)
        std::printf("%s %s %s\n", name_of(model_sweep(&d)), name_of(model_callback(&d)), name_of(model_async(&d)));
    return 0;
}
