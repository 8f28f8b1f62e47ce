// Host harness for plant_model_by_id of contactimplicitmpc/jl_amd/csrc/plant_model.h: for every id given on the command line
// prints "id found nq nu nc nb nw" (the dimensions 0 where the id has no model).
#include <cstdio>
#include <cstdlib>
#include "../../contactimplicitmpc/jl_amd/csrc/plant_model.h"
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const int id = atoi(argv[a]);
        cimpc::PlantModel M{};
        if (cimpc::plant_model_by_id(id, &M)) printf("%d 1 %d %d %d %d %d\n", id, M.nq, M.nu, M.nc, M.nb(), M.nw);
        else printf("%d 0 0 0 0 0 0\n", id);
    }
    return 0;
}
