// Host harness for plant_instance / plant_visit_instance of contactimplicitmpc/jl_amd/csrc/plant_ground.h: for every id given on the
// command line, flat and on terrain, for the step kernel and for the linearization / sensitivity, prints
//   "id found on_terrain for_step nz nth NZ NTH GROUND visited"
// - the model's sizes, the instance plant_instance chooses and whether plant_visit_instance handed exactly that instance to its
// visitor.  An id without a model prints "id 0".
#include <cstdio>
#include <cstdlib>
#include "../../contactimplicitmpc/jl_amd/csrc/plant_ground.h"
int main(int argc, char** argv) {
    using namespace cimpc;
    for (int a = 1; a < argc; ++a) {
        const int id = atoi(argv[a]);
        PlantModel M{};
        if (!plant_model_by_id(id, &M)) { printf("%d 0\n", id); continue; }
        for (int on_terrain = 0; on_terrain < 2; ++on_terrain)
            for (int for_step = 0; for_step < 2; ++for_step) {
                const PlantInstance I = plant_instance(M, on_terrain, for_step);
                const bool visited = plant_visit_instance(M, on_terrain, for_step, [&](auto tag) {
                    return tag.NZ == I.NZ && tag.NTH == I.NTH && tag.GROUND == I.GROUND;
                });
                printf("%d 1 %d %d %d %d %d %d %d %d\n", id, on_terrain, for_step, M.nz(), M.nth(), I.NZ, I.NTH, I.GROUND, (int)visited);
            }
    }
    return 0;
}
