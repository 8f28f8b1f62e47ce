// Host-only driver of contactimplicitmpc/jl_amd/csrc/plant_rollout_plan.h (tests/test_plant_rollout.py): one query per input line,
//   row t hold K                 -> the schedule row of step t
//   chunks T steps_per_launch    -> the count, then t0 n of every launch
// and one output line per query.
#include "../../contactimplicitmpc/jl_amd/csrc/plant_rollout_plan.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

using namespace cimpc;

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "row") {
            int t, hold, K;
            if (!(std::cin >> t >> hold >> K)) return 1;
            std::printf("%d\n", rollout_row(t, hold, K));
        } else if (what == "chunks") {
            int T, spl;
            if (!(std::cin >> T >> spl)) return 1;
            const int n = rollout_chunk_count(T, spl);
            std::vector<RolloutChunk> list;      // on the heap: the sanitizer build sees every element
            for (int k = 0; k < n; ++k) list.push_back(rollout_chunk(T, spl, k));
            std::printf("%d", n);
            for (const RolloutChunk& c : list) std::printf(" %d %d", c.t0, c.n);
            std::printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
