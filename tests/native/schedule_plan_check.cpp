// Host-only driver of contactimplicitmpc/jl_amd/csrc/schedule_plan.h (tests/test_schedule_plan.py): one case per input line,
//   policy: async_mode async_tail async_full_max spec_first iter_cap tail_div drain_pct drain_min sweep_wgs waves32
//   facts:  B H H_ref G async_available
//   solve:  backend (KktBackend) warm_start budget newton_max_iter ip_max_iter
//   round:  kkt blind last_sweep last_slots active
//   sweep:  hint launch_cap (0: the policy's iter_cap) drain
// and one output line of name=value pairs per case.
#include "../../contactimplicitmpc/jl_amd/csrc/schedule_plan.h"

#include <cstdio>
#include <iostream>

using namespace cimpc;

int main() {
    static const char* paths[] = {"Rounds", "Persistent", "Hybrid"};
    while (true) {
        SchedulePolicy p;
        ScheduleFacts f;
        int avail, be, warm, budget, newton_max_iter, ip_max_iter, kkt, blind, last_sweep, last_slots, active, launch_cap, drain;
        long long hint;
        if (!(std::cin >> p.async_mode)) return 0;
        std::cin >> p.async_tail >> p.async_full_max >> p.spec_first >> p.iter_cap >> p.tail_div >> p.drain_pct >> p.drain_min >> p.sweep_wgs
            >> p.waves32 >> f.B >> f.H >> f.H_ref >> f.G >> avail >> be >> warm >> budget >> newton_max_iter >> ip_max_iter
            >> kkt >> blind >> last_sweep >> last_slots >> active >> hint >> launch_cap >> drain;
        if (!std::cin) return 1;
        f.async_available = avail != 0;
        const SchedulePlan s = plan_schedule(p, f);
        const KktBackend backend = (KktBackend)be;
        const RoundPlan r = plan_round(p, s, ip_max_iter, kkt != 0, blind != 0, last_sweep, last_slots);
        const int cap = launch_cap > 0 ? launch_cap : p.iter_cap;
        const SweepLaunch l = plan_sweep(p, s, hint, cap, ip_max_iter, drain != 0);
        std::printf("async_on=%d path=%s async_tail=%d waves=%d adapt32=%lld wpk=%d async_grid=%d async_service=%d tail_grid=%d tail_service=%d "
                    "spec_all=%d spec_first=%d spec_mid=%d spec_tail=%d kkt_overlap=%d max_rounds=%d ahead=%d cap=%d n_slots=%d split_join=%d "
                    "hand_over=%d sweep_waves=%d sweep_wpk=%d direct=%d drain_thresh=%d\n",
                    s.async_on, paths[(int)choose_solve_path(s, backend)], s.async_tail, s.waves, s.adapt32, s.wpk, s.async_grid,
                    s.async_service, s.tail_grid, s.tail_service, s.spec_all, s.spec_first, s.spec_mid, s.spec_tail, s.kkt_overlap,
                    max_rounds(p, newton_max_iter, ip_max_iter), round_ahead(s, backend, warm != 0, budget != 0), r.cap, r.n_slots,
                    r.split_join, hand_over(s, active), l.waves, l.wpk, l.direct, l.drain_thresh);
    }
}
