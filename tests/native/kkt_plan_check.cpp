// Host-only driver of contactimplicitmpc/jl_amd/csrc/kkt_plan.h (tests/test_kkt_plan.py): one case per input line,
//   caps:   cfg velocity cf_tiny wide_tiles condensed mfma packed twisted duo mixed banded cf_reduce banded_twisted
//   want:   kkt_backend (cimpc_newton_opts)
//   policy: kkt_pipe kkt_twisted kkt_duo kkt_duo_hint kkt_duo_max kkt_tw_max kkt_pipe_max async_kkt_tw lazy_dz kkt_overlap (knob, -1: the handle's, schedule_plan.h)
//   site:   kind (1 / 2: a lock-step round, on whichever stream kkt_overlap gives) attempt n_kkt blind sweep_problems tw_off B async_tail waves
// and one output line per case: backend form two_ended lazy_commit.
#include "../../contactimplicitmpc/jl_amd/csrc/kkt_plan.h"
#include "../../contactimplicitmpc/jl_amd/csrc/schedule_plan.h"

#include <cstdio>
#include <iostream>

using namespace cimpc;

int main() {
    static const char* backends[] = {"Condensed", "CondensedMixed", "Banded", "DenseLu", "CfCondensed", "CfBanded"};
    static const char* forms[] = {"PerRollout", "Scalar", "Packed", "Pipelined", "Twisted", "Duo", "BandedOneEnded", "BandedTwisted",
                                  "Dense", "AsyncOneEnded", "AsyncTwoJob"};
    int v[13];
    while (true) {
        for (int& x : v) if (!(std::cin >> x)) return 0;
        KktCaps c;
        c.cfg = v[0]; c.velocity = v[1]; c.cf_tiny = v[2]; c.wide_tiles = v[3]; c.condensed = v[4]; c.mfma = v[5]; c.packed = v[6];
        c.twisted = v[7]; c.duo = v[8]; c.mixed = v[9]; c.banded = v[10]; c.cf_reduce = v[11]; c.banded_twisted = v[12];
        int want, lazy, overlap, kind, blind, tw_off;
        KktPolicy p;
        KktSite s;
        std::cin >> want >> p.kkt_pipe >> p.kkt_twisted >> p.kkt_duo >> p.kkt_duo_hint >> p.kkt_duo_max >> p.kkt_tw_max >> p.kkt_pipe_max
            >> p.async_kkt_tw >> lazy >> overlap >> kind >> s.attempt >> s.n_kkt >> blind >> s.sweep_problems >> tw_off >> s.B >> s.async_tail >> s.waves;
        if (!std::cin) return 1;
        p.lazy_dz = lazy != 0;
        ScheduleFacts facts;
        facts.B = s.B;
        p.kkt_overlap = overlap >= 0 ? overlap != 0 : plan_schedule(SchedulePolicy{}, facts).kkt_overlap;
        s.kind = (KktSite::Kind)kind;
        if (kind == KktSite::Round || kind == KktSite::Overlapped) s.kind = p.kkt_overlap ? KktSite::Overlapped : KktSite::Round;   // as the host
        s.blind = blind != 0;
        s.tw_off = tw_off != 0;
        const KktBackend be = select_kkt_backend(c, want);
        const KktForm f = choose_kkt_form(p, c, be, s);
        std::printf("%s %s %d %d\n", backends[(int)be], forms[(int)f], two_ended(f) ? 1 : 0, kkt_lazy_commit(p, c, be) ? 1 : 0);
    }
}
