"""`contactimplicitmpc/jl_amd/csrc/schedule_plan.h` - the schedule of a solve: its path, launch shapes, speculation depths and round
rules - is plain C++: built here with g++ (tests/native/schedule_plan_check.cpp) and driven through a table of named cases.  The
expected values are what cimpc_create, run_sweep and cimpc_newton_solve_dev computed before the rules moved into the header."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# driver inputs in their order, with the defaults of a cold quadruped solve
POLICY = dict(async_mode=2, async_tail=-1, async_full_max=32, spec_first=-1, iter_cap=28, tail_div=8, drain_pct=95, drain_min=4, sweep_wgs=0, waves32=0)
FACTS = dict(B=1, H=40, H_ref=60, G=16, async_available=1)
SOLVE = dict(backend=0, warm_start=0, budget=0, newton_max_iter=5, ip_max_iter=100)
ROUND = dict(kkt=1, blind=0, last_sweep=-1, last_slots=-1, active=0)
SWEEP = dict(hint=-1, launch_cap=0, drain=1)
BANDED, MIXED = 2, 1
CENT = dict(G=32, H=60, H_ref=80)
WIDE64 = dict(G=64)                     # a compiled 64-lane model (ny > 32: centroidal_wall)
RUNTIME = dict(G=64, async_available=0)  # runtime-dimension kernel: no persistent kernel


def case(name, expect, **kw):
    return name, expect, kw


QUADRUPED = {      # quadruped H = 40 (H_ref 60), every rule at its default
    1: {'async_on': 1, 'path': 'Rounds', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 40, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -2, 'direct': 1, 'ahead': 0, 'max_rounds': 1092},
    3: {'async_on': 1, 'path': 'Rounds', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 60, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -2, 'direct': 1, 'ahead': 0, 'max_rounds': 1092},
    4: {'async_on': 1, 'path': 'Persistent', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 60, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    32: {'async_on': 1, 'path': 'Persistent', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 60, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    33: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 60, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    63: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 79, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    64: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 80, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 64, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    128: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 160, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 128, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    129: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 162, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 129, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    255: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 63, 'waves': 4, 'adapt32': 0, 'wpk': 319, 'async_grid': 358, 'async_service': 39, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 255, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    256: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 64, 'waves': 4, 'adapt32': 0, 'wpk': 320, 'async_grid': 360, 'async_service': 40, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 256, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    512: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 85, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 512, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    1024: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 96, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 288, 'tail_service': 36, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 1024, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    1025: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 96, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 288, 'tail_service': 36, 'spec_all': 8, 'spec_first': 1, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 1025, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
    2048: {'async_on': 1, 'path': 'Hybrid', 'async_tail': 96, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 288, 'tail_service': 36, 'spec_all': 8, 'spec_first': 1, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 2048, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
}

CASES = [case(f"quadruped_b{B}", e, B=B) for B, e in QUADRUPED.items()] + [
    # 32-lane model, H = 60
    case("centroidal_b8_single_launch", {'async_on': 1, 'path': 'Persistent', 'async_tail': 16, 'waves': 4, 'adapt32': 7000, 'wpk': 80, 'async_grid': 256, 'async_service': 30, 'tail_grid': 256, 'tail_service': 30, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=8, **CENT),
    case("centroidal_b33_hybrid_tail_16", {'async_on': 1, 'path': 'Hybrid', 'async_tail': 16, 'waves': 4, 'adapt32': 7000, 'wpk': 124, 'async_grid': 256, 'async_service': 30, 'tail_grid': 256, 'tail_service': 30, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=33, **CENT),
    case("centroidal_b99_below_6000", {'async_on': 1, 'path': 'Hybrid', 'async_tail': 16, 'waves': 4, 'adapt32': 7000, 'wpk': 256, 'async_grid': 256, 'async_service': 32, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 99, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=99, **CENT),
    case("centroidal_b100_eight_waves", {'async_on': 1, 'path': 'Hybrid', 'async_tail': 16, 'waves': 8, 'adapt32': 7000, 'wpk': 188, 'async_grid': 256, 'async_service': 30, 'tail_grid': 256, 'tail_service': 30, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 100, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=100, **CENT),
    case("centroidal_b64_hint_6999", {'sweep_waves': 4, 'sweep_wpk': 256},
         B=64, hint=6999, **CENT),
    case("centroidal_b64_hint_7000", {'sweep_waves': 8, 'sweep_wpk': 219},
         B=64, hint=7000, **CENT),
    case("centroidal_b64_hint_600", {'sweep_waves': 4, 'sweep_wpk': 80},
         B=64, hint=600, **CENT),
    case("centroidal_b64_hint_unknown", {'sweep_waves': 4, 'sweep_wpk': 240},
         B=64, hint=-1, **CENT),
    case("centroidal_b32_not_overlapped_keeps_build", {'sweep_waves': 4, 'sweep_wpk': 120},
         B=32, hint=8000, async_mode=0, **CENT),
    case("centroidal_b128_hint_20000", {'waves': 8, 'sweep_waves': 8, 'sweep_wpk': 256},
         B=128, hint=20000, **CENT),
    case("centroidal_waves32_4", {'async_on': 1, 'path': 'Hybrid', 'async_tail': 16, 'waves': 4, 'adapt32': 0, 'wpk': 256, 'async_grid': 256, 'async_service': 32, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 128, 'direct': 0, 'ahead': 0, 'max_rounds': 1092, 'sweep_waves': 4, 'sweep_wpk': 256},
         B=128, waves32=4, hint=20000, **CENT),
    case("centroidal_waves32_8", {'async_on': 1, 'path': 'Hybrid', 'async_tail': 16, 'waves': 8, 'adapt32': 0, 'wpk': 120, 'async_grid': 256, 'async_service': 30, 'tail_grid': 256, 'tail_service': 30, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 64, 'direct': 0, 'ahead': 0, 'max_rounds': 1092, 'sweep_waves': 8, 'sweep_wpk': 120},
         B=64, waves32=8, hint=600, **CENT),
    case("centroidal_waves32_threshold", {'adapt32': 3000, 'sweep_waves': 8, 'sweep_wpk': 94},
         B=64, waves32=3000, hint=3000, **CENT),
    case("centroidal_waves32_threshold_below", {'adapt32': 3000, 'sweep_waves': 4, 'sweep_wpk': 188},
         B=64, waves32=3000, hint=2999, **CENT),
    case("centroidal_sweep_wgs_keeps_grid", {'wpk': 100, 'sweep_waves': 4, 'sweep_wpk': 100, 'async_grid': 112, 'async_service': 12},
         B=64, sweep_wgs=100, hint=9000, **CENT),
    # 64-lane and runtime-dimension models
    case("lanes64_b64", {'async_on': 1, 'path': 'Hybrid', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 256, 'async_grid': 256, 'async_service': 32, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 1, 'n_slots': 64, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=64, **WIDE64),
    case("lanes64_b16", {'async_on': 1, 'path': 'Persistent', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 80, 'async_grid': 256, 'async_service': 30, 'tail_grid': 256, 'tail_service': 30, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=16, **WIDE64),
    case("runtime_dims_b16", {'async_on': 0, 'path': 'Rounds', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 80, 'async_grid': 256, 'async_service': 30, 'tail_grid': 256, 'tail_service': 30, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=16, **RUNTIME),
    case("runtime_dims_b512", {'async_on': 0, 'path': 'Rounds', 'async_tail': 85, 'waves': 4, 'adapt32': 0, 'wpk': 256, 'async_grid': 256, 'async_service': 32, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 512, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=512, **RUNTIME),
    # persistent kernel unavailable, other backends
    case("unavailable_b16_rounds", {'async_on': 0, 'path': 'Rounds', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 60, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=16, async_available=0),
    case("unavailable_b512_rounds", {'async_on': 0, 'path': 'Rounds', 'async_tail': 85, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 512, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=512, async_available=0),
    case("banded_b16_rounds", {'path': 'Rounds', 'waves': 4},
         B=16, backend=BANDED),
    case("banded_b512_rounds", {'path': 'Rounds'},
         B=512, backend=BANDED),
    case("banded_32lane_waves_quirk", {'path': 'Rounds', 'waves': 4},
         B=32, backend=BANDED, **dict(CENT, H=200)),
    case("mixed_b1_no_round_ahead", {'ahead': 0},
         B=1, backend=MIXED, warm_start=1),
    # overrides
    case("async_0_b16", {'async_on': 0, 'path': 'Rounds', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 60, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -1, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=16, async_mode=0),
    case("async_0_b512", {'async_on': 0, 'path': 'Rounds', 'async_tail': 85, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 512, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=512, async_mode=0),
    case("async_1_b1", {'async_on': 1, 'path': 'Persistent', 'async_tail': 32, 'waves': 4, 'adapt32': 0, 'wpk': 40, 'async_grid': 270, 'async_service': 30, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 3, 'spec_first': 3, 'spec_mid': 8, 'kkt_overlap': 0, 'n_slots': -2, 'direct': 1, 'ahead': 0, 'max_rounds': 1092},
         B=1, async_mode=1),
    case("async_1_b512", {'async_on': 1, 'path': 'Persistent', 'async_tail': 85, 'waves': 4, 'adapt32': 0, 'wpk': 512, 'async_grid': 512, 'async_service': 64, 'tail_grid': 256, 'tail_service': 32, 'spec_all': 8, 'spec_first': 3, 'spec_mid': 1, 'kkt_overlap': 1, 'n_slots': 512, 'direct': 0, 'ahead': 0, 'max_rounds': 1092},
         B=512, async_mode=1),
    case("async_tail_override", {'async_tail': 200, 'tail_grid': 512, 'tail_service': 64},
         B=512, async_tail=200),
    case("async_tail_override_32lane", {'async_tail': 40},
         B=512, async_tail=40, **CENT),
    case("async_full_max_64", {'path': 'Persistent', 'waves': 4},
         B=64, async_full_max=64),
    case("async_full_max_2_b3_hybrid", {'path': 'Hybrid'},
         B=3, async_full_max=2),
    case("spec_first_override", {'spec_first': 5},
         B=2048, spec_first=5),
    case("sweep_wgs_override", {'wpk': 64, 'async_grid': 72, 'async_service': 8, 'tail_grid': 72, 'tail_service': 8, 'sweep_wpk': 64},
         B=512, sweep_wgs=64),
    case("sweep_wgs_b1_not_direct", {'direct': 0, 'sweep_wpk': 32},
         B=1, sweep_wgs=32),
    case("drain_default", {'drain_thresh': 486, 'max_rounds': 1092},
         B=512),
    case("drain_pct_0", {'drain_thresh': 0, 'max_rounds': 210},
         B=512, drain_pct=0),
    case("drain_uncapped_launch", {'drain_thresh': 0},
         B=512, launch_cap=100),
    case("drain_min_override", {'max_rounds': 2142},
         B=512, drain_min=2),
    case("iter_cap_override", {'cap': 10, 'max_rounds': 1092},
         B=512, iter_cap=10, last_sweep=512),
    case("tail_div_0_never_sparse", {'cap': 28},
         B=512, tail_div=0, last_sweep=1),
    case("tail_div_16", {'cap': 100},
         B=512, tail_div=16, last_sweep=32),
    case("tail_div_16_busy", {'cap': 28},
         B=512, tail_div=16, last_sweep=33),
    # rounds
    case("sighted_sparse_round", {'cap': 100},
         B=512, last_sweep=64),
    case("sighted_busy_round", {'cap': 28},
         B=512, last_sweep=65),
    case("blind_round_busy_cap", {'cap': 28},
         B=512, last_sweep=64, blind=1),
    case("small_batch_never_parks", {'cap': 100},
         B=7, last_sweep=7, blind=1),
    case("b8_parks", {'cap': 28},
         B=8, last_sweep=8),
    case("overlapped_list", {'n_slots': 300, 'split_join': 1},
         B=512, last_slots=300),
    case("overlapped_no_kkt", {'n_slots': 300, 'split_join': 0},
         B=512, last_slots=300, kkt=0),
    case("b4_every_pair", {'n_slots': -1, 'split_join': 0},
         B=16, last_slots=10),
    case("b1_every_pair_small", {'n_slots': -2, 'split_join': 0},
         B=1, last_slots=1),
    case("hand_over_at_tail", {'hand_over': 1},
         B=512, active=85),
    case("hand_over_above_tail", {'hand_over': 0},
         B=512, active=86),
    case("hand_over_none_active", {'hand_over': 0},
         B=512, active=0),
    case("b1_warm_ahead", {'ahead': 1},
         B=1, warm_start=1),
    case("b3_warm_ahead", {'ahead': 1},
         B=3, warm_start=1),
    case("b1_cold_not_ahead", {'ahead': 0},
         B=1),
    case("b1_warm_budget_not_ahead", {'ahead': 0},
         B=1, warm_start=1, budget=1),
    case("b4_warm_not_ahead", {'ahead': 0},
         B=4, warm_start=1),
]


def _line(kw):
    v = {**POLICY, **FACTS, **SOLVE, **ROUND, **SWEEP}
    for k, x in kw.items():
        assert k in v, k
        v[k] = x
    v["last_sweep"] = v["B"] if v["last_sweep"] < 0 else v["last_sweep"]      # (-1: every rollout)
    v["last_slots"] = v["B"] if v["last_slots"] < 0 else v["last_slots"]
    return " ".join(str(int(x)) for x in v.values())


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("schedule_plan") / "schedule_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "schedule_plan_check.cpp")])
    return exe


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_schedule_plan_table(plan_exe):
    inp = "\n".join(_line(kw) for _, _, kw in CASES) + "\n"
    out = subprocess.run([plan_exe], input=inp, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(CASES)
    wrong = []
    for (name, expect, _), line in zip(CASES, out):
        got = dict(t.split("=") for t in line.split())
        diff = {k: (v, got[k]) for k, v in expect.items() if str(v) != got[k]}
        if diff:
            wrong.append((name, diff))
    assert not wrong, wrong
