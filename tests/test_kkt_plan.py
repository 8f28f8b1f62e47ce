"""`contactimplicitmpc/jl_amd/csrc/kkt_plan.h` - which kernel serves each KKT stage - is plain C++: built here with g++
(tests/native/kkt_plan_check.cpp) and driven through a table of named cases.  The expected forms are the kernels the
launch sites chose before the policy moved into the header (lock-step rounds, persistent kernel, B1 seam)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

CAPS = ("cfg", "velocity", "cf_tiny", "wide_tiles", "condensed", "mfma", "packed", "twisted", "duo", "mixed", "banded",
        "cf_reduce", "banded_twisted")
# quadruped (nq 11, nu 8), H = 40: every condensed kernel applies
QUAD = dict(cfg=1, condensed=1, mfma=1, packed=1, twisted=1, duo=1, mixed=1)
# centroidal quadruped (nq 18, nu 12), H = 60: 24-wide tiles, no duo kernel
WIDE = dict(cfg=1, wide_tiles=1, condensed=1, mfma=1, packed=1, twisted=1, mixed=1)
QUAD_H100 = dict(cfg=1, condensed=1)                   # beyond kkt_max_h = 96 of 16-wide tiles: no MFMA kernel, no compact list
WIDE_H100 = dict(cfg=1, wide_tiles=1, condensed=1, mfma=1)   # within kkt_max_h = 108 of 24-wide tiles, beyond the list kernels' 96
TILES_25 = dict(cfg=1, condensed=1)                    # a compiled pair with tiles beyond 24: scalar kernel only
VELOCITY = dict(cfg=1, velocity=1, condensed=1, mfma=1, packed=1, twisted=1, duo=1, banded=1, banded_twisted=1)
# :configurationforce: the caps as the handle fills them - tested on the cf-mode problem, so no :configuration-mode kernel applies
# (mfma, packed, twisted, duo 0); the reduction's own solvers are cf_reduce and, with a velocity objective, banded_twisted
CF_TINY = dict(cf_tiny=1, condensed=1, cf_reduce=1)
CF_TINY_VEL = dict(velocity=1, cf_tiny=1, condensed=1, cf_reduce=1, banded_twisted=1)
CF_HEAVY = dict(condensed=1, cf_reduce=1)              # impulse weights above fp64 resolution: the dense LU

POLICY = dict(kkt_pipe=-1, kkt_twisted=-1, kkt_duo=1, kkt_duo_hint=20000, kkt_duo_max=256, kkt_tw_max=120, kkt_pipe_max=128,
              async_kkt_tw=1, lazy_dz=1, kkt_overlap=-1)
SEAM, ROUND, PERSISTENT, TAIL = 0, 1, 3, 4
SITE = dict(kind=ROUND, attempt=0, n_kkt=1, blind=0, sweep_problems=0, tw_off=0, B=1, async_tail=96, waves=4)


def case(name, caps, expect, want=0, lazy=None, backend=None, **kw):
    pol = {k: kw.pop(k) for k in list(kw) if k in POLICY}
    site = {k: kw.pop(k) for k in list(kw) if k in SITE}
    assert not kw, kw
    return name, caps, want, {**POLICY, **pol}, {**SITE, **site}, expect, lazy, backend


CASES = [
    # headline: B = 512 quadruped H = 40, overlapped rounds
    case("headline_many_systems_packed", QUAD, "Packed", lazy=1, B=512, n_kkt=400, sweep_problems=61440),
    case("headline_few_systems_short_sweep_duo", QUAD, "Duo", B=512, n_kkt=20, sweep_problems=4000),
    case("headline_few_systems_long_sweep_packed", QUAD, "Packed", B=512, n_kkt=20, sweep_problems=30000),
    case("headline_duo_hint_is_inclusive", QUAD, "Duo", B=512, n_kkt=20, sweep_problems=20000),
    case("headline_duo_max_inclusive", QUAD, "Duo", B=512, n_kkt=256, sweep_problems=4000),
    case("headline_duo_max_bound", QUAD, "Packed", B=512, n_kkt=257, sweep_problems=4000),
    case("headline_blind_round_not_duo", QUAD, "Packed", B=512, n_kkt=20, blind=1, sweep_problems=4000),
    case("headline_duo_off", QUAD, "Packed", B=512, n_kkt=20, sweep_problems=4000, kkt_duo=0),
    # the overlapped rounds' twisted kernel: batches within the pair bound of 120
    case("b96_overlapped_twisted", QUAD, "Twisted", B=96, n_kkt=40, sweep_problems=30000),
    case("b120_overlapped_twisted", QUAD, "Twisted", B=120, n_kkt=120, sweep_problems=30000),
    case("b128_overlapped_not_twisted", QUAD, "Packed", B=128, n_kkt=40, sweep_problems=30000),
    case("b128_twisted_bound_from_knob", QUAD, "Twisted", B=128, n_kkt=40, sweep_problems=30000, kkt_twisted=64),
    case("b128_twisted_bound_from_knob_exceeded", QUAD, "Packed", B=128, n_kkt=65, sweep_problems=30000, kkt_twisted=64),
    # rounds on the sweep's stream (B < 64)
    case("b1_round_twisted", QUAD, "Twisted", B=1, n_kkt=1),
    case("b16_round_twisted", QUAD, "Twisted", B=16, n_kkt=16),
    case("b16_round_blind_twisted", QUAD, "Twisted", B=16, n_kkt=16, blind=1),
    case("b1_round_twisted_off_pipelined", QUAD, "Pipelined", B=1, n_kkt=1, kkt_twisted=0),
    case("b1_round_pipe_off_packed", QUAD, "Packed", B=1, n_kkt=1, kkt_pipe=0),
    case("b512_forced_pipe_overlapped_twisted_beyond_pair_bound", QUAD, "Pipelined", B=512, n_kkt=121, kkt_pipe=1),
    case("b512_forced_pipe_overlapped_twisted", QUAD, "Twisted", B=512, n_kkt=120, kkt_pipe=5),
    case("b48_forced_overlap_twisted", QUAD, "Twisted", B=48, n_kkt=48, sweep_problems=30000, kkt_overlap=1),
    case("b256_no_overlap_pipe_bound", QUAD, "Packed", B=256, n_kkt=129, kkt_overlap=0, kkt_twisted=0),
    case("b256_no_overlap_pipelined", QUAD, "Pipelined", B=256, n_kkt=128, kkt_overlap=0, kkt_twisted=0),
    # wide tiles: the three-wave kernels everywhere
    case("wide_b64_twisted", WIDE, "Twisted", B=64, n_kkt=64, sweep_problems=4000),
    case("wide_b256_many_systems_pipelined", WIDE, "Pipelined", B=256, n_kkt=121, sweep_problems=4000),
    case("wide_b64_pipe_off_overlapped_twisted", WIDE, "Twisted", B=64, n_kkt=64, sweep_problems=30000, kkt_pipe=0),
    # a twisted hand-over timed out in this solve: one-ended kernels everywhere
    case("tw_off_round", QUAD, "Pipelined", B=1, n_kkt=1, tw_off=1),
    case("tw_off_overlapped", QUAD, "Packed", B=96, n_kkt=40, tw_off=1, sweep_problems=30000),
    case("tw_off_duo", QUAD, "Packed", B=512, n_kkt=20, sweep_problems=4000, tw_off=1),
    case("tw_off_persistent", QUAD, "AsyncOneEnded", kind=PERSISTENT, B=16, tw_off=1),
    case("tw_off_wide", WIDE, "Pipelined", B=64, n_kkt=64, tw_off=1),
    case("tw_off_banded", VELOCITY, "BandedOneEnded", B=16, n_kkt=16, tw_off=1),
    # B1 seam (cimpc_kkt_solve)
    case("seam_b1_twisted", QUAD, "Twisted", kind=SEAM, B=1),
    case("seam_b120_twisted", QUAD, "Twisted", kind=SEAM, B=120),
    case("seam_b121_per_rollout", QUAD, "PerRollout", kind=SEAM, B=121),
    case("seam_duo2", QUAD, "Duo", kind=SEAM, B=1, kkt_duo=2),
    case("seam_duo2_waives_pair_bound", QUAD, "Duo", kind=SEAM, B=512, kkt_duo=2),
    case("seam_duo2_wide_twisted", WIDE, "Twisted", kind=SEAM, B=4, kkt_duo=2),
    case("seam_second_attempt_one_ended", QUAD, "PerRollout", kind=SEAM, B=1, attempt=1),
    case("seam_twisted_off", QUAD, "PerRollout", kind=SEAM, B=1, kkt_twisted=0),
    # beyond the MFMA kernels' bounds
    case("long_horizon_scalar_round", QUAD_H100, "Scalar", lazy=0, B=1, n_kkt=1),
    case("long_horizon_scalar_overlapped", QUAD_H100, "Scalar", B=512, n_kkt=20, sweep_problems=4000),
    case("long_horizon_scalar_seam", QUAD_H100, "Scalar", kind=SEAM, B=1),
    case("long_horizon_wide_per_rollout", WIDE_H100, "PerRollout", lazy=0, B=512, n_kkt=400),
    case("tiles_beyond_24_scalar", TILES_25, "Scalar", B=1, n_kkt=1),
    # persistent kernel
    case("persistent_b32_two_jobs", QUAD, "AsyncTwoJob", kind=PERSISTENT, B=32),
    case("persistent_b4_two_jobs", QUAD, "AsyncTwoJob", kind=PERSISTENT, B=4),
    case("persistent_b64_one_ended", QUAD, "AsyncOneEnded", kind=PERSISTENT, B=64),
    case("hybrid_tail_32_two_jobs", QUAD, "AsyncTwoJob", kind=TAIL, B=512, async_tail=32),
    case("hybrid_tail_33_one_ended", QUAD, "AsyncOneEnded", kind=TAIL, B=512, async_tail=33),
    case("hybrid_tail_96_one_ended", QUAD, "AsyncOneEnded", kind=TAIL, B=128, async_tail=96),
    case("persistent_async_kkt_tw_0", QUAD, "AsyncOneEnded", kind=PERSISTENT, B=16, async_kkt_tw=0),
    case("persistent_async_kkt_tw_2", QUAD, "AsyncTwoJob", kind=PERSISTENT, B=64, async_kkt_tw=2),
    case("hybrid_tail_async_kkt_tw_2", QUAD, "AsyncTwoJob", kind=TAIL, B=512, async_tail=96, async_kkt_tw=2),
    case("persistent_twisted_off", QUAD, "AsyncOneEnded", kind=PERSISTENT, B=16, kkt_twisted=0),
    case("persistent_nq_beyond_16", WIDE, "AsyncOneEnded", kind=PERSISTENT, B=16),
    case("persistent_two_wave_workgroups", QUAD, "AsyncOneEnded", kind=PERSISTENT, B=16, waves=2),
    # backends
    case("velocity_b96_banded_twisted", VELOCITY, "BandedTwisted", lazy=0, B=96, n_kkt=40),
    case("velocity_b120_banded_twisted", VELOCITY, "BandedTwisted", B=120, n_kkt=40),
    case("velocity_b121_banded_one_ended", VELOCITY, "BandedOneEnded", B=121, n_kkt=40),
    case("velocity_seam_banded_twisted", VELOCITY, "BandedTwisted", kind=SEAM, B=1),
    case("velocity_seam_second_attempt", VELOCITY, "BandedOneEnded", kind=SEAM, B=1, attempt=1),
    case("velocity_twisted_off", VELOCITY, "BandedOneEnded", B=16, n_kkt=16, kkt_twisted=0),
    case("velocity_without_twisted_caps", {**VELOCITY, "banded_twisted": 0}, "BandedOneEnded", B=16, n_kkt=16),
    case("banded_on_request", {**QUAD, "banded": 1}, "BandedOneEnded", want=2, lazy=0, B=512, n_kkt=16),
    case("banded_on_request_does_not_fit", QUAD, "Dense", want=2, lazy=0, B=16, n_kkt=16),
    case("cf_tiny_reduced_condensed", CF_TINY, "PerRollout", lazy=0, backend="CfCondensed", B=512, n_kkt=20, sweep_problems=4000),
    case("cf_tiny_reduced_seam", CF_TINY, "PerRollout", backend="CfCondensed", kind=SEAM, B=1),
    case("cf_tiny_velocity_reduced_banded_twisted", CF_TINY_VEL, "BandedTwisted", lazy=0, backend="CfBanded", B=16, n_kkt=16),
    case("cf_tiny_velocity_reduced_banded_b121", CF_TINY_VEL, "BandedOneEnded", B=121, n_kkt=16),
    case("cf_tiny_reduced_b1_round", CF_TINY, "PerRollout", backend="CfCondensed", B=1, n_kkt=1),
    case("cf_heavy_dense", CF_HEAVY, "Dense", lazy=0, backend="DenseLu", B=16, n_kkt=16),
    case("cf_tiny_dense_on_request", CF_TINY, "Dense", want=1, B=16, n_kkt=16),
    case("mixed_backend", QUAD, "PerRollout", want=3, lazy=0, B=512, n_kkt=400),
    case("mixed_seam", QUAD, "PerRollout", want=3, kind=SEAM, B=1),
    case("mixed_unavailable_condensed", {**QUAD, "mixed": 0}, "Twisted", want=3, lazy=1, B=1, n_kkt=1),
    case("dense_lu_on_request", QUAD, "Dense", want=1, lazy=0, B=512, n_kkt=400),
    case("no_compiled_condensed_dense", {"cfg": 1}, "Dense", lazy=0, B=1, n_kkt=1),
    case("headline_lazy_dz_off", QUAD, "Packed", lazy=0, B=512, n_kkt=400, sweep_problems=61440, lazy_dz=0),
]

BACKEND = {"PerRollout": None, "Scalar": None, "Packed": "Condensed", "Pipelined": "Condensed", "Twisted": "Condensed",
           "Duo": "Condensed", "AsyncOneEnded": "Condensed", "AsyncTwoJob": "Condensed"}
TWO_ENDED = {"Twisted", "Duo", "BandedTwisted", "AsyncTwoJob"}


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("kkt_plan") / "kkt_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "native", "kkt_plan_check.cpp")])
    return exe


def _run(exe, cases):
    lines = []
    for _, caps, want, pol, site, _, _, _ in cases:
        v = [int(caps.get(k, 0)) for k in CAPS] + [want] + list(pol.values()) + list(site.values())
        lines.append(" ".join(str(x) for x in v))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [o.split() for o in out[:len(cases)]]


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


def test_kkt_plan_table(plan_exe):
    got = _run(plan_exe, CASES)
    wrong = []
    for (name, _, _, _, _, expect, lazy, want_be), (backend, form, two, lz) in zip(CASES, got):
        want_be = want_be or BACKEND.get(expect)
        if form != expect or int(two) != (form in TWO_ENDED) or (lazy is not None and int(lz) != lazy) or \
                (want_be is not None and backend != want_be):
            wrong.append((name, expect, lazy, backend, form, lz))
    assert not wrong, wrong
