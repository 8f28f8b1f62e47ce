"""`contactimplicitmpc/jl_amd/csrc/plant_rollout_call.h` built with g++ (tests/native/plant_rollout_call_check.cpp), as a plain program
and as a stand-alone one under AddressSanitizer and UBSan: `plant_rollout_check` on a valid call through each of the eight entry points'
fillings and on every refusal the library's tests make through the built library - the `BAD` tables of tests/test_plant_rollout.py and
tests/test_plant_feedback.py, the gradient and the tape refusals -, and `plant_rollout_layout` against counts written out by hand."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib, plant
import test_plant_feedback as tpf
import test_plant_rollout as tpr

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID = 0, -1
ENTRIES = ("step", "step_terrain", "rollout", "grad", "tape", "feedback", "grad_feedback", "tape_feedback")
# the valid call of tests/test_plant_feedback.py's `_call` has no w; the driver's, like tests/test_plant_rollout.py's, has one
NO_W = ["w=null", "K_w=1", "n_w=1", "hold_w=1"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rollout_call") / "plant_rollout_call_check")
    # the sanitizer runtimes linked statically: the program then runs the same whatever else the loader brings in
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, os.path.join(HERE, "native", "plant_rollout_call_check.cpp")]
    if flags and subprocess.run(cmd, capture_output=True).returncode != 0:
        pytest.skip("this g++ has no static sanitizer runtime")
    subprocess.check_call(cmd)

    def run(queries):
        text = "".join(" ".join(q) + "\n" for q in queries)
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        out = res.stdout.strip().split("\n")
        assert len(out) == len(queries)
        return [line.split() for line in out]
    return run


def _tokens(over):
    """An `over` dict of the library tests' `_call` as the driver's key=value tokens."""
    out = []
    for k, v in over.items():
        if k == "model_name":
            out.append(f"model={plant.model_dims(v)[0]}")
        elif v is None:
            out.append(f"{k}=null")
        elif isinstance(v, _lib.IpOpts):
            out += [f"opts.{n}={float(getattr(v, n)).hex()}" for n, _ in v._fields_]
        elif isinstance(v, C.Array):
            out.append(f"terrain={len(v)}:{bytes(v).hex()}")
        elif isinstance(v, np.ndarray):
            out.append(f"{k}=" + ",".join(float(x).hex() for x in v.ravel()))
        else:
            out.append(f"{k}={float(v).hex()}")
    return out


def _sine(n=1):
    return _tokens(dict(terrain=tpr._terrains(*["sine1_2D_lc"] * n), n_terrain=n))


# ---- the check ---------------------------------------------------------------------------------------------------------------------------
def test_a_valid_call_passes_through_every_entry_and_names_its_model_and_ground(check):
    """hopper_2D (nq 4, nu 2, nc 1), B = 2, T = 3: flat ground is not rough, sine1_2D_lc is; the terrain step needs its terrain."""
    got = check([("check", e, *(_sine() if e == "step_terrain" else [])) for e in ENTRIES])
    assert got == [["0", "4", "2", "1", "1" if e == "step_terrain" else "0"] for e in ENTRIES]
    rough = check([("check", e, *_sine(2)) for e in ENTRIES if e != "step"])
    assert rough == [["0", "4", "2", "1", "1"]] * 7
    assert check([("check", "rollout", *_tokens(dict(terrain=tpr._terrains("flat_2D_lc"), n_terrain=1)))]) == [["0", "4", "2", "1", "0"]]
    assert check([("check", "rollout", *_tokens(dict(model_name="pushbot")))]) == [["0", "2", "2", "2", "0"]]
    # the second valid call of tests/test_plant_rollout.py: no w, one mu, one u schedule, a shared rough terrain
    assert check([("check", "rollout", *NO_W[:1], "K_w=0", "n_w=0", "hold_w=0", "n_mu=1", "n_u=1", "steps_per_launch=2", *_sine())])[0][0] == "0"


@pytest.mark.parametrize("what", sorted(tpr.BAD))
def test_the_rollout_refusals(check, what):
    """Every case of tests/test_plant_rollout.py's BAD, through the open-loop, the gradient and the tape filling."""
    for entry in ("rollout", "grad", "tape"):
        assert check([("check", entry, *_tokens(tpr.BAD[what]))]) == [[str(INVALID)]], entry


def test_the_step_entries_pair_their_terrain(check):
    """cimpc_plant_step passes no terrain; cimpc_plant_step_terrain refuses a null one, a count that is neither 1 nor B and a terrain the
    model cannot stand on; the wall takes no rough terrain."""
    assert check([("check", "step_terrain")]) == [[str(INVALID)]]
    assert check([("check", "step_terrain", "n_terrain=1")]) == [[str(INVALID)]]
    assert check([("check", "step_terrain", *_tokens(dict(n_terrain=3, terrain=tpr._terrains(*["sine1_2D_lc"] * 3))))]) == [[str(INVALID)]]
    assert check([("check", "step_terrain", *_tokens(dict(n_terrain=1, terrain=tpr._terrains("sine1_3D_lc"))))]) == [[str(INVALID)]]
    assert check([("check", "step", "model=6")]) == [[str(INVALID)]]      # particle_2D has no flat ground
    wall = _tokens(dict(model_name="centroidal_quadruped_wall", n_terrain=1, terrain=tpr._terrains("sine1_3D_lc")))
    assert check([("check", e, *wall) for e in ("rollout", "step_terrain")]) == [[str(INVALID)]] * 2


@pytest.mark.parametrize("entry", sorted(tpf.GRAD))
@pytest.mark.parametrize("what", sorted(tpf.BAD))
def test_the_closed_loop_refusals(check, entry, what):
    """Every case of tests/test_plant_feedback.py's BAD through the three closed-loop fillings."""
    fb_over, over = tpf.BAD[what]
    assert check([("check", entry[len("cimpc_plant_rollout_"):], *NO_W, *_tokens(fb_over or {}), *_tokens(over))]) == [[str(INVALID)]]


@pytest.mark.parametrize("over", [dict(n_cols=0), dict(n_cols=15), dict(reg=-1e-9), dict(reg=float("nan")), dict(reg=float("inf")), dict(grad_status=None)])
def test_the_gradient_refusals(check, over):
    """hopper_2D has nθ = 14 columns; reg is finite and not negative; the status is not optional, z is."""
    for entry in ("grad", "tape", "grad_feedback", "tape_feedback"):
        assert check([("check", entry, *_tokens(over))]) == [[str(INVALID)]], entry
    assert check([("check", e, "z=null", "n_cols=14") for e in ("grad", "tape")]) == [["0", "4", "2", "1", "0"]] * 2


def test_dz_is_needed_without_a_tape_and_a_tape_needs_the_columns_of_q0_q1_and_u(check):
    assert check([("check", e, "dz=null") for e in ("grad", "grad_feedback")]) == [[str(INVALID)]] * 2
    assert check([("check", e, "n_cols=9") for e in ("tape", "tape_feedback")]) == [[str(INVALID)]] * 2      # 2 nq + nu = 10
    assert check([("check", "grad", "n_cols=9")])[0][0] == "0"
    # T B past INT_MAX is refused where the sensitivity launch would count its entries in an int
    assert check([("check", "grad", "T=1073741824"), ("check", "rollout", "T=1073741824")]) == [[str(INVALID)], ["0", "4", "2", "1", "0"]]


def test_the_gains_are_not_read_before_their_schedule_is_checked(check):
    """K and x_ref of one double each: with a null K, or with K_f = 0 beside a K that is there, the call is refused, and the sanitized
    program would end at any read past the one double (the finite scan runs over K_f n_f 2nq nu of them)."""
    one = ["K=0x0p+0", "x_ref=0x0p+0"]
    got = check([("check", "feedback", *NO_W, "K=null", one[1]), ("check", "feedback", *NO_W, "K_f=0", *one),
                 ("check", "tape_feedback", *NO_W, "x_ref=null", one[0]), ("check", "grad_feedback", *NO_W, "n_f=3", *one)])
    assert got == [[str(INVALID)]] * 4


# ---- the layout --------------------------------------------------------------------------------------------------------------------------
BUFFERS = {"need_in": ("q", "u", "w", "mu"), "need_out": ("gamma", "b"), "need_st": ("status", "iters"), "need_z": ("z",), "need_grad": ("dz",),
           "need_grad_st": ("grad_status",), "need_fb": ("fb_K", "x_ref", "u_applied", "fb_err")}


def _layout(check, entry, *tokens):
    rc, *rest = check([("layout", entry, *tokens)])[0]
    assert rc == "0"
    L, k = {}, 0
    while k < len(rest):
        if rest[k] in ("row", "TB") or rest[k].startswith("need_"):
            L[rest[k]] = int(rest[k + 1]); k += 2
        else:
            L[rest[k]] = (int(rest[k + 1]), int(rest[k + 2])); k += 3
    return L


def _regions_tile_their_buffers(L, in_tape=False):
    """The regions of a buffer follow each other from 0 in the documented order, and their sum is what the buffer is grown to - but for a
    tape's dz and status, which are laid out in the tape's own memory while the workspace's are asked for nothing."""
    for need, names in BUFFERS.items():
        at = 0
        for n in names:
            assert L[n][0] == at, (n, L[n], at)
            at += L[n][1]
        assert L[need] == (0 if in_tape and need in ("need_grad", "need_grad_st") else at), need


def test_layout_of_the_open_loop_hopper_call(check):
    """hopper_2D (nq 4, nu 2, nc 1, nb 2), B = 2, T = 3, u per robot with K_u = 2, no w, one mu."""
    L = _layout(check, "rollout", *NO_W, "n_mu=1")
    assert (L["row"], L["TB"]) == (8, 6)
    assert L["q"] == (0, 40) and L["u"] == (40, 8) and L["w"] == (48, 0) and L["mu"] == (48, 0) and L["need_in"] == 48
    assert L["gamma"] == (0, 6) and L["b"] == (6, 12) and L["need_out"] == 18
    assert L["status"] == (0, 6) and L["iters"] == (6, 6) and L["need_st"] == 12
    for k in ("z", "dz", "grad_status", "fb_K", "x_ref", "u_applied", "fb_err"):
        assert L[k] == (0, 0), k
    assert L["need_z"] == L["need_grad"] == L["need_grad_st"] == L["need_fb"] == 0
    _regions_tile_their_buffers(L)
    step = _layout(check, "step")      # one step: three trajectory rows, a u and a w row per robot, one mu
    assert step["q"] == (0, 24) and step["u"] == (24, 4) and step["w"] == (28, 4) and step["mu"] == (32, 0) and step["need_st"] == 4


@pytest.mark.parametrize("entry", ["grad_feedback", "tape_feedback"])
def test_layout_with_everything_on(check, entry):
    """pushbot (nq 2, nu 2, nc 2, nb 4, nw 2, nz 18, nθ 10, nr 8), B = 3, T = 5: u per robot with K_u = 2, w per robot with K_w = 3, a mu per
    robot, every column of θ, a shared schedule of K_f = 2 rows."""
    L = _layout(check, entry, "model=12", "B=3", "T=5", "n_w=3", "n_cols=10", "n_f=1", "K_f=2")
    tape = entry == "tape_feedback"
    assert (L["row"], L["TB"]) == (6, 15)
    assert L["q"] == (0, 42) and L["u"] == (42, 12) and L["w"] == (54, 18) and L["mu"] == (72, 3) and L["need_in"] == 75
    assert L["gamma"] == (0, 30) and L["b"] == (30, 60) and L["need_out"] == 90
    assert L["status"] == (0, 15) and L["iters"] == (15, 15) and L["need_st"] == 30
    assert L["z"] == (0, 270) and L["need_z"] == 270
    assert L["dz"] == (0, 1200) and L["grad_status"] == (0, 15)
    assert (L["need_grad"], L["need_grad_st"]) == ((0, 0) if tape else (1200, 15))
    # the K region stays at the head of d_fb when the tape owns K
    assert L["fb_K"] == (0, 16) and L["x_ref"] == (16, 8) and L["u_applied"] == (24, 30) and L["fb_err"] == (54, 60) and L["need_fb"] == 114
    _regions_tile_their_buffers(L, in_tape=tape)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_tiles_its_buffers(check, entry):
    L = _layout(check, entry, *(_sine() if entry == "step_terrain" else []))
    _regions_tile_their_buffers(L, in_tape=entry.startswith("tape"))
    assert (L["need_z"] > 0) == ("grad" in entry or "tape" in entry) and (L["need_fb"] > 0) == entry.endswith("feedback")
