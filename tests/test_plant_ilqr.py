"""The device-resident iLQR loop (`cimpc_plant_ilqr`, `plant.ilqr(device_loop=True)`) without a device:
csrc/plant_ilqr.h built with g++ against the NumPy lines of `plant.ilqr` (`plant_ilqr_cases.rules_np`) bit for bit, on a few thousand
random robots and the edge states; the export, its ctypes signature and its Julia call, by text; every refusal that needs no device, each
by its reason, with *new_tape left NULL; the Python keyword's own refusals; and the host program under AddressSanitizer and UBSan.
tests/README_plant_ilqr.md has the rest."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import plant_ilqr_cases as pic

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "plant_ilqr_check.cpp")
NAME = "cimpc_plant_ilqr"
INVALID = -1
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "const int*": _lib._ip,
         "cimpc_plant_tape": C.c_void_p, "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
         "const cimpc_tracking_cost*": C.POINTER(_lib.TrackingCost), "cimpc_plant_tape*": C.POINTER(C.c_void_p)}
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*", "const int*"},
             "Ptr{Cvoid}": {"cimpc_plant_tape"}, "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"},
             "Ref{TrackingCostC}": {"const cimpc_tracking_cost*"}, "Ref{Ptr{Cvoid}}": {"cimpc_plant_tape*"}, "Ref{Cint}": {"int*"}}
RHO0, FACTOR, TOP = 1e-6, 10.0, 8
LADDER = pic.ladder(RHO0, FACTOR, TOP)
RHO_MAX, TOL = float(LADDER[4]), 1e-3
ALPHAS = (1.0, 0.5, 0.25)


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_rules(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("ilqr") / "plant_ilqr_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


def run_rules(exe, s, lad, alphas, rho_max, tol):
    hx = lambda x: float(x).hex()
    N = len(s["level"])
    text = [f"{N} {len(lad)} {len(alphas)}", f"{hx(rho_max)} {hx(tol)}", " ".join(hx(v) for v in lad), " ".join(hx(v) for v in alphas)]
    for i in range(N):
        text.append(f"{s['level'][i]} {int(s['active'][i])} {hx(s['J'][i])} {s['choice'][i]} {s['lq_status'][i]} " + " ".join(hx(v) for v in s["J_cand"][:, i]))
    res = subprocess.run([exe, "rules"], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [line.split() for line in res.stdout.strip().split("\n")]
    assert len(rows) == N
    f = lambda k: np.array([float.fromhex(r[k]) for r in rows])
    i = lambda k: np.array([int(r[k]) for r in rows])
    return dict(rho=f(0), J_nom=f(1), level=i(2), active=i(3).astype(bool), J=f(4), hist_J=f(5), alpha=f(6), hist_rho=f(7), accepted=i(8).astype(bool))


def same(a, b):
    """Bit for bit, NaN matching NaN (a NaN's sign and payload are not the rule's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.tolist() == b.tolist()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.ascontiguousarray(a[~nan]).tobytes() == np.ascontiguousarray(b[~nan].astype(a.dtype)).tobytes()


def assert_rules(got, want, names=None):
    for key, ref in (("rho", "rho"), ("J_nom", "J_nom"), ("level", "level"), ("active", "active"), ("J", "J"), ("hist_J", "J"), ("alpha", "alpha"),
                     ("hist_rho", "rho"), ("accepted", "accepted")):
        if not same(got[key], want[ref]):
            bad = [k for k in range(len(want[ref])) if not same(got[key][k:k + 1], np.asarray(want[ref])[k:k + 1])]
            raise AssertionError(f"{key} differs at states {bad[:8]}" + (f" ({[names[k] for k in bad if k in names]})" if names else ""))


def test_the_host_build_of_the_rules_is_the_numpy_lines_bit_for_bit(host_rules):
    s, edge_names = pic.states(11, 4000, len(ALPHAS), LADDER, RHO_MAX, TOL)
    N = len(s["level"])
    names = {N - len(edge_names) + k: name for k, name in enumerate(edge_names)}
    want = pic.rules_np(s["level"], s["active"], s["J"], s["J_cand"], s["choice"], s["lq_status"], ALPHAS, LADDER, RHO_MAX, TOL)
    got = run_rules(host_rules, s, LADDER, ALPHAS, RHO_MAX, TOL)
    assert_rules(got, want, names)
    # the random states are not one-sided: every branch of the rules is taken many times
    acc, act = want["accepted"], s["active"]
    assert 500 < acc.sum() < N - 500 and (want["active"] & act).sum() > 300 and (act & ~want["active"]).sum() > 300
    assert (~np.isfinite(want["J_nom"])).sum() > 300 and (want["level"] < s["level"]).sum() > 300 and (want["level"] > s["level"]).sum() > 300


def test_the_edge_states_do_what_the_loop_does(host_rules):
    """Each edge state's outcome written out by hand, so that a rule changed in the header AND in the restatement still fails here."""
    s, edge_names = pic.states(11, 0, len(ALPHAS), LADDER, RHO_MAX, TOL)
    got = run_rules(host_rules, s, LADDER, ALPHAS, RHO_MAX, TOL)
    at = {name: k for k, name in enumerate(edge_names)}
    top = len(LADDER) - 1
    expect = {      # name -> (level', active', accepted)
        "J = 0 with tol > 0, accepted at J_new = 0": (0, True, True),       # 0 - 0 < tol 0 is false: not small
        "J_new = J exactly": (1, False, True),                               # a zero decrease is small
        "J_new one ulp below J": (1, False, True),
        "a rejection onto the last ladder entry": (top, False, False),       # the last entry lies above rho_max
        "accepted at the last ladder entry": (top - 1, False, True),
        "inactive at the last ladder entry": (top, False, False),
        "a rejection onto rho = rho_max exactly": (4, True, False),          # rho <= rho_max holds with equality
        "a rejection past rho_max": (5, False, False),
        "an acceptance down onto rho_max exactly": (4, True, True),
        "a NaN J_cand on a rejected robot": (1, True, False),
        "an inactive robot that is accepted nowhere": (3, False, False),
        "a backward pass that ended early": (1, True, False),
        "level 0 accepted stays at level 0": (0, True, True),
        "a negative J": (0, True, True),
    }
    assert sorted(expect) == sorted(edge_names)
    for name, (level, active, accepted) in expect.items():
        k = at[name]
        assert (got["level"][k], bool(got["active"][k]), bool(got["accepted"][k])) == (level, active, accepted), name
    k = at["a NaN J_cand on a rejected robot"]
    assert got["J"][k] == 2.0 and np.isnan(got["alpha"][k]) and got["hist_J"][k] == 2.0
    k = at["a backward pass that ended early"]
    assert got["J_nom"][k] == -np.inf and got["rho"][k] == LADDER[0]
    k = at["an inactive robot that is accepted nowhere"]
    assert got["J_nom"][k] == -np.inf and got["hist_rho"][k] == LADDER[3]


VALID = {"max_iter 0": ((0, 3, [1.0, 2.0, 3.0]), "max_iter below 1"),
         "a short ladder": ((3, 3, [1.0, 2.0, 3.0]), "a ladder shorter than max_iter + 1"),
         "a negative entry": ((2, 3, [1.0, -2.0, 3.0]), "a ladder entry that is negative or not finite"),
         "an infinite entry": ((2, 3, [1.0, 2.0, float("inf")]), "a ladder entry that is negative or not finite"),
         "a NaN entry": ((1, 2, [float("nan"), 2.0]), "a ladder entry that is negative or not finite"),
         "good": ((2, 3, [0.0, 2.0, 3.0]), "ok")}


@pytest.mark.parametrize("what", sorted(VALID))
def test_the_loops_own_refusals_in_the_host_build(host_rules, what):
    (max_iter, n_ladder, lad), reason = VALID[what]
    text = f"{max_iter} {n_ladder} {float(1e6).hex()} {float(1e-6).hex()}\n" + " ".join(float(v).hex() for v in lad) + "\n"
    res = subprocess.run([host_rules, "valid"], input=text, capture_output=True, text=True, check=True)
    assert res.stdout.strip() == reason


def test_the_host_build_runs_clean_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_ilqr_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    s, _ = pic.states(12, 500, len(ALPHAS), LADDER, RHO_MAX, TOL)
    want = pic.rules_np(s["level"], s["active"], s["J"], s["J_cand"], s["choice"], s["lq_status"], ALPHAS, LADDER, RHO_MAX, TOL)
    assert_rules(run_rules(exe, s, LADDER, ALPHAS, RHO_MAX, TOL), want)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


def test_the_export_is_declared_and_bound():
    params = _prototype(NAME)
    assert NAME in _lib.SIGNATURES, f"{NAME} has no ctypes signature"
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(params) == 55
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), NAME)
    # the rollout arguments are those of cimpc_plant_tape_linesearch_box, under the same names
    names = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"\bint\s+" + n + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S).group(1).split(",")]
    mine, theirs = names(NAME), names("cimpc_plant_tape_linesearch_box")
    shared = ["tape", "steps_per_launch", "n_terrain", "terrain", "q_nom", "u_nom", "w", "K_w", "n_w", "hold_w", "mu", "n_mu", "h", "opts", "n_alpha", "alpha",
              "armijo", "cost", "reg", "n_lim", "u_lo", "u_hi", "new_tape"]
    ptypes = dict(zip(theirs, _prototype("cimpc_plant_tape_linesearch_box")))
    for name, ctype in zip(mine, params):
        if name in shared:
            assert ptypes[name] == ctype, name
    assert set(shared) <= set(mine)


def test_the_source_is_built_and_exported():
    make = open(os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc", "Makefile")).read()
    assert "plant_ilqr.hip" in make and "plant_ilqr.h" in make and "plant_stage_launch.h" in make
    src = open(os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc", "plant_ilqr.hip")).read()
    assert 'extern "C" int cimpc_plant_ilqr(' in src and '#include "plant_ilqr.h"' in src and "asm" not in src
    loop = src[src.index("for (int it = 0; it < max_iter"):src.index("// down, once")]
    assert "hipMalloc" not in loop and "plant_grow" not in loop and loop.count("down(") == 1 and "up(" not in loop, "a transfer or an allocation inside the loop"


def test_julia_call_matches_the_prototype():
    assert "function plant_ilqr(" in JL, "julia/CIMPCHip.jl has no plant_ilqr"
    fn = JL[JL.index("function plant_ilqr("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + NAME + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"plant_ilqr does not call {NAME}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = _prototype(NAME)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"
    doc = JL[:JL.index("function plant_ilqr(")][-3000:]
    assert "unexecuted" in doc.lower(), "the docstring must say that the Julia call has not been run"


# what is changed in the stand-in call -> the reason left for cimpc_last_error(NULL).  The stand-in tape is zeroed memory: model 0, B = 0, no
# device memory, which is what the last of the tape-free checks refuses.
REFUSED = {
    "max_iter 0": (dict(max_iter=0), "max_iter below 1"),
    "a short ladder": (dict(max_iter=3), "a ladder shorter than max_iter + 1"),
    "a negative ladder entry": (dict(ladder=[1e-6, -1e-5, 1e-4]), "a ladder entry that is negative or not finite"),
    "an infinite ladder entry": (dict(ladder=[1e-6, float("inf"), 1e-4]), "a ladder entry that is negative or not finite"),
    "a NaN ladder entry": (dict(ladder=[1e-6, 1e-5, float("nan")]), "a ladder entry that is negative or not finite"),
    "a NaN tol": (dict(tol=float("nan")), "rho_max or tol not a number"),
    "null ladder": (dict(ladder=None), "null ladder"),
    "null J_nom": (dict(null="J_nom"), "null J_nom"),
    "null hist_rho": (dict(null="hist_rho"), "null hist_rho"),
    "null n_iter": (dict(null="n_iter"), "null n_iter"),
    "null tape": (dict(null="tape"), "null tape"),
    # what cimpc_plant_tape_linesearch_box refuses
    "n_alpha 0": (dict(n_alpha=0), "n_alpha outside 1 .. 64"),
    "n_alpha 65": (dict(n_alpha=65), "n_alpha outside 1 .. 64"),
    "an infinite alpha": (dict(alpha=[1.0, float("inf")]), "a non-finite alpha"),
    "a negative armijo": (dict(armijo=-1.0), "armijo negative or not a number"),
    "a null pointer in the cost": (dict(cost_null=True), "a null pointer in the cost"),
    "n_Q 0": (dict(n_Q=0), "n_Q, n_R or n_x of the cost below 1"),
    "h 0": (dict(h=0.0), "h not positive"),
    "u_lo alone": (dict(u_hi=None), "one of u_lo, u_hi without the other"),
    "n_lim 3": (dict(n_lim=3), "n_lim neither 1 nor B"),
    "a zeroed tape": (dict(), "a closed tape"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_the_entry_refuses_by_reason_without_a_device_and_leaves_no_tape(what):
    change, reason = REFUSED[what]
    a = dict(max_iter=2, ladder=[1e-6, 1e-5, 1e-4], tol=1e-6, rho_max=1e6, n_alpha=2, alpha=[1.0, 0.5], armijo=1e-4, h=0.01, n_Q=1, cost_null=False, n_lim=1,
             u_lo=None, u_hi=None, null=None)
    if what in ("u_lo alone", "n_lim 3"):
        a.update(u_lo=[[-1.0] * 16], u_hi=[[1.0] * 16])
    a.update(change)
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    some = np.zeros(64)
    somei = np.zeros(64, dtype=np.int32)
    D, I = dp(some), somei.ctypes.data_as(_lib._ip)
    cost = _lib.TrackingCost(None if a["cost_null"] else D, D, D, D, D, a["n_Q"], 1, 1)
    opts = _lib.IpOpts()
    lad, al, lo, hi = arr(a["ladder"]), arr(a["alpha"]), arr(a["u_lo"]), arr(a["u_hi"])
    handle = C.c_void_p(0xdead)      # what a refusal must overwrite with NULL
    n_iter = C.c_int(-7)
    p = dict(tape=C.cast(C.create_string_buffer(4096), C.c_void_p), J_nom=D, hist_rho=D, n_iter=C.byref(n_iter))
    if a["null"]:
        p[a["null"]] = None
    lib = _lib.load()
    rc = lib.cimpc_plant_ilqr(p["tape"], 0, 0, None, D, D, D, D, I, I, p["J_nom"], D, D, None, 1, 1, 1, D, 1, a["h"], C.byref(opts), C.byref(cost),
                              a["n_alpha"], dp(al), a["armijo"], 1e-8, 0 if lad is None else lad.size, dp(lad), a["rho_max"], a["tol"], a["max_iter"],
                              a["n_lim"], dp(lo), dp(hi), D, D, D, D, I, I, D, D, I, D, D, p["hist_rho"], I, p["n_iter"], None, None, None, None, None, None,
                              C.byref(handle))
    assert rc == INVALID
    assert lib.cimpc_last_error(None).decode() == NAME + ": " + reason
    assert handle.value is None, "*new_tape must be NULL after a refusal"
    assert n_iter.value == -7 and not some.any() and not somei.any(), "a refusal wrote to an output"


def test_a_null_new_tape_is_refused_first():
    lib = _lib.load()
    rc = lib.cimpc_plant_ilqr(None, 0, 0, None, *([None] * 9), None, 1, 1, 1, None, 1, 0.01, None, None, 1, None, 0.0, 0.0, 0, None, 0.0, 0.0, 0, 1, None, None,
                              *([None] * 20), None)
    assert rc == INVALID and lib.cimpc_last_error(None).decode() == NAME + ": null new_tape"


# ---- the Python keyword ------------------------------------------------------------------------------------------------------------------------
def test_python_refuses_wrong_shapes_before_the_library_is_called(monkeypatch):
    from contactimplicitmpc.jl_amd import plant
    import inspect
    assert inspect.signature(plant.ilqr).parameters["device_loop"].default is False
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    nq, nu, B, T = 4, 2, 3, 5
    good_cost = plant.TrackingCost(np.eye(2 * nq), np.eye(nu))
    a = ["hopper_2D", np.zeros((B, nq)), np.zeros((B, nq)), np.zeros((T, nu)), 0.01, 0.5, good_cost]
    with_ = lambda k, v: [v if i == k else x for i, x in enumerate(a)]
    for args, kw, match in ((with_(3, np.zeros((T, nu + 1))), {}, "u must be"), (with_(3, np.zeros((T, 2, nu))), {}, "robots"),
                            (with_(1, np.zeros((B, nq + 1))), {}, "q1 and v1"), (with_(6, plant.TrackingCost(np.eye(3), np.eye(nu))), {}, "TrackingCost"),
                            (with_(6, plant.TrackingCost(np.eye(2 * nq), np.eye(nu), x_goal=np.zeros((T, 2 * nq)))), {}, "x_goal"),
                            (a, dict(max_iter=0), "max_iter"), (a, dict(alphas=()), "alphas"), (a, dict(alphas=(1.0, np.inf)), "alphas"),
                            (a, dict(armijo=-1.0), "armijo"), (a, dict(rho0=-1e-6), "rho0"), (a, dict(rho_factor=1e200, max_iter=3), "rho0"),
                            (a, dict(tol=np.nan), "rho_max and tol"), (a, dict(u_lo=[-1.0, -1.0]), "go together"),
                            (a, dict(u_lo=[0.0], u_hi=[1.0]), "must be"), (a, dict(u_lo=[2.0, 0.0], u_hi=[1.0, 1.0]), "must not exceed")):
        with pytest.raises(ValueError, match=match):
            plant.ilqr(*args, device_loop=True, **kw)
