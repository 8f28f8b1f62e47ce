"""The receding-horizon iLQR policy (`cimpc_plant_mpc`, `plant.ILQRPolicy`) without a device:
csrc/plant_mpc.h built with g++ against the NumPy index rules (`plant_mpc_cases`) exactly - the goal window below, at and past L, L = 1,
shifts 0, 1, H - 1, H and above, H = 1 -; the same program under AddressSanitizer and UBSan; `TrackingReference.window` against that build
row for row; every refusal that needs no device, each by its reason; the exports, their ctypes signatures and their Julia calls, by text;
and the Python classes' own refusals before the library is called.  tests/README_plant_mpc.md has the rest."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from contactimplicitmpc.jl_amd import _lib
import plant_mpc_cases as pmc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "plant_mpc_check.cpp")
INVALID = -1
HDR = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cimpc.h")).read(), flags=re.S)
JL = open(os.path.join(ROOT, "julia", "CIMPCHip.jl")).read()
NAMES = {"cimpc_plant_mpc_create": 34, "cimpc_plant_mpc_control": 13, "cimpc_plant_mpc_plan": 7, "cimpc_plant_mpc_reset": 2, "cimpc_plant_mpc_dims": 6,
         "cimpc_plant_mpc_destroy": 1}
JL_FUNCS = {"cimpc_plant_mpc_create": "plant_mpc_create", "cimpc_plant_mpc_control": "plant_mpc_control", "cimpc_plant_mpc_plan": "plant_mpc_plan",
            "cimpc_plant_mpc_reset": "plant_mpc_reset", "cimpc_plant_mpc_dims": "plant_mpc_dims", "cimpc_plant_mpc_destroy": "plant_mpc_destroy"}
CTYPE = {"int": C.c_int, "double": C.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int*": _lib._ip, "const int*": _lib._ip,
         "cimpc_plant_mpc": C.c_void_p, "const cimpc_terrain*": C.POINTER(_lib.Terrain), "const cimpc_ip_opts*": C.POINTER(_lib.IpOpts),
         "cimpc_plant_mpc*": C.POINTER(C.c_void_p)}
JL_COMPAT = {"Cint": {"int"}, "Cdouble": {"double"}, "Ptr{Cdouble}": {"const double*", "double*"}, "Ptr{Cint}": {"int*", "const int*"},
             "Ptr{Cvoid}": {"cimpc_plant_mpc"}, "Ptr{Terrain}": {"const cimpc_terrain*"}, "Ref{IpOpts}": {"const cimpc_ip_opts*"},
             "Ref{Ptr{Cvoid}}": {"cimpc_plant_mpc*"}, "Ref{Cint}": {"int*"}}
hx = lambda x: float(x).hex()


# ---- the header --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("mpc") / "plant_mpc_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-O1", "-o", exe, SRC])
    return exe


def run(exe, mode, text):
    res = subprocess.run([exe, mode], input=text + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout.strip().split("\n")


def ints(line):
    return np.array([int(v) for v in line.split()])


def doubles(line):
    return np.array([float.fromhex(v) for v in line.split()])


# (H, L): s + t below, at and past L; L = 1; H = 1; H above, equal to and below L
WINDOWS = ((14, 10), (1, 1), (1, 5), (5, 1), (4, 4), (3, 7), (8, 2))


def check_rows(exe):
    for H, L in WINDOWS:
        steps = sorted({0, 1, max(L - H - 1, 0), max(L - H, 0), max(L - H + 1, 0), L - 1, L, L + 1, L + H, 2 ** 31 - 1 - H, 2 ** 31 - 1})
        lines = run(exe, "rows", f"{H} {L} {len(steps)} " + " ".join(str(s) for s in steps))
        assert len(lines) == len(steps)
        for s, line in zip(steps, lines):
            got = ints(line)
            assert np.array_equal(got[:H + 1], pmc.x_rows(s, H, L)), (H, L, s)
            assert np.array_equal(got[H + 1:], pmc.u_rows(s, H, L)), (H, L, s)
            assert got[:H + 1].max() <= L and got[H + 1:].max() <= L - 1 and got.min() >= 0
    for H in (1, 2, 14):
        shifts = sorted({0, 1, max(H - 1, 0), H, H + 1, 3, 1000, 2 ** 31 - 1})
        lines = run(exe, "warm", f"{H} {len(shifts)} " + " ".join(str(s) for s in shifts))
        for shift, line in zip(shifts, lines):
            assert np.array_equal(ints(line), pmc.warm_rows(shift, H)), (H, shift)
        assert np.array_equal(ints(lines[0]), np.arange(H)), "shift 0 must leave the plan as it is"
        assert (ints(lines[shifts.index(H)]) == H - 1).all(), "shift H: every row the last"


def check_copies(exe, seed):
    rng = np.random.default_rng(seed)
    for H, L in WINDOWS:
        for n_x in (1, 3):
            n, m = 8, 2
            xr, ur = rng.standard_normal((L + 1, n_x, n)), rng.standard_normal((L, n_x, m))
            for s in (0, 1, L - 1, L, L + 3):
                text = f"{s} {H} {L} {n_x} {n} {m} " + " ".join(hx(v) for v in xr.ravel()) + " " + " ".join(hx(v) for v in ur.ravel())
                xg, ug = (doubles(line) for line in run(exe, "window", text))
                assert np.array_equal(xg.reshape(H + 1, n_x, n), xr[pmc.x_rows(s, H, L)]), (H, L, n_x, s)
                assert np.array_equal(ug.reshape(H, n_x, m), ur[pmc.u_rows(s, H, L)]), (H, L, n_x, s)
    for H, B, nu in ((14, 3, 2), (1, 1, 3), (2, 5, 1)):
        plan = rng.standard_normal((H, B, nu))
        for shift in (0, 1, H - 1, H, H + 4):
            got = doubles(run(exe, "shift", f"{shift} {H} {B} {nu} " + " ".join(hx(v) for v in plan.ravel()))[0])
            assert np.array_equal(got.reshape(H, B, nu), plan[pmc.warm_rows(shift, H)]), (H, B, nu, shift)
    assert run(exe, "reset", "5 0") == ["0 1"] and run(exe, "reset", "0 1") == ["0 1"]


def test_the_host_build_of_the_index_rules_is_numpy_exactly(host):
    check_rows(host)
    check_copies(host, 3)


def test_the_host_build_runs_clean_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "plant_mpc_check_san")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtimes: " + build.stderr[-300:])
    check_rows(exe)
    check_copies(exe, 4)
    for mode, text, _ in HEADER_REFUSALS:
        run(exe, mode, text)


def test_the_window_of_a_reference_is_the_header_build_row_for_row(host):
    from contactimplicitmpc.jl_amd import plant
    rng = np.random.default_rng(9)
    nq, nu, B = 4, 2, 3
    n, m = 2 * nq, nu
    for H, L in WINDOWS:
        for per_robot in (False, True):
            xr = rng.standard_normal((L + 1, B, n) if per_robot else (L + 1, n))
            ur = rng.standard_normal((L, m))      # shared beside per-robot x goals: spread as TrackingCost spreads it
            ref = plant.TrackingReference(np.eye(n), np.eye(m), x_ref=xr, u_ref=ur)
            xa, ua = ref._arrays(B)
            n_x = B if per_robot else 1
            assert xa.shape == (L + 1, n_x, n) and ua.shape == (L, n_x, m)
            for s in (0, 1, L - 1, L, L + 2):
                cost = ref.window(s, H)
                cc, (Qc, Rc, Qfc, xg, ug) = cost._struct(nq, nu, B, H)
                assert cc.n_x == n_x and xg.shape == (H + 1, n_x, n) and ug.shape == (H, n_x, m)
                text = f"{s} {H} {L} {n_x} {n} {m} " + " ".join(hx(v) for v in xa.ravel()) + " " + " ".join(hx(v) for v in ua.ravel())
                hxg, hug = (doubles(line) for line in run(host, "window", text))
                assert np.array_equal(hxg.reshape(xg.shape), xg) and np.array_equal(hug.reshape(ug.shape), ug), (H, L, per_robot, s)
    ref = plant.TrackingReference(np.eye(n), np.eye(m))      # the defaults: zeros with L = 1
    assert ref.L == 1 and ref.x_ref.shape == (2, n) and ref.u_ref.shape == (1, m) and not ref.x_ref.any()
    xi, ui = ref.rows(5, 3)
    assert xi.tolist() == [1, 1, 1, 1] and ui.tolist() == [0, 0, 0]


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------
nan, inf = float("nan"), float("inf")
HEADER_REFUSALS = (
    ("problem", "0 5 1", "H or L below 1"), ("problem", "5 0 1", "H or L below 1"), ("problem", "5 5 0", "n_iter below 1"), ("problem", "1 1 1", "ok"),
    ("step", "-1 0 1", "shift or s negative"), ("step", "0 -1 1", "shift or s negative"), ("step", "0 1 0", "a shift with no plan loaded"),
    ("step", "0 0 0", "a shift with no plan loaded"), ("step", "3 1 1", "ok"), ("step", "2147483647 2147483647 1", "ok"),
    ("state", f"2 {hx(1.0)} {hx(nan)} {hx(0.0)} {hx(0.0)}", "a non-finite entry of q0"),
    ("state", f"2 {hx(1.0)} {hx(2.0)} {hx(0.0)} {hx(-inf)}", "a non-finite entry of q1"),
    ("state", f"1 {hx(1.0)} {hx(2.0)}", "ok"),
    ("plan", f"1 1 2 0 {hx(1.0)} {hx(inf)}", "a non-finite entry of u0"),
    ("plan", f"1 1 2 1 {hx(1.0)} {hx(0.5)} {hx(-1.0)} {hx(-1.0)} {hx(1.0)} {hx(0.25)}", "an entry of u0 outside the limits"),
    ("plan", f"1 2 1 2 {hx(1.0)} {hx(-3.0)} {hx(-1.0)} {hx(-2.0)} {hx(1.0)} {hx(2.0)}", "an entry of u0 outside the limits"),
    ("plan", f"1 2 1 2 {hx(1.0)} {hx(-2.0)} {hx(-1.0)} {hx(-2.0)} {hx(1.0)} {hx(2.0)}", "ok"),
    ("plan", f"2 1 1 1 {hx(1.0)} {hx(-1.0)} {hx(-inf)} {hx(inf)}", "ok"),
)


@pytest.mark.parametrize("k", range(len(HEADER_REFUSALS)))
def test_the_headers_refusals_by_reason(host, k):
    mode, text, reason = HEADER_REFUSALS[k]
    assert run(host, mode, text) == [reason]


def _create(**change):
    """cimpc_plant_mpc_create on a small stand-in problem (hopper_2D, B 2, H 3, L 2) with `change` applied -> (rc, reason, handle value)."""
    nq, nu, B, H, L = 4, 2, 2, 3, 2
    n = 2 * nq
    a = dict(model=2, B=B, H=H, L=L, n_iter=2, ladder=[1e-6, 1e-5, 1e-4], tol=1e-6, rho_max=1e6, alpha=[1.0, 0.5], n_alpha=None, armijo=1e-4, h=0.01, n_Q=1, n_x=1,
             n_lim=1, u_lo=None, u_hi=None, u0=np.zeros((H, B, nu)), n_cols=2 * nq + nu, null=None, mu=[0.5], n_mu=1, handle=True)
    a.update(change)
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib._dp)
    Q, Qf, R, xr, ur = np.eye(n), np.eye(n), np.eye(nu), np.zeros((max(a["L"], 0) + 1, a["n_x"], n)), np.zeros((max(a["L"], 1), a["n_x"], nu))
    p = dict(mu=arr(a["mu"]), Q=Q, Qf=Qf, R=R, x_ref=xr, u_ref=ur, alpha=arr(a["alpha"]), ladder=arr(a["ladder"]), u0=arr(a["u0"]))
    opts = _lib.IpOpts()
    _lib.load().cimpc_default_ip_opts(C.byref(opts))
    po = C.byref(opts)
    if a["null"] == "opts":
        po = None
    elif a["null"]:
        p[a["null"]] = None
    lo, hi = arr(a["u_lo"]), arr(a["u_hi"])
    handle = C.c_void_p(0xdead)      # what a refusal must overwrite with NULL
    lib = _lib.load()
    n_alpha = (0 if p["alpha"] is None else p["alpha"].size) if a["n_alpha"] is None else a["n_alpha"]
    rc = lib.cimpc_plant_mpc_create(a["model"], a["B"], a["H"], 0, 0, None, dp(p["mu"]), a["n_mu"], a["h"], po, dp(p["Q"]), dp(p["Qf"]), dp(p["R"]), a["n_Q"], 1,
                                    a["L"], a["n_x"], dp(p["x_ref"]), dp(p["u_ref"]), n_alpha, dp(p["alpha"]), a["armijo"], 1e-9, a["n_cols"],
                                    0 if p["ladder"] is None else p["ladder"].size, dp(p["ladder"]), a["rho_max"], a["tol"], a["n_iter"], a["n_lim"], dp(lo), dp(hi),
                                    dp(p["u0"]), C.byref(handle) if a["handle"] else None)
    return rc, lib.cimpc_last_error(None).decode(), handle.value


REFUSED = {
    "H 0": (dict(H=0), "H or L below 1"),
    "L 0": (dict(L=0), "H or L below 1"),
    "n_iter 0": (dict(n_iter=0), "n_iter below 1"),
    "a short ladder": (dict(n_iter=3), "a ladder shorter than max_iter + 1"),
    "a negative ladder entry": (dict(ladder=[1e-6, -1e-5, 1e-4]), "a ladder entry that is negative or not finite"),
    "a NaN tol": (dict(tol=nan), "rho_max or tol not a number"),
    "null ladder": (dict(null="ladder"), "null ladder"),
    "null u0": (dict(null="u0"), "null u0"),
    "null x_ref": (dict(null="x_ref"), "null x_ref"),
    "null opts": (dict(null="opts"), "null opts"),
    "null mu": (dict(null="mu"), "null mu"),
    "an unknown model": (dict(model=99), "an unknown model"),
    "B 0": (dict(B=0), "B below 1"),
    "n_alpha 65": (dict(n_alpha=65), "n_alpha outside 1 .. 64"),
    "an infinite alpha": (dict(alpha=[1.0, inf]), "a non-finite alpha"),
    "a negative armijo": (dict(armijo=-1.0), "armijo negative or not a number"),
    "n_Q 0": (dict(n_Q=0), "n_Q, n_R or n_x of the cost below 1"),
    "n_Q 2": (dict(n_Q=2), "n_Q of the cost neither 1 nor T"),
    "n_x 3": (dict(n_x=3), "n_x of the cost neither 1 nor B"),
    "h 0": (dict(h=0.0), "h not positive"),
    "u_lo alone": (dict(u_lo=[[-1.0, -1.0]]), "one of u_lo, u_hi without the other"),
    "n_lim 3": (dict(u_lo=[[-1.0, -1.0]], u_hi=[[1.0, 1.0]], n_lim=3), "n_lim neither 1 nor B"),
    "u_lo above u_hi": (dict(u_lo=[[2.0, -1.0]], u_hi=[[1.0, 1.0]]), "u_lo above u_hi"),
    "a NaN limit": (dict(u_lo=[[nan, -1.0]], u_hi=[[1.0, 1.0]]), "a NaN limit"),
    "too few columns": (dict(n_cols=9), "an argument that cimpc_plant_rollout_tape refuses for the tape's B robots"),
    "a non-finite u0": (dict(u0=np.full((3, 2, 2), nan)), "a non-finite entry of u0"),
    "u0 outside the limits": (dict(u_lo=[[-1.0, -1.0]], u_hi=[[1.0, 1.0]], u0=np.full((3, 2, 2), 1.5)), "an entry of u0 outside the limits"),
    "n_mu 3": (dict(n_mu=3, mu=[0.5, 0.5, 0.5]), "an argument that cimpc_plant_rollout_tape refuses for the tape's B robots"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_create_refuses_by_reason_without_a_device_and_leaves_no_handle(what):
    change, reason = REFUSED[what]
    rc, why, handle = _create(**change)
    assert rc == INVALID
    assert why == "cimpc_plant_mpc_create: " + reason
    assert handle is None, "*handle must be NULL after a refusal"


def test_a_null_handle_is_refused_first_and_by_every_entry():
    lib = _lib.load()
    rc, why, _ = _create(handle=False, H=0)
    assert rc == INVALID and why == "cimpc_plant_mpc_create: null handle"
    some = np.zeros(8)
    somei = np.zeros(8, dtype=np.int32)
    D, I = some.ctypes.data_as(_lib._dp), somei.ctypes.data_as(_lib._ip)
    n_done = C.c_int(-7)
    assert lib.cimpc_plant_mpc_control(None, 0, 0, D, D, D, D, D, D, D, I, C.byref(n_done), I) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_mpc_control: null handle"
    assert n_done.value == -7 and not some.any() and not somei.any(), "a refusal wrote to an output"
    assert lib.cimpc_plant_mpc_plan(None, D, None, None, None, None, None) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_mpc_plan: null handle"
    assert lib.cimpc_plant_mpc_reset(None, D) == INVALID
    assert lib.cimpc_last_error(None).decode() == "cimpc_plant_mpc_reset: null handle"
    assert lib.cimpc_plant_mpc_dims(None, I, I, I, I, I) == INVALID
    assert lib.cimpc_plant_mpc_destroy(None) == 0
    assert not some.any() and not somei.any()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", HDR, flags=re.S)
    assert m, f"{name} is not declared in include/cimpc.h"
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_the_exports_are_declared_and_bound(name):
    params = _prototype(name)
    assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(params) == NAMES[name]
    assert [CTYPE[p] for p in params] == args
    assert hasattr(_lib.load(), name)


def test_the_source_is_built_and_the_loop_body_exists_once():
    csrc = os.path.join(ROOT, "contactimplicitmpc", "jl_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "plant_mpc.hip" in make and "plant_mpc.h " in make
    src = open(os.path.join(csrc, "plant_mpc.hip")).read()
    for name in NAMES:
        assert f'extern "C" int {name}(' in src
    assert '#include "plant_mpc.h"' in src and "asm" not in src and "__builtin" not in src
    assert "plant_mpc_begin_kernel" in src and "plant_mpc_nominal_kernel" in src and "plant_cost_trajectory" in src and "PlantCostWave" in src
    assert "plant_step_kernel" not in src, "no new instantiation of the step kernel"
    ilqr = open(os.path.join(csrc, "plant_ilqr.hip")).read()
    for text in (src, ilqr):      # both entries call the one body; neither launches its kernels itself
        assert "plant_ilqr_iteration(" in text
    assert src.count("plant_riccati_box_launch") == 0 and src.count("plant_linesearch_stages") == 0
    assert ilqr.count("plant_riccati_box_launch(") == 1 and ilqr.count("plant_linesearch_stages(") == 1
    # a control step: no allocation and one read per iteration inside the loop
    control = src[src.index('extern "C" int cimpc_plant_mpc_control('):src.index('extern "C" int cimpc_plant_mpc_plan(')]
    assert "hipMalloc" not in control
    loop = control[control.index("for (int it = 0; it < n_iter"):control.index("plant_mpc_converged_kernel")]
    assert loop.count("down(") == 1 and "up(" not in loop and "plant_grow" not in loop


@pytest.mark.parametrize("name", sorted(NAMES))
def test_julia_calls_match_the_prototypes(name):
    fname = JL_FUNCS[name]
    assert f"function {fname}(" in JL, f"julia/CIMPCHip.jl has no {fname}"
    fn = JL[JL.index(f"function {fname}("):]
    fn = fn[:fn.index("\nend\n") + 5]
    m = re.search(r"@ccall LIB\." + name + r"\((.*?)\)::Cint", fn, flags=re.S)
    assert m, f"{fname} does not call {name}"
    types = [a.rsplit("::", 1)[1].strip() for a in m.group(1).split(",")]
    params = _prototype(name)
    assert len(types) == len(params), f"{len(types)} Julia arguments, {len(params)} C parameters"
    for k, (jt, ct) in enumerate(zip(types, params)):
        assert ct in JL_COMPAT[jt], f"argument {k}: Julia {jt} against C `{ct}`"
    doc = JL[:JL.index(f"function {fname}(")][-3000:]
    assert "unexecuted" in doc.lower(), "the docstring must say that the Julia call has not been run"


# ---- the Python classes --------------------------------------------------------------------------------------------------------------------------
def test_python_refuses_wrong_shapes_before_the_library_is_called(monkeypatch):
    from contactimplicitmpc.jl_amd import plant
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    nq, nu, B, H = 4, 2, 3, 5
    n = 2 * nq
    good = plant.TrackingReference(np.eye(n), np.eye(nu), x_ref=np.zeros((4, n)))
    for kw, match in ((dict(x_ref=np.zeros((4, n + 1))), "x_ref must be"), (dict(x_ref=np.zeros((1, n))), "x_ref must be"),
                      (dict(u_ref=np.zeros((3, nu + 1))), "u_ref must be"), (dict(x_ref=np.zeros((4, n)), u_ref=np.zeros((4, nu))), "u_ref must have")):
        with pytest.raises(ValueError, match=match):
            plant.TrackingReference(np.eye(n), np.eye(nu), **kw)
    with pytest.raises(ValueError, match="Q must be"):
        plant.TrackingReference(np.eye(n)[0], np.eye(nu))
    with pytest.raises(ValueError, match="negative"):
        good.window(-1, H)
    a = dict(model="hopper_2D", B=B, H=H, h=0.01, mu=0.5, ref=good, u0=np.zeros((H, nu)))
    for change, match in ((dict(u0=np.zeros((H, nu + 1))), "u0 must be"), (dict(u0=np.zeros((H + 1, nu))), "u0 must be"), (dict(u0=np.zeros((H, 2, nu))), "u0 must be"),
                          (dict(u0=np.full((H, nu), np.nan)), "finite"), (dict(H=0), "B and H"), (dict(B=0), "B and H"), (dict(ref=None), "TrackingReference"),
                          (dict(h=0.0), "h must be"), (dict(mu=[0.5, 0.5]), "mu:"), (dict(n_iter=0), "max_iter"), (dict(alphas=()), "alphas"),
                          (dict(armijo=-1.0), "armijo"), (dict(rho0=-1e-6), "rho0"), (dict(tol=np.nan), "rho_max and tol"), (dict(u_lo=[-1.0, -1.0]), "go together"),
                          (dict(u_lo=[2.0, 0.0], u_hi=[1.0, 1.0]), "must not exceed"), (dict(grad_cols=3), "grad_cols"),
                          (dict(ref=plant.TrackingReference(np.eye(3), np.eye(nu))), "TrackingCost"),
                          (dict(ref=plant.TrackingReference(np.eye(n), np.eye(nu), x_ref=np.zeros((4, 2, n)))), "robots"),
                          (dict(ref=plant.TrackingReference(np.zeros((H + 1, n, n)), np.eye(nu))), "TrackingCost")):
        kw = dict(a, **change)
        with pytest.raises(ValueError, match=match):
            plant.ILQRPolicy(kw.pop("model"), kw.pop("B"), kw.pop("H"), kw.pop("h"), kw.pop("mu"), kw.pop("ref"), kw.pop("u0"), **kw)


def test_control_refuses_wrong_states_before_the_library_is_called():
    """A policy whose handle is a stand-in: `control`, `reset` and `__call__` refuse from shapes and values alone."""
    from contactimplicitmpc.jl_amd import plant

    class Lib:
        def __getattr__(self, name):
            raise AssertionError("the library was called")
    pol = object.__new__(plant.ILQRPolicy)
    pol._handle, pol._lib, pol.B, pol.H, pol.h, pol.n_iter, pol._dims, pol._lo, pol._hi = object(), Lib(), 3, 5, 0.01, 1, (4, 2, 1, 2), None, None
    pol.s, pol._fresh, pol._prev, pol.last = 0, True, None, None
    q = np.zeros((3, 4))
    for args, kw, match in (((np.zeros((3, 5)), q), {}, "q1 and v1"), ((q, np.zeros((2, 4))), {}, "q1 and v1"), ((q, q), dict(shift=-1), "shift"),
                            ((np.full((3, 4), np.inf), q), {}, "finite"), ((q, np.full((3, 4), np.nan)), {}, "finite")):
        with pytest.raises(ValueError, match=match):
            pol.control(*args, **kw)
    with pytest.raises(ValueError, match="start"):
        pol(q)
    with pytest.raises(ValueError, match="u0 must be"):
        pol.reset(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="negative"):
        pol.reset(s=-1)
    assert pol.s == 0 and pol._fresh, "a refusal changed the policy"
    pol._handle = None
    with pytest.raises(ValueError, match="closed"):
        pol.control(q, q)
